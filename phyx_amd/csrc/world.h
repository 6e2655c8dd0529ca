// world.h — World: the whole step of ref: src/World.cpp:19-37 on HBM-resident arrays, and every call between steps.
//
// Bodies live on the device as the RESIDENT structure of arrays (body_view.h: velocities, displacing velocities,
// {invMass, invInertia, pos}, frame, AABB, size — every kernel of the step reads the 16-byte granules it needs, coalesced);
// the reference's 128-byte records exist at the C-ABI edge only (construction, phx_world_get_bodies).  Manifolds / contact
// points / joints live on the device in the reference's POD layouts; the host keeps only their counts.
//
// One class, one translation unit per concern: world.hip (construction, the upload, the step), world_state.hip, world_edit.hip,
// world_units.hip, world_query.hip and c_api_world.hip (DESIGN.md §5b has the table).  A member template is defined in the one file
// that holds all its uses, or instantiated there explicitly; no kernel is launched from two of them.
#pragma once
#include "reslab.h"
#include "handles.h"
#include "world_kernels.h"
#include "query.h"
#include "contact.h"
#include "snapshot.h"
#include "pins.h"
#include "fields.h"
#include "exclusions.h"
#include "sweep.h"

#include <algorithm>
#include <cmath>

namespace phx {

inline int wgrid(int n) { return std::max(1, std::min(div_up(n, 256), 4096)); }      // (the removal's streaming passes take listing.h's stream_grid)

// ref: World.cpp:11-17, RigidBody.h:15-36: the record AddBody makes, index aside (world.hip; add_body and add_bodies both build from it)
phx_rigid_body body_record(float px, float py, float angle, float sx, float sy);

// The pinned staging of the between-step batches (edits, gathers, spawns, queries, unit fields).  A batch is {indices | values} in ONE
// H2D copy on the world's stream: the indices (if any) padded to 16 bytes in front of the values (if any).  The pinned buffer is
// bump-allocated while earlier batches' copies are still queued (they may sit behind a step in flight) and reused from the start once
// the event behind the last copy has passed; it starts at 64 KB and doubles.  An outgrown pinned buffer and an outgrown device batch
// are KEPT until the world goes: a queued copy or scatter may still read them.
class BatchStage {
public:
    BatchStage() = default;
    BatchStage(const BatchStage&) = delete;
    BatchStage& operator=(const BatchStage&) = delete;
    // the values alone / the indices alone / (indexed, below) `count` indices with `width` floats each: the device pointers of what was staged
    int values(const float* values, int count, int width, hipStream_t stream, const float** d_values)
    {
        const int* none = nullptr;
        return indexed(nullptr, values, count, width, stream, &none, d_values);
    }
    int indices(const int* indices, int count, hipStream_t stream, const int** d_indices)
    {
        const float* none = nullptr;
        return indexed(indices, nullptr, count, 0, stream, d_indices, &none);
    }
    // The pinned buffers and the event go.  Called by the owner with its device current and its stream drained (~World), and by no
    // destructor: a world that cannot select its device frees nothing.  (The device batches are DevBufs: freed with the object.)
    void release()
    {
        for (char* p : retired_) (void)hipHostFree(p);
        if (pin_) (void)hipHostFree(pin_);
        if (done_) (void)hipEventDestroy(done_);
        retired_.clear(); pin_ = nullptr; cap_ = 0; used_ = 0; done_ = nullptr;
    }
    int indexed(const int* indices, const float* values, int count, int width, hipStream_t stream, const int** d_indices, const float** d_values)
    {
        const size_t ib = indices ? ((size_t)count * sizeof(int) + 15) & ~size_t(15) : 0, bytes = ib + (size_t)count * (size_t)width * sizeof(float);
        if (!done_) PHX_HIP(hipEventCreateWithFlags(&done_, hipEventDisableTiming));
        else if (used_) {
            const hipError_t q = hipEventQuery(done_);
            if (q == hipSuccess) used_ = 0;
            else if (q != hipErrorNotReady) { set_error("staging: %s", hipGetErrorString(q)); return PHX_ERR_HIP; }
        }
        size_t off = (used_ + 15) & ~size_t(15);
        if (off + bytes > cap_) {
            const size_t cap = std::max<size_t>(std::max<size_t>(2 * bytes, 2 * cap_), 64u << 10);
            if (pin_) retired_.push_back(pin_);
            pin_ = nullptr; cap_ = 0;
            PHX_HIP(hipHostMalloc(reinterpret_cast<void**>(&pin_), cap, hipHostMallocDefault));
            cap_ = cap;
            off = 0;
        }
        if (bytes > dev_.cap && dev_.p) dev_retired_.push_back(std::move(dev_));
        PHX_TRY(dev_.reserve(bytes));
        if (indices) std::memcpy(pin_ + off, indices, (size_t)count * sizeof(int));
        if (width) std::memcpy(pin_ + off + ib, values, bytes - ib);
        PHX_HIP(hipMemcpyAsync(dev_.p, pin_ + off, bytes, hipMemcpyHostToDevice, stream));
        PHX_HIP(hipEventRecord(done_, stream));
        used_ = off + bytes;
        *d_indices = indices ? reinterpret_cast<const int*>(dev_.p) : nullptr;
        *d_values = reinterpret_cast<const float*>(dev_.p + ib);
        return PHX_OK;
    }

private:
    char* pin_ = nullptr; size_t cap_ = 0, used_ = 0;      // bump-allocated while copies are pending
    hipEvent_t done_ = nullptr;                 // recorded behind the last batch's copy: once it has passed, the pinned buffer is free again
    std::vector<char*> retired_;                // outgrown pinned buffers a pending copy may still read
    DevBuf<char> dev_;                          // the batch on the device (stream order protects it from the next batch's copy)
    std::vector<DevBuf<char>> dev_retired_;     // outgrown device batches a pending scatter may still read
};

// What every body always has on the device: the 128-byte records (the C-ABI edge: uploaded once, refreshed from the resident arrays only
// when a getter asks) and the six resident arrays every kernel of the step reads (body_view.h).  The World holds two: the live one and
// the spare a removal compacts into, which then change places.
struct BodyStore {
    DevBuf<phx_rigid_body> records;
    DevBuf<float4> vel, dvel, mpos, frame, aabb;
    DevBuf<float2> size;
    int reserve(size_t n)
    {
        PHX_TRY(records.reserve(n));
        PHX_TRY(vel.reserve(n)); PHX_TRY(dvel.reserve(n)); PHX_TRY(mpos.reserve(n)); PHX_TRY(frame.reserve(n)); PHX_TRY(aabb.reserve(n));
        return size.reserve(n);
    }
    int reserve_keep(size_t total, size_t keep, hipStream_t stream)      // geometric, contents kept; a buffer that grows waits for the stream once
    {
        PHX_TRY(records.reserve_keep(total, keep, stream));
        PHX_TRY(vel.reserve_keep(total, keep, stream)); PHX_TRY(dvel.reserve_keep(total, keep, stream)); PHX_TRY(mpos.reserve_keep(total, keep, stream));
        PHX_TRY(frame.reserve_keep(total, keep, stream)); PHX_TRY(aabb.reserve_keep(total, keep, stream));
        return size.reserve_keep(total, keep, stream);
    }
    WorldBodies view() const { return WorldBodies{BodyView{vel.p, dvel.p, mpos.p}, frame.p, aabb.p, size.p}; }
};

// An optional per-body column (world_kernels.h FilterColumn, MaterialColumn) through the bodies' life.  `active` is conservative: it is
// set by the first value anybody sets and stays set when every value has gone back to the default (that costs time only); while it is
// clear there is no table and every body has the default.  While the bodies are host-staged `host` is the truth and goes up with them,
// otherwise `dev`, which grows with a spawn and is compacted into `spare` by a removal, beside the body store.
template <class Column>
struct BodyTable {
    using column = Column;
    using T = typename Column::value;
    bool active = false;
    DevBuf<T> dev, spare;
    std::vector<T> host;

    T* ptr() const { return active ? dev.p : nullptr; }
    T* spare_ptr() const { return active ? spare.p : nullptr; }
    void reset() { active = false; host.clear(); }                          // every body has the default again
    void push_default() { if (active) host.push_back(Column::initial()); }  // add_body
    int grow(size_t total, size_t keep, hipStream_t stream) { return active ? dev.reserve_keep(total, keep, stream) : PHX_OK; }
    int reserve_spare(size_t n) { return active ? spare.reserve(n) : PHX_OK; }
    void adopt_spare() { if (active) std::swap(dev, spare); }
    // the bodies become host-staged: so does the table
    int to_host(int n, int device, hipStream_t stream)
    {
        if (!active) return PHX_OK;
        host.resize((size_t)n);
        if (!n) return PHX_OK;
        PHX_TRY(use_device(device));
        PHX_HIP(hipStreamSynchronize(stream));
        PHX_HIP(hipMemcpy(host.data(), dev.p, (size_t)n * sizeof(T), hipMemcpyDeviceToHost));
        return PHX_OK;
    }
    // ... and goes up with them again (the caller waits for the stream, then clears `host`)
    int upload(size_t n, hipStream_t stream)
    {
        if (!active) return PHX_OK;
        PHX_TRY(dev.reserve(n));
        if (!host.empty()) PHX_HIP(hipMemcpyAsync(dev.p, host.data(), host.size() * sizeof(T), hipMemcpyHostToDevice, stream));
        return PHX_OK;
    }
    // a batch of values for `n` host-staged bodies / a staged batch scattered on the stream; the first one makes the table
    void set_host(const int32_t* bodies, const typename Column::api* values, int count, int n)
    {
        if (!active) host.assign((size_t)n, Column::initial());
        active = true;
        for (int k = 0; k < count; ++k) host[(size_t)bodies[k]] = Column::stored(values[k]);
    }
    int set_device(const int* d_bodies, const float* d_values, int count, int n, hipStream_t stream)
    {
        if (!active) {
            PHX_TRY(dev.reserve((size_t)std::max(n, 1)));
            hipLaunchKernelGGL(k_fill_column<Column>, dim3(wgrid(n)), dim3(256), 0, stream, dev.p, n);
            active = true;
        }
        hipLaunchKernelGGL(k_scatter_column<Column>, dim3(wgrid(count)), dim3(256), 0, stream, d_bodies, reinterpret_cast<const typename Column::api*>(d_values), count, dev.p);
        PHX_HIP(hipGetLastError());
        return PHX_OK;
    }
    // f(i, value) for every body, from wherever the truth is
    template <class F> int visit(int n, bool host_staged, int device, Readback& rb, hipStream_t stream, F f)
    {
        std::vector<T> tmp;
        const T* src = host.data();
        if (active && !host_staged && n) {
            PHX_TRY(use_device(device));
            tmp.resize((size_t)n);
            PHX_TRY(rb.add(tmp.data(), dev.p, (size_t)n * sizeof(T), stream));
            PHX_TRY(rb.wait(stream));
            src = tmp.data();
        }
        for (int i = 0; i < n; ++i) f(i, active ? src[i] : Column::initial());
        return PHX_OK;
    }
};

class World {
public:
    explicit World(int device) : broadphase_h(device), solver_h(device), device_(device), broadphase_(broadphase_h.impl), solver_(solver_h.impl) {}
    ~World();
    int init();

    int add_body(float px, float py, float angle, float sx, float sy);
    int add_bodies(const float* spawn, int count, int* first);      // phx_world_add_bodies
    int set_static(int body);
    int set_inverse_mass(int body, float inv_mass, float inv_inertia);
    int synchronize();
    int update(float dt, const phx_config& cfg);
    int pre_solve(float dt);
    int finish_step(float dt, const phx_config& cfg);
    int step_begin(float dt, const phx_config& cfg, size_t* segment_bytes);
    int step_end(float dt);
    int set_comm(Comm* c);
    int step_sharded(float dt, const phx_config& cfg);
    int step_sharded_inner(float dt, const phx_config& cfg);
    int check_exchange();
    int x_extent(float out[2]);
    hipStream_t stream() const { return stream_; }
    int download_bodies(phx_rigid_body* out, int cap);
    int download_manifolds(phx_manifold* out, int cap);
    int download_contact_points(phx_contact_point* out, int cap);
    int download_joints(phx_contact_joint* out, int cap);
    int set_state(const phx_rigid_body* bodies, int body_count, const phx_manifold* manifolds, int manifold_count,
                  const phx_contact_point* cps, int cp_count, const phx_contact_joint* joints, int joint_count);
    int get_slab_state(const long long* global_index, int count, SlabState* out);      // this world as a re-slab hands it over (reslab.h)
    // snapshots (phx_world_save / phx_world_load): between steps; the whole state stays in HBM
    int save(Snapshot& s);
    int load(Snapshot& s);
    // edits and gathers between steps (phx_world_add_accelerations ... phx_world_get_poses_device)
    enum Edit { EDIT_ACCELERATIONS, EDIT_VELOCITIES, EDIT_POSES };
    int edit(Edit kind, const int* bodies, const float* values, int count);
    int set_inverse_masses(const int* bodies, const float* values, int count);      // phx_world_set_inverse_masses
    int get_body_states(const int* bodies, int count, phx_rigid_body* out);
    int get_poses(float* out, int cap);
    int get_poses_device(void* d_out, int cap);
    // removal between steps (phx_world_remove_bodies / phx_world_remove_outside): the listed bodies, or (`box` non-null) every body
    // whose AABB does not overlap the box
    int remove(const char* what, const int* bodies, int count, const float* box, int* removed, int* remap);
    // queries (phx_world_query_aabb ... phx_world_raycast_device): any time, nothing changes
    int query_aabb(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total);
    int query_points(const float* points, int count, int flags, int32_t* body);
    int raycast(const float* rays, int count, int flags, phx_ray_hit* out);
    int query_points_device(const void* d_points, int count, int flags, void* d_body);
    int raycast_device(const void* d_rays, int count, int flags, void* d_out);
    int query_boxes(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total);
    int cast_boxes(const float* casts, int count, int flags, phx_shape_hit* out);
    int cast_boxes_device(const void* d_casts, int count, int flags, void* d_out);
    int query_circles(const float* circles, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total);
    int cast_circles(const float* casts, int count, int flags, phx_shape_hit* out);
    int cast_circles_device(const void* d_casts, int count, int flags, void* d_out);
    int query_nearest(const float* queries, int count, int flags, phx_near_hit* out);
    int query_nearest_device(const void* d_queries, int count, int flags, void* d_out);
    int query_index_build();            // the query index alone, built unless current (tools/query_cost.py)
    int query_index_builds() const { return query_.index_builds(); }
    // contact reports (phx_world_query_contacts ... phx_world_contact_index): between steps; only the events' baseline changes
    int query_contacts(const int32_t* bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap, int64_t* total);
    int contact_events(int32_t* begin, int begin_cap, int64_t* begin_total, int32_t* end, int end_cap, int64_t* end_total);
    int contact_markers_device(void* d_out, int cap);
    int contact_index_build();           // the contact index alone, built unless current (tools/contact_cost.py)
    int contact_index_builds() const { return contacts_.index_builds(); }
    // collision filters (phx_world_set_collision_filters / get_collision_filters): between steps; a change that makes pairs fail drops
    // their manifolds as set_state of the dropped state would
    int set_collision_filters(const int32_t* bodies, const phx_collision_filter* filters, int count, int* dropped);
    int get_collision_filters(phx_collision_filter* out, int cap);
    // collision exclusions (phx_world_add_collision_exclusions ... get_collision_exclusions): between steps; an add drops the manifolds
    // of the pairs it excludes as a change of filters would
    int add_collision_exclusions(const int32_t* pairs, int count, int* dropped);
    int remove_collision_exclusions(const int32_t* pairs, int count);
    int clear_collision_exclusions();
    int get_collision_exclusions(int32_t* out, int cap, int32_t* count) const;
    // materials (phx_world_set_materials / get_materials): between steps; they change no topology
    int set_materials(const int32_t* bodies, const phx_material* materials, int count);
    int get_materials(phx_material* out, int cap);
    // body flags (phx_world_set_body_flags / get_body_flags): between steps; the joints of a sensor go or come at the next step's refresh
    int set_body_flags(const int32_t* bodies, const uint32_t* flags, int count);
    int get_body_flags(uint32_t* out, int cap);
    // shapes (phx_world_set_shapes / get_shapes): between steps; the kind and the half extents of a body, the AABB recomputed
    int set_shapes(const int32_t* bodies, const phx_shape* shapes, int count);
    int get_shapes(phx_shape* out, int cap);
    // polygons (phx_world_set_polygons / get_polygons): the fourth kind; the record, the frame box and the AABB
    int set_polygons(const int32_t* bodies, const phx_polygon* polygons, int count);
    int get_polygons(const int32_t* bodies, phx_polygon* out, int count);
    int queue_shapes(const int32_t* bodies, const phx_shape* shapes, int count, bool kinds);
    int queue_polygons(const int32_t* bodies, const phx_polygon* polygons, int count);
    // continuous bodies (phx_world_set_continuous ... phx_world_sweep_counts): between steps; the pass runs behind IntegratePosition (sweep.h)
    int set_continuous(const int32_t* bodies, const float* radii, int count);
    int get_continuous(float* out, int cap);
    int sweep_hits(phx_sweep_hit* out, int cap, int64_t* total);
    int sweep_counts(int64_t* passes, int64_t* clamps_total);
    int sweep_timing(int enable, double* last_pass_ms);
    template <class Column> int get_table(const char* what, BodyTable<Column>& table, typename Column::api* out, int cap);
    // units: pins, links, angles and sliders, `P` = phx_pin, phx_link, phx_angle or phx_slider (phx_world_add_pins ... phx_world_get_sliders, phx_world_get_pin_schedule): between
    // steps; solved at the end of pre_solve (pins.h)
    template <class P> int add_units(const P* recs, int count, int* first);
    template <class P> int remove_units(const int32_t* which, int count);
    template <class P> int set_unit_anchors(const int32_t* which, const float* anchors, int count);
    template <class P> int get_units(P* out, int cap);
    int set_link_lengths(const int32_t* which, const float* lengths, int count);
    template <class P> int set_unit_limits(const int32_t* which, const float* limits, int count);      // (`P`: phx_angle or phx_slider)
    template <class P> int set_unit_motors(const int32_t* which, const float* motors, int count);
    template <class P> int unit_count(int* out);
    int set_pin_iterations(int n);
    int pin_schedule(const Schedule** out);
    // breaks (phx_world_set_break_limits, get_break_limits, break_events): between steps
    int set_break_limits(int kind, const int32_t* which, const float* limits, int count);
    int get_break_limits(int kind, float* out, int cap);
    int break_events(phx_break_event* out, int cap, int64_t* total);
    // sleeping (phx_world_set_sleeping ... phx_world_sleep_counts): between steps; the pass runs at the end of finish_step (sleep.h)
    int set_sleeping(const phx_sleep_params* p);
    int get_sleeping(phx_sleep_params* out, int32_t* enabled) const;
    int get_sleep_states(phx_sleep_state* out, int cap);
    int wake_bodies(const int32_t* bodies, int count);
    int sleep_counts(int32_t* asleep, int64_t* slept_total, int64_t* woken_total);
    int set_gravity(float g);
    // force fields (phx_world_set_fields ... phx_world_field_passes): between steps; the pass runs at the head of pre_solve (fields.h)
    int set_fields(const phx_field* fields, int count);
    int get_fields(phx_field* out, int cap, int32_t* count) const;
    int pulse_fields(const phx_field* fields, int count);
    int apply_impulses(const int* bodies, const float* impulses, int count);
    long long field_passes() const { return fields_.passes(); }
    PinSet& pins() { return pins_; }
    // what the sharded modes (phx_world_set_shard, set_comm, reslab) do not carry: PHX_ERR_STATE while the world holds a unit, sleeping, a
    // value in an optional column that is not the default, (`fields`) a force field, or a collision exclusion
    int refuse_unsharded_state(const char* what, bool fields);

    int nb() const { return (int)host_bodies_.size(); }
    int nm = 0, nj = 0;
    float gravity = 0.f;      // (written through set_gravity)
    int shard = 0, shard_count = 1;
    double phase_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool phase_timing = false;          // per-phase host timers: one stream synchronisation per phase, off by default
    int dropped_points = 0;
    long long deferred_packs = 0, deferred_pack_retries = 0;      // PackManifolds counts settled with the joint counts / of those, the ones that found dead manifolds
    phx_broadphase broadphase_h;     // world-owned handles, also reachable through phx_world_broadphase()/phx_world_solver()
    phx_solver solver_h;
    DeviceBroadphase& broadphase() { return broadphase_; }
    DeviceSolver& solver() { return solver_; }

private:
    int sync_bodies_to_device();
    int refresh_records();               // resident arrays -> the 128-byte records (getters)
    WorldBodies resident() const { return bodies_.view(); }
    WorldBodies query_view() const { WorldBodies w = bodies_.view(); w.sleep = sleep_col_.ptr(); w.kinds = shapes_.ptr(); w.capsules = capsules() ? 1u : 0u; w.polys = polygons() ? polys_.ptr() : nullptr; return w; }      // (to a query a sleeper is not static, and a circle is a disc)
    bool host_staged() const { return bodies_dirty_ || !bodies_.records.p; }      // the host-staged records are the world
    int restage_on_host();               // ... again, after the device copy was: records and tables come down
    int refuse_mid_step(const char* what) const;      // PHX_ERR_STATE between pre_solve / step_begin and finish_step / step_end
    int refuse_sharded(const char* what, const char* plural) const;      // PHX_ERR_STATE: a sharded world carries no columns and no units
    int settle_on_device();              // this world's device is current and a pending solve settled: what a call queues goes behind it, never under a replay
    // ... and the other settle: DeviceSolver::synchronize() whether or not a solve is pending (it also collects the pending stats: a host
    // wait), then host-staged bodies go up as the next step would take them
    int settle_and_upload();
    int update_pairs();
    bool fuse_velocity_ = false; float step_dt_ = 0.f;      // IntegrateVelocity rides on the broadphase's key build (update_pairs)
    int fresh_manifolds_ = 0;           // pairs UpdatePairs found this step: their manifolds are created by UpdateManifolds' kernel
    int manifolds_updated_ = 0;         // manifolds [0, this) were updated during update_pairs' round trip (update_manifolds() does the rest)
    int update_manifolds();
    void queue_update_manifolds(int first, int nm_old, const uint2* new_pairs, const MailRide& ride);
    int finish_pack(int dead, int dropped);
    int pack_manifolds();
    int refresh_contact_joints();
    int solve(const phx_config& cfg, bool settle);
    int solve_and_integrate(float dt, const phx_config& cfg);
    int scratch_for(int n);
    int forget_step_history();           // the bookkeeping a restored or compacted contact cache starts without
    int snapshot_guard(const char* what, const Snapshot& s) const;      // the refusals save and load share
    SnapshotWorld snapshot_view();       // the world's arrays as a save reads them / a load writes them

    int device_;
    DeviceBroadphase& broadphase_;
    DeviceSolver& solver_;
    hipStream_t stream_ = nullptr;
    std::vector<phx_rigid_body> host_bodies_;     // construction-time staging; the device copy is authoritative after upload (then only its size counts)
    bool bodies_dirty_ = false;
    BodyStore bodies_;
    bool records_stale_ = false;                  // a step has run since the records were last refreshed
    DevBuf<float4> accel_; bool accel_pending_ = false;      // accelerations the uploaded records came with: consumed by the next IntegrateVelocity
    DevBuf<phx_manifold> d_manifolds_;
    DevBuf<phx_contact_point> d_cps_;
    DevBuf<phx_contact_joint> d_joints_;
    DevBuf<unsigned> flags_, dead_flags_, counters_, joint_seen_;      // joint_seen_[j] == joint_epoch_: a contact point re-attached joint j this step
    DevBuf<unsigned> pack_flags_;       // dead-manifold flags, then their scan (a table of its own: the joint match reuses flags_ while the pack may still be pending)
    // PackManifolds' count is not waited for when the previous step found no dead manifold (the steady state of a stack): the
    // joint match is queued behind the scan on the assumption that nothing dies, both counts come back in ONE round trip, and
    // only if a manifold did die is the pack run then and the match repeated (a new epoch makes the first one void)
    bool pack_pending_ = false, expect_no_dead_manifolds_ = false;
    unsigned joint_epoch_ = 0;
    bool packed_this_step_ = false;          // PackManifolds moved manifolds in this step
    const MailRide* old_ride_ = nullptr;     // update_pairs: the post the old manifolds' UpdateManifolds launch carries
    ScanScratch scan_tiles_;     // counters_: [0] new joints, [1] dead joints, [2] dead manifolds, [3] dropped points
    Readback rb_;
    bool joints_changed_ = true;          // joints were created / destroyed (or a body's mass changed) since the last solve
    DevBuf<int> mover_pos_;
    DevBuf<uint2> erased_;
    // native transport (comm.hip): the world owns — and grows — the exchange buffers
    Comm* comm_ = nullptr;
    DevBuf<unsigned> xch_send_, xch_recv_;
    size_t xch_capacity_ = 0;
    unsigned sharded_steps_ = 0;
    size_t agreed_seg_ = 0;                  // segment bytes of the last host-read agreement (0: none): step_sharded
    int ensure_exchange_capacity(size_t bytes);
    // edits between steps: the bracket they are refused in, and their staging
    bool mid_step_ = false;                  // set by pre_solve, cleared by finish_step / step_end (and by the calls that wrap them)
    int check_batch(const char* what, const int* bodies, const void* values, int count, bool edit);
    std::vector<unsigned> edit_seen_; unsigned edit_epoch_ = 0;      // duplicate check: edit_seen_[i] == edit_epoch_ <=> body i is in this batch
    BatchStage stage_;                       // the batches' pinned staging and their place on the device (released by ~World)
    DevBuf<phx_rigid_body> gathered_;
    DevBuf<float4> poses_;
    std::vector<float> spawn_rows_;          // add_bodies: the 10-float rows of a batch (spawn_row), staged from here
    // removal: keep flags and the exclusive scans that place the kept bodies / manifolds / joints, the counts ([0] bodies, [1] manifolds,
    // [2] joints kept, [3] kept records with an acceleration), the remap, the kept pairs; the compaction writes into the spare buffers,
    // which then change places with the world's own (the old ones are the spares of the next removal)
    DevBuf<unsigned> rm_keep_, rm_bnew_, rm_mnew_, rm_jnew_, rm_counts_;
    DevBuf<int> rm_remap_;
    DevBuf<uint2> rm_pairs_;
    int compaction_scratch();
    template <class Keep> int scan_compaction(const Keep& kept);
    template <class Keep> int queue_compaction(const Keep& kept);
    int adopt_compaction(const unsigned got[5]);      // the compacted contact cache becomes the world's
    template <class Keep> int drop_manifolds(const Keep& kept, int* dropped);      // the manifolds `kept` rejects go, with their slots and joints
    struct Spare {
        BodyStore bodies;
        DevBuf<float4> accel;
        DevBuf<phx_manifold> manifolds;
        DevBuf<phx_contact_point> cps;
        DevBuf<phx_contact_joint> joints;
    } spare_;
    // queries: the geometry epoch is bumped by every path that writes the AABBs (or the frames behind it) or changes the body count; the
    // query index is current while it was built for this epoch
    unsigned long long geom_epoch_ = 0;
    DeviceQuery query_;
    DevBuf<int> q_body_;
    DevBuf<phx_ray_hit> q_hits_;
    DevBuf<phx_shape_hit> q_shape_hits_;
    DevBuf<phx_near_hit> q_near_hits_;
    int query_prepare(bool host_wait);
    // the three skeletons of the query calls (world_query.hip): one result per query through `buf` to the host (`miss`: what an empty
    // world answers) / the same on caller-owned device memory / the overlap lists.  `run`: the DeviceQuery call; `kind`: what a row
    // holds, and with it its width and the rules its values are checked by.
    enum QueryRows { ROWS_POINTS, ROWS_BOXES, ROWS_RAYS, ROWS_SHAPES, ROWS_CASTS, ROWS_CIRCLES, ROWS_CIRCLE_CASTS, ROWS_NEAR };
    template <class Hit> using QueryRun = int (DeviceQuery::*)(const WorldBodies&, int, unsigned long long, const float*, int, int, Hit*, hipStream_t);
    using OverlapRun = int (DeviceQuery::*)(const WorldBodies&, int, unsigned long long, const float*, int, int, int32_t*, int32_t*, int, int64_t*, Readback&, hipStream_t);
    template <class Hit> int query_rows(const char* what, const float* rows, int count, QueryRows kind, int flags, Hit* out, const Hit& miss, DevBuf<Hit>& buf, QueryRun<Hit> run);
    template <class Hit> int query_rows_device(const char* what, const void* d_rows, int count, QueryRows kind, int flags, void* d_out, QueryRun<Hit> run);
    int query_overlaps(const char* what, const float* boxes, int count, QueryRows kind, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total, OverlapRun run);
    // contact reports: the contact epoch is bumped by every path that can change the manifolds (every step, a removal, set_state and so
    // a re-slab) or the body count; the contact index is current while it was built for this epoch
    unsigned long long contact_epoch_ = 0;
    DeviceContacts contacts_;
    ContactCache contact_cache() const { return ContactCache{d_manifolds_.p, nm, d_cps_.p, d_joints_.p, nj, bodies_.mpos.p, nb(), sleep_col_.ptr()}; }
    int contact_prepare(const char* what, bool host_wait);
    // the optional columns (BodyTable): collision filters — an active table picks the filtered sweep — and materials — an active table
    // picks the solver's material kernels (DeviceSolver::set_materials) — and body flags — an active table picks the sensor variants of
    // the joint match and takes the schedule rebuild's components from the joints (refresh_contact_joints, pre_solve)
    BodyTable<FilterColumn> filters_;
    // the collision exclusions (exclusions.h): a set that is not empty picks the excluded sweep
    ExclusionSet exclusions_;
    int check_exclusion_pairs(const char* what, const int32_t* pairs, int count, std::vector<unsigned long long>* keys);
    BodyTable<MaterialColumn> materials_;
    BodyTable<FlagsColumn> flags_col_;
    // ... and the sleep states (sleep.h): active exactly while sleeping is enabled
    BodyTable<SleepColumn> sleep_col_;
    // ... and the shapes' kinds (include/phyx_amd.h SHAPES): active once some set_shapes call named a circle; an active table picks
    // UpdateManifolds' BodyShapes instantiation and hands the kinds to the queries.  capsules_: some call named a capsule since the last
    // set_state / load (a load takes the saved world's bit); with the table active it picks the BodyCapsules instantiation and the
    // queries' capsule instantiations, so a world of boxes and circles launches the kernels it always did
    BodyTable<ShapeColumn> shapes_;
    bool capsules_ = false;
    bool capsules() const { return capsules_ && shapes_.active; }
    // ... and the polygon records (include/phyx_amd.h POLYGONS): active once some set_polygons call named a polygon.  polygons_: the bit
    // that call sets and set_state clears (a load takes the saved world's); with both tables active it picks the BodyPolygons
    // instantiation and the queries' polygon instantiations
    BodyTable<PolygonColumn> polys_;
    bool polygons_ = false;
    bool polygons() const { return polygons_ && shapes_.active && polys_.active; }
    // ... and the continuous bodies' {rc, start} (include/phyx_amd.h CONTINUOUS BODIES): active once some set_continuous call named one
    BodyTable<SweepColumn> sweep_col_;
    DeviceSweep sweep_;
    int sweep_begin();                   // queued in front of the integrator: start := pos of the continuous bodies; a world without queues nothing
    int sweep_pass();                    // queued behind IntegratePosition, in front of the sleep pass
    // set_shapes / set_polygons: no listed continuous body's core radius is left at or above its new inradius (`polygons`: null unless polygons are set)
    int check_core_radii(const char* what, const int32_t* bodies, const phx_shape* shapes, const phx_polygon* polygons, int count);
    DeviceSleep sleep_;
    bool sleep_count_pending_ = false;   // the pass or a wake may have changed the static set: the device's count has not been looked at yet
    DevBuf<phx_sleep_state> sleep_out_;
    SleepGraph sleep_graph();            // the edges as the device holds them now (the unit lists uploaded)
    int sleep_pass(float dt);            // queued behind IntegratePosition
    // the sleeping components of the named bodies wake (queued; nothing happens in a world without the column): `bodies`, or the bodies
    // whose `d_keep` word is 0, or (`all`) every sleeper.  At the top of every call between steps that names a body or a unit.
    int wake_named(const int* bodies, int count, const unsigned* d_keep = nullptr, bool all = false);
    template <class P> int wake_units(const int32_t* which, int count);      // both bodies of the listed units
    void take_sleep_count(unsigned changed);      // what set_inverse_masses does when the static set changed
    int settle_sleep_count();            // ... by a readback of its own, where no step's count readback has brought it yet
    template <class F> int each_table(F f) { PHX_TRY(f(filters_)); PHX_TRY(f(materials_)); PHX_TRY(f(flags_col_)); PHX_TRY(f(sleep_col_)); PHX_TRY(f(shapes_)); PHX_TRY(f(polys_)); return f(sweep_col_); }
    // the three setters' skeleton: `rule(k)` is the call's own check of entry k
    template <class Column, class Rule>
    int set_column(const char* what, BodyTable<Column>& table, const int32_t* bodies, const typename Column::api* values, int count, Rule rule, bool host_path_ok);
    PinSet pins_;
    DeviceFields fields_;
    FieldBodies field_bodies() const { return FieldBodies{bodies_.mpos.p, bodies_.vel.p, filters_.ptr(), nb()}; }
    int field_pass(float dt);            // queued in front of IntegrateVelocity; a world without fields queues nothing
    bool accel_from_fields_ = false;     // accel_ holds this step's field sums alone: the records' accelerations are zero already
    int break_step_ = 0;                 // the steps taken since the break events were last taken: the next step's ordinal in them
    int settle_breaks();                 // between steps: what the last step's break test found is applied (PinSet::settle); at the top of every call that reads or changes units
    template <class P> int check_unit_indices(const char* what, const int32_t* which, const void* values, int count);
    int check_unit_bodies(const char* what, const char* noun, int k, int body1, int body2);
    // an edit of Fields::width floats per listed unit (already checked): staged for the scatter kernel when the list is on the device
    template <class P, class Fields> int set_unit_fields(const int32_t* which, const float* values, int count);
    BodyColumns columns() const { return BodyColumns{accel_pending_ ? accel_.p : nullptr, filters_.ptr(), materials_.ptr(), flags_col_.ptr(), sleep_col_.ptr(), shapes_.ptr(), polys_.ptr(), sweep_col_.ptr()}; }
    BodyColumns spare_columns() const { return BodyColumns{accel_pending_ ? spare_.accel.p : nullptr, filters_.spare_ptr(), materials_.spare_ptr(), flags_col_.spare_ptr(), sleep_col_.spare_ptr(), shapes_.spare_ptr(), polys_.spare_ptr(), sweep_col_.spare_ptr()}; }
};

} // namespace phx

struct phx_world {
    phx::World impl;
    explicit phx_world(int d) : impl(d) {}
};
