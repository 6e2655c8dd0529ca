// world.hip — World: the whole step of ref: src/World.cpp:19-37 on HBM-resident arrays.
//
// Bodies live on the device as the RESIDENT structure of arrays (body_view.h: velocities, displacing velocities,
// {invMass, invInertia, pos}, frame, AABB, size — every kernel of the step reads the 16-byte granules it needs, coalesced);
// the reference's 128-byte records exist at the C-ABI edge only (construction, phx_world_get_bodies).  Manifolds / contact
// points / joints live on the device in the reference's POD layouts; the host keeps only their counts.  Per step: IntegrateVelocity (kernel) -> UpdateBroadphase + UpdatePairs (DeviceBroadphase) ->
// manifold creation + UpdateManifolds (narrowphase kernel) -> PackManifolds -> RefreshContactJoints (scan-based,
// order-preserving, world_kernels.h) -> SolveJoints (DeviceSolver) -> IntegratePosition (kernel).  What crosses
// PCIe per step is a handful of counters (new pairs, dead manifolds, new / dead joints) and, only when the joint
// topology changed, the body-pair list the host schedule builder needs.
#include "reslab.h"
#include "handles.h"
#include "device_scan.h"
#include "world_kernels.h"
#include "query.h"
#include "contact.h"
#include "snapshot.h"
#include "pins.h"
#include "fields.h"
#include "exclusions.h"

#include <algorithm>
#include <chrono>
#include <cmath>

namespace phx {

static inline int wgrid(int n) { return std::max(1, std::min(div_up(n, 256), 4096)); }
static inline int rgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }      // the removal's streaming passes (grid-stride beyond 2048 workgroups)
constexpr int PRELABEL_EARLY_MANIFOLDS = 400000;      // worlds from this size on queue the side stream's share of the schedule rebuild before the joint match (refresh_contact_joints)

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
    int query_index_build();             // the query index alone, built unless current (tools/query_cost.py)
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
    int refuse_exclusions(const char* what) const;      // PHX_ERR_STATE while the set is not empty (the sharded modes carry none)
    // materials (phx_world_set_materials / get_materials): between steps; they change no topology
    int set_materials(const int32_t* bodies, const phx_material* materials, int count);
    int get_materials(phx_material* out, int cap);
    // body flags (phx_world_set_body_flags / get_body_flags): between steps; the joints of a sensor go or come at the next step's refresh
    int set_body_flags(const int32_t* bodies, const uint32_t* flags, int count);
    int get_body_flags(uint32_t* out, int cap);
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
    int refuse_fields(const char* what) const;      // PHX_ERR_STATE while the field list is not empty (the sharded modes carry none)
    int refuse_pins(const char* what);         // PHX_ERR_STATE while a pin or a link exists (the sharded modes carry none)
    PinSet& pins() { return pins_; }
    int refuse_tables(const char* what);       // PHX_ERR_STATE if some body's value in an optional column is not the default (the sharded modes carry none)

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
    WorldBodies query_view() const { WorldBodies w = bodies_.view(); w.sleep = sleep_col_.ptr(); return w; }      // (to a query a sleeper is not static)
    bool host_staged() const { return bodies_dirty_ || !bodies_.records.p; }      // the host-staged records are the world
    int restage_on_host();               // ... again, after the device copy was: records and tables come down
    int refuse_mid_step(const char* what) const;      // PHX_ERR_STATE between pre_solve / step_begin and finish_step / step_end
    int refuse_sharded(const char* what, const char* plural) const;      // PHX_ERR_STATE: a sharded world carries no columns and no units
    int settle_on_device();              // this world's device is current and a pending solve settled: what a call queues goes behind it, never under a replay
    int update_pairs();
    bool fuse_velocity_ = false; float step_dt_ = 0.f;      // IntegrateVelocity rides on the broadphase's key build (update_pairs)
    int fresh_manifolds_ = 0;           // pairs UpdatePairs found this step: their manifolds are created by UpdateManifolds' kernel
    int manifolds_updated_ = 0;         // manifolds [0, this) were updated during update_pairs' round trip (update_manifolds() does the rest)
    int update_manifolds();
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
    int stage_batch(const int* bodies, const float* values, int count, int width, const int** d_bodies, const float** d_values);
    std::vector<unsigned> edit_seen_; unsigned edit_epoch_ = 0;      // duplicate check: edit_seen_[i] == edit_epoch_ <=> body i is in this batch
    char* stage_pin_ = nullptr; size_t stage_cap_ = 0, stage_used_ = 0;      // pinned staging of the batches: bump-allocated while copies are pending
    hipEvent_t stage_done_ = nullptr;        // recorded behind the last batch's copy: once it has passed, the staging buffer is free again
    std::vector<char*> stage_retired_;       // outgrown staging buffers a pending copy may still read: freed with the world
    DevBuf<char> edit_dev_;                  // the batch on the device (stream order protects it from the next batch's copy)
    std::vector<DevBuf<char>> edit_dev_retired_;      // outgrown device batches a pending scatter may still read: freed with the world
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
    int query_prepare(bool host_wait);
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
    template <class F> int each_table(F f) { PHX_TRY(f(filters_)); PHX_TRY(f(materials_)); PHX_TRY(f(flags_col_)); return f(sleep_col_); }
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
    BodyColumns columns() const { return BodyColumns{accel_pending_ ? accel_.p : nullptr, filters_.ptr(), materials_.ptr(), flags_col_.ptr(), sleep_col_.ptr()}; }
    BodyColumns spare_columns() const { return BodyColumns{accel_pending_ ? spare_.accel.p : nullptr, filters_.spare_ptr(), materials_.spare_ptr(), flags_col_.spare_ptr(), sleep_col_.spare_ptr()}; }
};

World::~World()
{
    if (hipSetDevice(device_) != hipSuccess) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    for (char* p : stage_retired_) (void)hipHostFree(p);
    if (stage_pin_) (void)hipHostFree(stage_pin_);
    if (stage_done_) (void)hipEventDestroy(stage_done_);
    // (device buffers are DevBuf members: freed with the object)
    // (stream_ belongs to the broadphase handle, which is destroyed after this body and after the solver handle)
}

int World::init()
{
    PHX_TRY(broadphase_.init());
    PHX_TRY(solver_.init());
    // one stream for the whole step: broadphase, narrowphase, contact cache, solver and integrators are ordered by it, the
    // host waits only where it needs a count to size the next launch
    stream_ = broadphase_.stream();
    PHX_TRY(solver_.adopt_stream(stream_));
    PHX_TRY(counters_.reserve(8));
    PHX_TRY(query_.configure_from_env());
    PHX_TRY(pins_.configure_from_env());
    return contacts_.configure_from_env();
}

// ref: World.cpp:11-17, RigidBody.h:15-36, Coords2.h:10-17 (cos/sin resolve to the double overloads): the record AddBody makes (index
// aside).  add_body and add_bodies both build from it; the frame stays on the host because the device's cos / sin are not promised to
// round as the host's do.
static phx_rigid_body body_record(float px, float py, float angle, float sx, float sy)
{
    phx_rigid_body b;
    std::memset(&b, 0, sizeof b);
    const float pi = 3.141592f;
    const float quarter = angle + pi / 2.0f;
    b.xvector.x = (float)std::cos((double)angle);   b.xvector.y = (float)std::sin((double)angle);
    b.yvector.x = (float)std::cos((double)quarter); b.yvector.y = (float)std::sin((double)quarter);
    b.pos.x = px; b.pos.y = py;
    b.geom_size.x = sx; b.geom_size.y = sy;
    const float density = 1e-5f;
    const float mass = density * (sx * sy);
    const float inertia = mass * (sx * sx + sy * sy);
    b.inv_mass = 1.0f / mass;
    b.inv_inertia = 1.0f / inertia;
    update_geom(b);
    return b;
}

int World::add_body(float px, float py, float angle, float sx, float sy)
{
    PHX_TRY(restage_on_host());
    phx_rigid_body b = body_record(px, py, angle, sx, sy);
    b.index = (uint32_t)host_bodies_.size();
    host_bodies_.push_back(b);
    each_table([](auto& t) { t.push_default(); return PHX_OK; });
    bodies_dirty_ = true;
    return (int)host_bodies_.size() - 1;
}

int World::restage_on_host()
{
    if (host_staged()) return PHX_OK;
    if (!host_bodies_.empty()) PHX_TRY(download_bodies(host_bodies_.data(), (int)host_bodies_.size()));
    return each_table([this](auto& t) { return t.to_host(nb(), device_, stream_); });
}

int World::refuse_mid_step(const char* what) const
{
    if (!mid_step_) return PHX_OK;
    set_error("%s: the world is between pre_solve / step_begin and finish_step / step_end", what);
    return PHX_ERR_STATE;
}

int World::refuse_sharded(const char* what, const char* plural) const
{
    if (shard_count <= 1 && !comm_) return PHX_OK;
    set_error("%s: a sharded world carries no %s", what, plural);
    return PHX_ERR_STATE;
}

int World::settle_on_device()
{
    PHX_TRY(use_device(device_));
    return solver_.has_pending() ? solver_.synchronize() : PHX_OK;
}

int World::set_static(int body)
{
    PHX_TRY(wake_named(&body, 1));
    PHX_TRY(restage_on_host());
    host_bodies_[body].inv_mass = 0.f;
    host_bodies_[body].inv_inertia = 0.f;
    bodies_dirty_ = true;
    pins_.statics_changed();
    return PHX_OK;
}

int World::set_inverse_mass(int body, float inv_mass, float inv_inertia)
{
    PHX_TRY(wake_named(&body, 1));
    PHX_TRY(restage_on_host());
    host_bodies_[body].inv_mass = inv_mass;
    host_bodies_[body].inv_inertia = inv_inertia;
    bodies_dirty_ = true;
    joints_changed_ = true;              // which bodies are static is part of the schedule's topology
    pins_.statics_changed();
    return PHX_OK;
}

int World::sync_bodies_to_device()
{
    if (!bodies_dirty_) return PHX_OK;
    PHX_TRY(use_device(device_));
    const size_t n = std::max<size_t>(host_bodies_.size(), 1);
    PHX_TRY(bodies_.reserve(n));
    if (!host_bodies_.empty()) {
        PHX_HIP(hipMemcpyAsync(bodies_.records.p, host_bodies_.data(), host_bodies_.size() * sizeof(phx_rigid_body), hipMemcpyHostToDevice, stream_));
        hipLaunchKernelGGL(k_bodies_to_world, dim3(wgrid(nb())), dim3(256), 0, stream_, (const phx_rigid_body*)bodies_.records.p, nb(), resident());
        PHX_HIP(hipGetLastError());
        // records that come with accelerations (a handed-over state; AddBody leaves none): the next IntegrateVelocity applies them,
        // once, like the reference (ref: World.cpp:44-53)
        accel_pending_ = false;
        for (const phx_rigid_body& b : host_bodies_) if (b.acceleration.x != 0.f || b.acceleration.y != 0.f || b.angular_acceleration != 0.f) { accel_pending_ = true; break; }
        if (accel_pending_) {
            std::vector<float4> acc(host_bodies_.size());
            for (size_t i = 0; i < acc.size(); ++i) acc[i] = make_float4(host_bodies_[i].acceleration.x, host_bodies_[i].acceleration.y, host_bodies_[i].angular_acceleration, 0.f);
            PHX_TRY(accel_.reserve(acc.size()));
            PHX_HIP(hipMemcpyAsync(accel_.p, acc.data(), acc.size() * sizeof(float4), hipMemcpyHostToDevice, stream_));
            PHX_HIP(hipStreamSynchronize(stream_));      // (`acc` is a local)
        }
    }
    PHX_TRY(each_table([&](auto& t) { return t.upload(n, stream_); }));
    PHX_HIP(hipStreamSynchronize(stream_));
    each_table([](auto& t) { t.host.clear(); return PHX_OK; });
    bodies_dirty_ = false;
    records_stale_ = false;
    ++geom_epoch_;
    ++contact_epoch_;
    return PHX_OK;
}

int World::refresh_records()
{
    if (!records_stale_ || !nb()) return PHX_OK;
    hipLaunchKernelGGL(k_world_to_bodies, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), bodies_.records.p);
    PHX_HIP(hipGetLastError());
    records_stale_ = false;
    return PHX_OK;
}

int World::scratch_for(int n)
{
    PHX_TRY(flags_.reserve((size_t)n + 2));
    PHX_TRY(mover_pos_.reserve((size_t)n + 2));
    return PHX_OK;
}

int World::update_pairs()                                                   // ref: Collider.cpp:251-345
{
    const DeviceBroadphase::StepPrologue prologue{gravity, step_dt_, counters_.p, bodies_.vel.p, bodies_.mpos.p, accel_pending_ ? (const float4*)accel_.p : nullptr};
    // UpdateManifolds of the manifolds that exist already needs nothing from this update (positions, rotations and AABBs do not
    // change in it): it is queued behind the mailbox post of the new-pair count and runs while that round trip is under way — the
    // GPU used to idle through it.  The new pairs' manifolds follow in update_manifolds().  (Not with per-phase timing: the phases
    // would overlap.)
    manifolds_updated_ = 0;
    packed_this_step_ = false;
    const std::function<int()> old_manifolds = [this]() -> int {
        if (!nm) return PHX_OK;
        PHX_TRY(scratch_for(nm));
        PHX_TRY(pack_flags_.reserve((size_t)nm + 2));
        hipLaunchKernelGGL(k_update_manifolds, dim3(wgrid(nm)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p,
                           pack_flags_.p, reinterpret_cast<int*>(counters_.p + 3), nm, (const uint2*)nullptr, 0, counters_.p + 2, old_ride_ ? *old_ride_ : MailRide{});
        PHX_HIP(hipGetLastError());
        manifolds_updated_ = nm;
        return PHX_OK;
    };
    // (that launch also CARRIES the post of the new-pair count: its first workgroup posts before it updates — a dispatch fewer per step)
    const MailCarrier old_manifolds_with = [&](const MailRide* ride) -> int { old_ride_ = ride; const int st = old_manifolds(); old_ride_ = nullptr; return st; };
    PHX_TRY(exclusions_.sync(nb(), stream_));                               // (nothing unless the set or the body count changed since the last step)
    PHX_TRY(broadphase_.update_resident(bodies_.aabb.p, nb(), fuse_velocity_ ? &prologue : nullptr, phase_timing ? nullptr : &old_manifolds,
                                        phase_timing || !nm ? nullptr : &old_manifolds_with,      // same stream; returns once the new-pair count is known
                                        filters_.ptr(), exclusions_.view()));
    fuse_velocity_ = false;
    if (accel_pending_) {                  // IntegrateVelocity of this step has consumed the uploaded accelerations (ref: World.cpp:50, 53)
        accel_pending_ = false;
        if (nb() && !accel_from_fields_) hipLaunchKernelGGL(k_clear_accelerations, dim3(wgrid(nb())), dim3(256), 0, stream_, bodies_.records.p, nb());
        PHX_HIP(hipGetLastError());
    }
    const int fresh = broadphase_.new_pair_count();
    if (!fresh) return PHX_OK;
    PHX_TRY(d_manifolds_.reserve_keep((size_t)nm + fresh, nm, stream_));
    PHX_TRY(d_cps_.reserve_keep(2 * ((size_t)nm + fresh), 2 * (size_t)nm, stream_));
    nm += fresh;                                                            // (created by UpdateManifolds' kernel, in the lane that updates them)
    fresh_manifolds_ = fresh;
    return PHX_OK;
}

int World::update_manifolds()                                               // ref: Collider.cpp:368-377
{
    const int first = manifolds_updated_;                                   // (the old manifolds may have been updated during update_pairs' round trip)
    manifolds_updated_ = 0;
    if (nm <= first) { fresh_manifolds_ = 0; return PHX_OK; }
    PHX_TRY(scratch_for(nm));
    PHX_TRY(pack_flags_.reserve_keep((size_t)nm + 2, (size_t)first, stream_));      // (a pending pack keeps its scan in it until refresh_contact_joints settles it)
    hipLaunchKernelGGL(k_update_manifolds, dim3(wgrid(nm - first)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p,
                       pack_flags_.p, reinterpret_cast<int*>(counters_.p + 3), nm - fresh_manifolds_, broadphase_.new_pairs_device(), first, counters_.p + 2, MailRide{});
    fresh_manifolds_ = 0;
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int World::pack_manifolds()                                                 // ref: Collider.cpp:379-416
{
    pack_pending_ = false;
    if (!nm) return PHX_OK;
    // counters_[2] holds the number of dead manifolds already (k_update_manifolds counts them); the scan of their flags — what the
    // clean-up places its movers by — runs only when there are any: at once if the last step had some, else (the bet) after
    // refresh_contact_joints' round trip has shown the count
    if (expect_no_dead_manifolds_ && !phase_timing) { pack_pending_ = true; return PHX_OK; }
    PHX_TRY(device_exclusive_scan(pack_flags_.p, nm, counters_.p + 2, scan_tiles_, stream_));
    unsigned host[2] = {0, 0};                                              // [0] dead manifolds, [1] dropped points
    PHX_TRY(rb_.add(host, counters_.p + 2, sizeof host, stream_));
    PHX_TRY(rb_.wait(stream_));
    return finish_pack((int)host[0], (int)host[1]);
}

int World::finish_pack(int dead, int dropped)
{
    dropped_points += dropped;
    expect_no_dead_manifolds_ = dead == 0;
    if (!dead) return PHX_OK;
    packed_this_step_ = true;
    PHX_TRY(erased_.reserve(dead));
    hipLaunchKernelGGL(k_compact_movers, dim3(wgrid(dead)), dim3(256), 0, stream_, (const unsigned*)pack_flags_.p, (const unsigned*)(counters_.p + 2), nm, nm, mover_pos_.p);
    hipLaunchKernelGGL(k_pack_manifolds, dim3(wgrid(nm)), dim3(256), 0, stream_, d_manifolds_.p, d_cps_.p, nm, (const unsigned*)pack_flags_.p,
                       (const unsigned*)(counters_.p + 2), (const int*)mover_pos_.p, erased_.p);
    PHX_HIP(hipGetLastError());
    nm -= dead;
    return broadphase_.erase_pairs_device(erased_.p, dead);                 // ref: Collider.cpp:391 manifoldMap.erase
}

int World::refresh_contact_joints()                                         // ref: World.cpp:72-149
{
    PHX_TRY(scratch_for(std::max(nm, nj + 2 * nm)));
    PHX_TRY(dead_flags_.reserve((size_t)nj + 2));
    const size_t seen_cap = joint_seen_.cap;
    PHX_TRY(joint_seen_.reserve((size_t)nj + 2));
    if (joint_seen_.cap != seen_cap) {                                      // new (uninitialised) table: stale stamps could alias
        PHX_HIP(hipMemsetAsync(joint_seen_.p, 0, joint_seen_.cap * sizeof(unsigned), stream_));
        joint_epoch_ = 0;
    }
    // One host round trip for the counts.  A joint is dead iff no contact point re-attached it (the match), which is
    // known before the new joints exist; the new joints are appended behind the old ones and are alive by construction.
    unsigned host[4] = {0, 0, 0, 0};                                        // [0] new joints, [1] dead joints, [2] dead manifolds, [3] dropped points
    const uint32_t* const sensor_flags = flags_col_.ptr();                  // the sensor rule (world_kernels.h BodySensors); null: no body ever got a flag
    for (;;) {
        if (++joint_epoch_ == 0) {                                          // the epoch wrapped: stale stamps could alias
            PHX_HIP(hipMemsetAsync(joint_seen_.p, 0, joint_seen_.cap * sizeof(unsigned), stream_));
            joint_epoch_ = 1;
        }
        // (the side stream's share of the rebuild is queued BEHIND the match and its scans in a small world — the host needs ~30 us for its
        //  eight launches, more than those kernels run, and the GPU would idle — but IN FRONT of them in a large one, whose match alone runs
        //  longer than that: at 1M boxes the side stream's 140 us were the critical path of the step, started 100 us after they could have)
        if (nm >= PRELABEL_EARLY_MANIFOLDS) PHX_TRY(solver_.prelabel_components((const float4*)bodies_.mpos.p, nb(), (const phx_manifold*)d_manifolds_.p, nm));
        if (nm) {
            // (a null column pointer picks the plain instantiation: the kernels of a world that never set a flag)
            if (sensor_flags) hipLaunchKernelGGL(k_joints_match<BodySensors>, dim3(wgrid(nm)), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, nm, d_cps_.p,
                                                 d_joints_.p, joint_seen_.p, joint_epoch_, flags_.p, BodySensors{sensor_flags});
            else hipLaunchKernelGGL(k_joints_match<NoSensors>, dim3(wgrid(nm)), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, nm, (const phx_contact_point*)d_cps_.p,
                                    d_joints_.p, joint_seen_.p, joint_epoch_, flags_.p, NoSensors{});
            PHX_TRY(device_exclusive_scan(flags_.p, nm, counters_.p, scan_tiles_, stream_));
        }
        if (nj) PHX_TRY(device_exclusive_scan_of(JointDeadLoad{(const unsigned*)joint_seen_.p, joint_epoch_}, dead_flags_.p, nj, counters_.p + 1, scan_tiles_, stream_));
        if (nm || nj || pack_pending_) {                                    // counters_[0 .. 3]: adjacent words, one copy
            unsigned got[4] = {0, 0, 0, 0}, sleep_changed = 0;
            PHX_TRY(rb_.add(got, counters_.p, sizeof got, stream_));
            const bool with_sleep = sleep_count_pending_;                  // (the last pass's count rides along: no wait of its own)
            if (with_sleep) PHX_TRY(rb_.add(&sleep_changed, sleep_.words() + SLEEP_CHANGED, sizeof sleep_changed, stream_));
            PHX_TRY(solver_.prelabel_components((const float4*)bodies_.mpos.p, nb(), (const phx_manifold*)d_manifolds_.p, nm));      // (once: the mark is consumed)
            PHX_TRY(rb_.wait(stream_));
            if (with_sleep) take_sleep_count(sleep_changed);
            host[0] = got[0]; host[1] = got[1];
            if (pack_pending_) { host[2] = got[2]; host[3] = got[3]; }      // (else PackManifolds has settled them already)
            if (!nm) host[0] = 0;                                           // (not written this step)
            if (!nj) host[1] = 0;
        }
        if (!pack_pending_) break;
        // PackManifolds' count came back with the joints': normally 0 (that was the bet) — if not, pack now and match again
        pack_pending_ = false;
        const int nm_before = nm;
        ++deferred_packs;
        if (host[2]) {
            // the bet was lost: now the flags are scanned, and the manifolds MOVE — under the side stream, which is reading them to count
            // and bin the components: what it makes of them is void, and this step's rebuild takes its components from the joints
            PHX_TRY(solver_.cancel_prelabel());
            PHX_TRY(device_exclusive_scan(pack_flags_.p, nm, counters_.p + 2, scan_tiles_, stream_));
        }
        PHX_TRY(finish_pack((int)host[2], (int)host[3]));
        if (nm == nm_before) break;
        ++deferred_pack_retries;                                            // the bet was lost: match again under a new epoch (one more pass: nothing is pending now)
    }
    PHX_TRY(settle_sleep_count());                                          // (a world without manifolds and joints: nothing brought it)
    const int fresh = (int)host[0], dead = (int)host[1], old = nj;
    const int total = nj + fresh;
    if (dead) PHX_TRY(mover_pos_.reserve((size_t)total + 2));
    if (fresh) {
        joints_changed_ = true;
        PHX_TRY(d_joints_.reserve_keep((size_t)nj + fresh, nj, stream_));
        const int mover_blocks = dead ? wgrid(dead) : 0;                    // the clean-up's movers ride along (independent of the new joints)
        if (sensor_flags) hipLaunchKernelGGL(k_joints_create<BodySensors>, dim3(wgrid(nm) + mover_blocks), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, nm, d_cps_.p,
                                             d_joints_.p, nj, (const unsigned*)flags_.p, mover_blocks, (const unsigned*)dead_flags_.p, (const unsigned*)(counters_.p + 1), total,
                                             mover_pos_.p, BodySensors{sensor_flags});
        else hipLaunchKernelGGL(k_joints_create<NoSensors>, dim3(wgrid(nm) + mover_blocks), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, nm, d_cps_.p, d_joints_.p, nj,
                                (const unsigned*)flags_.p, mover_blocks, (const unsigned*)dead_flags_.p, (const unsigned*)(counters_.p + 1), total, mover_pos_.p, NoSensors{});
    }
    if (dead) {                                                             // cleanup (ref: World.cpp:125-143): holes take movers from the tail
        joints_changed_ = true;
        if (!fresh) hipLaunchKernelGGL(k_compact_movers, dim3(wgrid(dead)), dim3(256), 0, stream_, (const unsigned*)dead_flags_.p, (const unsigned*)(counters_.p + 1), total, old,
                                       mover_pos_.p);
        hipLaunchKernelGGL(k_joints_fill, dim3(wgrid(total)), dim3(256), 0, stream_, d_joints_.p, total, old, (const unsigned*)dead_flags_.p,
                           (const unsigned*)(counters_.p + 1), (const int*)mover_pos_.p, d_cps_.p);
    }
    nj = total - dead;
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int World::solve(const phx_config& cfg, bool settle)                        // ref: World.cpp:34
{
    // island sharding: the solver sweeps only this rank's groups (DeviceSolver::set_shard); the other groups' bodies
    // keep their velocities here
    if (!joints_changed_) PHX_TRY(solver_.cancel_prelabel());              // (no rebuild will pick the side stream's bins up)
    solver_.set_materials(materials_.ptr());      // (the table moves with spawns and removals: handed over every solve)
    PHX_TRY(solver_.solve_resident(resident().s, nb(), d_cps_.p, 2 * nm, d_joints_.p, nj, cfg, joints_changed_));
    joints_changed_ = false;
    // a solve that is still unverified (it ran speculatively on the cached schedule, or on a device-built schedule whose 'every
    // bin fits' flag has not been read) must be settled before anything consumes its result unconditionally
    return settle && solver_.has_pending() ? solver_.synchronize() : PHX_OK;
}

// IntegratePosition behind the solve.  An unverified solve is NOT waited for first: the integrator is queued behind it gated by
// the same fingerprint word (it integrates nothing if the solve committed nothing), THEN the host settles the solve — its
// round trip overlaps the island kernel and the integrator instead of idling the GPU — and repeats the integrator only if the
// solve had to be repeated.
int World::solve_and_integrate(float dt, const phx_config& cfg)
{
    { RoctxRange r("SolveJoints"); PHX_TRY(solve(cfg, false)); }
    RoctxRange r("IntegratePosition");                                      // ref: World.cpp:57-70
    ++geom_epoch_;
    const bool pending = solver_.has_pending();
    const unsigned replays = solver_.replays();
    // (what the settle reads is final when the solve's last kernel ends, so its mailbox post goes in FRONT of the integrator and the
    //  integrator is queued while the post crosses the link: the host wakes up a kernel earlier)
    bool integrated = false;
    // (the integrator also CARRIES the settle's post: its first workgroup posts before it integrates — a dispatch fewer per step)
    const MailCarrier integrate_with = [&](const MailRide* ride) -> int {
        integrated = true;
        if (nb()) hipLaunchKernelGGL(k_integrate_position, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), dt,
                                     pending ? solver_.fingerprint_word() : (const unsigned long long*)nullptr, solver_.expected_fingerprint(), ride ? *ride : MailRide{});
        PHX_HIP(hipGetLastError());
        return PHX_OK;
    };
    const std::function<int()> integrate = [&]() -> int { return integrate_with(nullptr); };
    if (!pending) PHX_TRY(integrate());
    if (pending) {
        PHX_TRY(solver_.synchronize(&integrate, nb() ? &integrate_with : nullptr));
        if (!integrated) { set_error("the settle did not queue the integrator"); return PHX_ERR_STATE; }
        if (solver_.replays() != replays && nb())
            hipLaunchKernelGGL(k_integrate_position, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), dt, (const unsigned long long*)nullptr, 0ull, MailRide{});
        PHX_HIP(hipGetLastError());
    }
    return PHX_OK;
}

int World::pre_solve(float dt)
{
    using clk = std::chrono::steady_clock;
    PHX_TRY(use_device(device_));
    mid_step_ = true;
    ++contact_epoch_;
    PHX_TRY(sync_bodies_to_device());
    auto t = clk::now();
    auto lap = [&](int phase) { if (!phase_timing) return; (void)hipStreamSynchronize(stream_); auto n = clk::now(); phase_ms[phase] = std::chrono::duration<double, std::milli>(n - t).count(); t = n; };
    RoctxRange update_range("Update (before SolveJoints)");                 // ref: World.cpp:21
    {
        RoctxRange r("IntegrateVelocity");                                  // ref: World.cpp:39-55
        // (normally fused into the broadphase's first kernel, update_pairs(); a kernel of its own only when the phases are timed one by one)
        fuse_velocity_ = !phase_timing;
        step_dt_ = dt;
        records_stale_ = true;
        PHX_TRY(field_pass(dt));
        if (nb() && !fuse_velocity_) hipLaunchKernelGGL(k_integrate_velocity, dim3(wgrid(nb())), dim3(256), 0, stream_, bodies_.vel.p, (const float4*)bodies_.mpos.p, nb(), gravity, dt, counters_.p, accel_pending_ ? (const float4*)accel_.p : nullptr);
        PHX_HIP(hipGetLastError());
        lap(0);
    }
    // the device runs sort and sweep back to back; the host clock cannot split them, so the whole device broadphase
    // is booked under UpdatePairs and UpdateBroadphase reads 0 (phx_broadphase_stats has the device time)
    phase_ms[1] = 0.0;
    { RoctxRange r("UpdateBroadphase + UpdatePairs"); PHX_TRY(update_pairs()); lap(2); }            // ref: Collider.cpp:253, 288
    { RoctxRange r("UpdateManifolds"); PHX_TRY(update_manifolds()); lap(3); }                        // ref: Collider.cpp:370
    // the manifolds say which bodies hang together: the solver labels the connected components on its side stream while the joint
    // list is still being matched, extended and compacted (solver.h prelabel_components) — not with per-phase timing: the phases overlap
    // (marked here — the manifolds are final from this point of the stream on — and queued from refresh_contact_joints, once the stream has
    //  the match and its scans to run while the host queues the side stream's kernels)
    { RoctxRange r("PackManifolds"); PHX_TRY(pack_manifolds()); lap(4); }                            // ref: Collider.cpp:381
    // (marked BEHIND PackManifolds: a pack that runs here moves manifolds, and the side stream must read them where they end up —
    //  ADVICE r5; a pack that is only found necessary later, with the joint counts, voids the side stream's work: refresh_contact_joints)
    // (not in a world with an active flags column either: the side stream takes "a manifold with contact points" for a unit and reads its
    //  joints through the slots, and a sensor manifold has points and no joints — such a world's rebuild takes its components from the
    //  joints, the path PHX_NO_PRELABEL=1 takes, which is exact)
    if (flags_col_.active) PHX_TRY(solver_.cancel_prelabel());
    else if (!phase_timing) PHX_TRY(solver_.prelabel_mark());
    { RoctxRange r("RefreshContactJoints"); PHX_TRY(refresh_contact_joints()); lap(5); }             // ref: World.cpp:74
    // the pins and links edit the velocities the contacts are then solved on (include/phyx_amd.h PINS, LINKS); a world without queues nothing
    const int ordinal = break_step_++;
    if (pins_.units()) { RoctxRange r("SolvePins"); PHX_TRY(pins_.solve(resident(), nb(), dt, ordinal, rb_, stream_)); }
    return PHX_OK;
}

// A sharded world (island sharding across ranks): this rank solves only its own groups, so the step has
// two halves around the caller's all-gather of the ranks' results (exchange.h).  The unsplit entry points would integrate
// the other ranks' bodies with unsolved velocities, so they refuse to run sharded.
int World::step_begin(float dt, const phx_config& cfg, size_t* segment_bytes)
{
    PHX_TRY(pre_solve(dt));
    { RoctxRange r("SolveJoints (this rank's groups)"); PHX_TRY(solve(cfg, true)); }
    RoctxRange r("Exchange: pack");
    const BodyView bodies = resident().s;
    return solver_.exchange_pack_resident(&bodies, d_joints_.p, segment_bytes);
}

int World::step_end(float dt)
{
    mid_step_ = false;
    PHX_TRY(use_device(device_));
    { RoctxRange r("Exchange: unpack"); PHX_TRY(solver_.exchange_unpack_resident(resident().s, d_joints_.p)); }
    RoctxRange r("IntegratePosition");
    records_stale_ = true;
    ++geom_epoch_;
    if (nb()) hipLaunchKernelGGL(k_integrate_position, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), dt, (const unsigned long long*)nullptr, 0ull, MailRide{});            // ref: World.cpp:57-70
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// ---- the sharded step with the native transport (comm.hip) -------------------------------------------------------------
int World::ensure_exchange_capacity(size_t bytes)
{
    if (bytes <= xch_capacity_ && xch_send_.p) return PHX_OK;
    PHX_TRY(solver_.synchronize());
    PHX_HIP(hipStreamSynchronize(stream_));
    const size_t cap = (std::max<size_t>(2 * bytes, 1u << 20) + 255) / 256 * 256;
    PHX_TRY(xch_send_.reserve(cap / 4));
    PHX_TRY(xch_recv_.reserve(cap / 4 * (size_t)std::max(shard_count, 1)));
    xch_capacity_ = cap;
    return solver_.set_exchange_buffers(xch_send_.p, xch_recv_.p, cap);
}

int World::set_comm(Comm* c)
{
    PHX_TRY(use_device(device_));
    comm_ = c;
    agreed_seg_ = 0;
    // from here on the stream carries collectives: every host wait on it is bounded (a peer that dies or stops stepping must end
    // this rank's step with an error, not hang it — ADVICE r5)
    const double bound = c ? Comm::timeout_s() : 0.0;
    rb_.set_timeout(bound); solver_.set_wait_timeout(bound); broadphase_.set_wait_timeout(bound);
    if (!c) return PHX_OK;
    shard = c->rank(); shard_count = c->size();
    PHX_TRY(solver_.set_shard(shard, shard_count));
    xch_capacity_ = 0;                                                      // (the recv buffer is sized by the rank count)
    return ensure_exchange_capacity(1u << 20);
}

// (Any error return forgets the agreed segment size, on every rank alike — the failed one included: the next step's ranks then all
//  wait for their agreement again, whatever this step left behind.)
int World::step_sharded(float dt, const phx_config& cfg)
{
    const int st = step_sharded_inner(dt, cfg);
    mid_step_ = false;
    if (st != PHX_OK) agreed_seg_ = 0;
    return st;
}

int World::step_sharded_inner(float dt, const phx_config& cfg)
{
    if (!comm_) { set_error("phx_world_step_sharded needs a communicator (phx_world_set_comm)"); return PHX_ERR_STATE; }
    size_t seg = 0;
    int st = step_begin(dt, cfg, &seg);
    if (st == PHX_ERR_CAPACITY) {
        // the layout is a pure function of the schedule: every rank finds the same segment size too big and grows the same way;
        // the solve is done, only the pack is repeated
        PHX_TRY(ensure_exchange_capacity(solver_.exchange_segment_bytes()));
        const BodyView bodies = resident().s;
        st = solver_.exchange_pack_resident(&bodies, d_joints_.p, &seg);
    }
    // Before the collective the ranks agree on {did anybody fail in this step, the segment size} — one 16-byte all-reduce (max) QUEUED
    // on the stream in every step.  Its result is waited for on the host only by a rank that NEEDS it: one whose segment size is
    // not the size of the last agreement (the layout pads segments to 64 KB, exchange.h: in a running world that is rare), or one
    // that failed.  The steady step is therefore stream-ordered end to end again (round 4 waited for the agreement in every step);
    // healthy replicas all wait or all do not (the size is a pure function of the schedule), and:
    //   * a rank that failed learns its healthy peers' size from the result, hence whether THEY waited: if they did, they have seen
    //     its failure and nobody enters the all-gather; if they did not, they are in the all-gather already and it joins them with a
    //     header-only segment of the agreed size that carries its status (the unpack and check_exchange report it) — either way the
    //     step ends on every rank with an error and no collective is left half-entered;
    //   * sizes that differ among healthy ranks (replicas that diverged) end the step on every rank that waited.
    const std::string why = st != PHX_OK ? last_error() : std::string();
    const bool failed = st != PHX_OK;
    const int posted = comm_->agree_post(failed ? 1 : 0, failed ? 0ll : (long long)seg, stream_);
    if (posted != PHX_OK && posted != PHX_ERR_INVALID) return posted;      // (the collective itself could not be queued)
    if (failed || posted == PHX_ERR_INVALID) {
        const std::string cause = failed ? why : std::string(last_error());
        int worst = 0; long long lo = 0, hi = 0;
        PHX_TRY(comm_->agree_read(&worst, &lo, &hi, stream_));
        const bool peers_waited = lo != hi || hi != (long long)agreed_seg_;      // (no healthy peer at all: lo = 2^31 - 1, hi = 0)
        if (!peers_waited && agreed_seg_ > 0) {
            size_t hdr = 0;
            (void)solver_.exchange_pack_resident(nullptr, nullptr, &hdr, 1);      // header only: magic, serial, status
            (void)comm_->all_gather(xch_send_.p, xch_recv_.p, agreed_seg_, stream_);
        }
        set_error("%s", cause.c_str());
        return failed ? st : PHX_ERR_INVALID;
    }
    if (seg != agreed_seg_) {
        int worst = 0; long long lo = 0, hi = 0;
        agreed_seg_ = 0;
        PHX_TRY(comm_->agree_read(&worst, &lo, &hi, stream_));
        if (worst) { set_error("island-sharded step: a peer failed before the exchange (this rank's half of the step is done, nothing was exchanged)"); return PHX_ERR_STATE; }
        if (lo != hi) { set_error("island-sharded step: the ranks' segment sizes differ (%lld .. %lld bytes): the replicas diverged", lo, hi); return PHX_ERR_STATE; }
        agreed_seg_ = seg;
    }
    { RoctxRange r("Exchange: all-gather (RCCL)"); PHX_TRY(comm_->all_gather(xch_send_.p, xch_recv_.p, seg, stream_)); }
    PHX_TRY(step_end(dt));
    if ((++sharded_steps_ & 15u) == 0) PHX_TRY(check_exchange());
    return PHX_OK;
}

// the peers' headers of every exchange so far (exchange.h) and the communicator's asynchronous error state
int World::check_exchange()
{
    int bits = 0;
    PHX_TRY(solver_.exchange_status(&bits));
    if (bits) { set_error("island-sharded exchange inconsistent: PHX_XCH bits %d (1 peer error, 2 step serial, 4 topology, 8 segment never written)", bits); return PHX_ERR_STATE; }
    if (comm_) {
        int e = 0;
        PHX_TRY(comm_->async_error(&e));
        if (e) { set_error("RCCL asynchronous error %d", e); return PHX_ERR_STATE; }
    }
    return PHX_OK;
}

// [min x, max x] over the AABBs of the dynamic bodies (an ownership-sharded caller checks it against its slab, dist.py SlabWorld)
int World::x_extent(float out[2])
{
    PHX_TRY(use_device(device_));
    PHX_TRY(sync_bodies_to_device());
    PHX_TRY(flags_.reserve(4));
    const unsigned init[2] = {0xFFFFFFFFu, 0u};
    PHX_HIP(hipMemcpyAsync(flags_.p, init, sizeof init, hipMemcpyHostToDevice, stream_));
    PHX_HIP(hipStreamSynchronize(stream_));                                 // (`init` is on the stack)
    if (nb()) hipLaunchKernelGGL(k_x_extent, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), flags_.p);
    PHX_HIP(hipGetLastError());
    unsigned keys[2] = {0, 0};
    PHX_TRY(rb_.add(keys, flags_.p, sizeof keys, stream_));
    PHX_TRY(rb_.wait(stream_));
    auto unkey = [](unsigned k) { const unsigned u = (k & 0x80000000u) ? (k & 0x7FFFFFFFu) : ~k; float f; std::memcpy(&f, &u, 4); return f; };
    if (keys[0] == 0xFFFFFFFFu) { out[0] = 0.f; out[1] = 0.f; }            // no dynamic body
    else { out[0] = unkey(keys[0]); out[1] = unkey(keys[1]); }
    return PHX_OK;
}

int World::finish_step(float dt, const phx_config& cfg)
{
    using clk = std::chrono::steady_clock;
    if (shard_count > 1) { set_error("a sharded world steps through phx_world_step_begin / all-gather / phx_world_step_end"); return PHX_ERR_STATE; }
    mid_step_ = false;
    PHX_TRY(use_device(device_));
    PHX_TRY(sync_bodies_to_device());
    auto t = clk::now();
    auto lap = [&](int phase) { if (!phase_timing) return; (void)hipStreamSynchronize(stream_); auto n = clk::now(); phase_ms[phase] = std::chrono::duration<double, std::milli>(n - t).count(); t = n; };
    if (phase_timing) {                                                     // (per-phase host timing: settle the solve before the integrator)
        { RoctxRange r("SolveJoints"); PHX_TRY(solve(cfg, true)); lap(6); }
        RoctxRange r("IntegratePosition");
        ++geom_epoch_;
        if (nb()) hipLaunchKernelGGL(k_integrate_position, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), dt, (const unsigned long long*)nullptr, 0ull, MailRide{});
        PHX_HIP(hipGetLastError());
    } else PHX_TRY(solve_and_integrate(dt, cfg));
    records_stale_ = true;
    if (sleep_.on()) PHX_TRY(sleep_pass(dt));                               // (a world that never enabled sleeping queues nothing here)
    lap(7);
    return PHX_OK;
}

int World::synchronize()
{
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    if (comm_) return comm_->wait_stream(stream_, "World::synchronize");      // (bounded: the stream carries collectives)
    PHX_HIP(hipStreamSynchronize(stream_));
    return PHX_OK;
}

int World::update(float dt, const phx_config& cfg)
{
    if (shard_count > 1) { set_error("a sharded world steps through phx_world_step_begin / all-gather / phx_world_step_end"); return PHX_ERR_STATE; }
    const int st = pre_solve(dt);
    if (st != PHX_OK) { mid_step_ = false; return st; }
    return finish_step(dt, cfg);
}

#define PHX_DOWNLOAD(fn, type, buf, count_expr)                                                                    \
    int World::fn(type* out, int cap)                                                                                \
    {                                                                                                                \
        const int n = (count_expr);                                                                                  \
        if (cap < n) { set_error(#fn ": buffer too small"); return PHX_ERR_CAPACITY; }                             \
        PHX_TRY(use_device(device_));                                                                                \
        PHX_HIP(hipStreamSynchronize(stream_));                                                                      \
        if (n) PHX_HIP(hipMemcpy(out, buf.p, (size_t)n * sizeof(type), hipMemcpyDeviceToHost));                     \
        return PHX_OK;                                                                                               \
    }
PHX_DOWNLOAD(download_manifolds, phx_manifold, d_manifolds_, nm)
PHX_DOWNLOAD(download_contact_points, phx_contact_point, d_cps_, 2 * nm)
PHX_DOWNLOAD(download_joints, phx_contact_joint, d_joints_, nj)

// Restore (or hand over) a whole world: what the four getters return, put back.  The contact cache is the state the reference
// carries from step to step (ref: Collider.h:57-58 manifolds + manifoldMap, World.h:33 contactJoints with their warm-start
// impulses, ContactPoint::solverIndex linking the two); everything else a step needs is rebuilt by the step.  Used by
// checkpoint / resume and by the hand-over of bodies between the ranks of an ownership-sharded world.
int World::set_state(const phx_rigid_body* bodies, int body_count, const phx_manifold* manifolds, int manifold_count,
                     const phx_contact_point* cps, int cp_count, const phx_contact_joint* joints, int joint_count)
{
    PHX_TRY(use_device(device_));
    PHX_REQUIRE(body_count >= 0 && manifold_count >= 0 && joint_count >= 0 && cp_count == 2 * manifold_count, "bad counts (two contact-point slots per manifold)");
    PHX_REQUIRE((body_count == 0 || bodies) && (manifold_count == 0 || (manifolds && cps)) && (joint_count == 0 || joints), "null array");
    PHX_REQUIRE(shard_count == 1 && !comm_, "a sharded world cannot be restored");
    // the invariants the step's kernels rely on (shared with the snapshot blob's validator: snapshot_blob.h)
    if (const char* bad = snap_check_state(body_count, manifolds, manifold_count, cps, cp_count, joints, joint_count)) { set_error("%s", bad); return PHX_ERR_INVALID; }
    PHX_TRY(synchronize());
    host_bodies_.assign(bodies, bodies + body_count);
    bodies_dirty_ = true;
    each_table([](auto& t) { t.reset(); return PHX_OK; });                  // every optional column is the default again
    pins_.clear();                                                          // ... and no pin or link is left, no break limit and no break event
    exclusions_.clear();                                                    // ... and no pair is excluded
    break_step_ = 0;
    if (sleep_.on()) {                                                      // sleeping stays enabled: nobody asleep, the totals 0
        sleep_col_.host.assign((size_t)body_count, SleepColumn::initial());
        sleep_col_.active = true;
        PHX_TRY(sleep_.clear_totals(stream_));
    }
    PHX_TRY(sync_bodies_to_device());
    nm = manifold_count; nj = joint_count;
    PHX_TRY(d_manifolds_.reserve(std::max<size_t>(nm, 1))); PHX_TRY(d_cps_.reserve(std::max<size_t>(2 * (size_t)nm, 1))); PHX_TRY(d_joints_.reserve(std::max<size_t>(nj, 1)));
    if (nm) {
        PHX_HIP(hipMemcpyAsync(d_manifolds_.p, manifolds, (size_t)nm * sizeof(phx_manifold), hipMemcpyHostToDevice, stream_));
        PHX_HIP(hipMemcpyAsync(d_cps_.p, cps, 2 * (size_t)nm * sizeof(phx_contact_point), hipMemcpyHostToDevice, stream_));
    }
    if (nj) PHX_HIP(hipMemcpyAsync(d_joints_.p, joints, (size_t)nj * sizeof(phx_contact_joint), hipMemcpyHostToDevice, stream_));
    PHX_HIP(hipStreamSynchronize(stream_));
    std::vector<uint2> pairs((size_t)nm);
    for (int i = 0; i < nm; ++i) pairs[i] = make_uint2((unsigned)manifolds[i].body1, (unsigned)manifolds[i].body2);
    PHX_TRY(broadphase_.reset_pairs(pairs.data(), nm));
    PHX_TRY(forget_step_history());
    ++contact_epoch_;
    std::vector<unsigned long long> touching;                               // the events' baseline: T(restored state)
    for (int i = 0; i < nm; ++i)
        if (manifolds[i].point_count > 0) touching.push_back(((unsigned long long)(unsigned)manifolds[i].body1 << 32) | (unsigned)manifolds[i].body2);
    std::sort(touching.begin(), touching.end());
    touching.erase(std::unique(touching.begin(), touching.end()), touching.end());
    PHX_TRY(contacts_.set_baseline(touching, stream_));
    PHX_HIP(hipStreamSynchronize(stream_));
    return PHX_OK;
}

// nothing of the old world's bookkeeping survives: the schedule is rebuilt, no pack or joint match is pending, the velocity step is
// not fused yet, and the joints' match stamps start again from zero
int World::forget_step_history()
{
    joints_changed_ = true; pack_pending_ = false; expect_no_dead_manifolds_ = false; fresh_manifolds_ = 0; manifolds_updated_ = 0; fuse_velocity_ = false; mid_step_ = false;
    if (joint_seen_.p) { PHX_HIP(hipMemsetAsync(joint_seen_.p, 0, joint_seen_.cap * sizeof(unsigned), stream_)); }
    joint_epoch_ = 0;
    return PHX_OK;
}

// ---- snapshots ---------------------------------------------------------------------------------------------------------------------
// Defined in include/phyx_amd.h SNAPSHOTS: a load leaves exactly the world that phx_world_set_state of the saved arrays, the three
// column setters and B := saved B would have made.  Here the state never leaves HBM: one kernel each way on the world's stream
// (snapshot.hip), and the host does what set_state's tail and the removal's do — the counts are on the host between steps.
int World::snapshot_guard(const char* what, const Snapshot& s) const
{
    PHX_TRY(refuse_mid_step(what));
    if (shard_count > 1 || comm_) { set_error("%s: a sharded world has no snapshots", what); return PHX_ERR_STATE; }
    if (sleep_.on()) { set_error("%s: sleeping is enabled and a snapshot does not carry the sleep states (phx_world_set_sleeping(w, NULL) first)", what); return PHX_ERR_STATE; }
    if (s.device() != device_) { set_error("%s: the snapshot lives on device %d, the world on device %d (move it as a blob)", what, s.device(), device_); return PHX_ERR_INVALID; }
    return PHX_OK;
}

SnapshotWorld World::snapshot_view()
{
    SnapshotWorld v = {};
    v.records = bodies_.records.p; v.resident = resident(); v.records_stale = records_stale_;
    v.accel = accel_.p;
    v.manifolds = d_manifolds_.p; v.cps = d_cps_.p; v.joints = d_joints_.p;
    v.filters = filters_.dev.p; v.materials = materials_.dev.p; v.flags = flags_col_.dev.p;
    v.baseline = contacts_.baseline();
    v.pairs = rm_pairs_.p;
    return v;
}

int World::save(Snapshot& s)
{
    static const char* const what = "phx_world_save";
    PHX_TRY(snapshot_guard(what, s));
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before its results are read)
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    PHX_TRY(settle_breaks());
    SnapshotWorld v = snapshot_view();
    v.counts.bodies = nb(); v.counts.manifolds = nm; v.counts.joints = nj; v.counts.baseline = contacts_.baseline_count();
    v.counts.columns = (filters_.active ? SNAP_HAS_FILTERS : 0) | (materials_.active ? SNAP_HAS_MATERIALS : 0) | (flags_col_.active ? SNAP_HAS_FLAGS : 0);
    v.accel_pending = accel_pending_;      // (while it is clear every record's accelerations are zero: IntegrateVelocity clears them)
    PHX_TRY(pins_.upload(stream_));
    PHX_TRY(exclusions_.sync(nb(), stream_));
    PHX_TRY(pins_.each_list([&](auto& l) { return s.reserve_units<typename std::decay_t<decltype(l)>::record>(l.count(), l.limited(), stream_); }));
    PHX_TRY(s.reserve_exclusions(exclusions_.count(), stream_));
    PHX_TRY(s.save(v, stream_));
    PHX_TRY(pins_.each_list([&](auto& l) { return s.save_units(l.device(), l.device_limits(), l.count(), stream_); }));
    return s.save_exclusions(exclusions_.device_pairs(), exclusions_.count(), stream_);
}

int World::load(Snapshot& s)
{
    static const char* const what = "phx_world_load";
    PHX_TRY(snapshot_guard(what, s));
    if (!s.filled()) { set_error("%s: the snapshot was never filled (phx_world_save, phx_snapshot_import)", what); return PHX_ERR_STATE; }
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before anything is replaced)
    const SnapCounts& c = s.counts();
    const size_t n = (size_t)c.bodies;
    // room first (a buffer that has to grow is replaced: its contents go anyway); nothing of the world changes before the kernel is queued
    PHX_TRY(bodies_.reserve(std::max<size_t>(n, 1)));
    if (s.accel_pending()) PHX_TRY(accel_.reserve(std::max<size_t>(n, 1)));
    PHX_TRY(d_manifolds_.reserve(std::max<size_t>((size_t)c.manifolds, 1))); PHX_TRY(d_cps_.reserve(std::max<size_t>(2 * (size_t)c.manifolds, 1)));
    PHX_TRY(d_joints_.reserve(std::max<size_t>((size_t)c.joints, 1)));
    PHX_TRY(rm_pairs_.reserve(std::max<size_t>((size_t)c.manifolds, 1)));
    if (c.columns & SNAP_HAS_FILTERS) PHX_TRY(filters_.dev.reserve(std::max<size_t>(n, 1)));
    if (c.columns & SNAP_HAS_MATERIALS) PHX_TRY(materials_.dev.reserve(std::max<size_t>(n, 1)));
    if (c.columns & SNAP_HAS_FLAGS) PHX_TRY(flags_col_.dev.reserve(std::max<size_t>(n, 1)));
    PHX_TRY(contacts_.reserve_baseline((size_t)c.baseline));
    PHX_TRY(s.load(snapshot_view(), stream_));
    // the device copy is the world (host-staged bodies and tables are dropped with the rest of the old world)
    host_bodies_.resize(n);                                                 // (only its size counts while the device copy is the world)
    bodies_dirty_ = false;
    records_stale_ = false;
    accel_pending_ = s.accel_pending();
    filters_.active = (c.columns & SNAP_HAS_FILTERS) != 0; materials_.active = (c.columns & SNAP_HAS_MATERIALS) != 0; flags_col_.active = (c.columns & SNAP_HAS_FLAGS) != 0;
    each_table([](auto& t) { t.host.clear(); return PHX_OK; });
    nm = c.manifolds; nj = c.joints;
    contacts_.baseline_replaced(c.baseline);
    ++geom_epoch_;
    ++contact_epoch_;
    // what set_state resets: the pair set becomes the saved manifolds' pairs, the schedule is rebuilt at the next step
    PHX_TRY(broadphase_.reset_pairs_device(rm_pairs_.p, nm));
    PHX_TRY(forget_step_history());
    pins_.drop_breaks();                                                    // (the abandoned timeline's unsettled breaks and its events go with it)
    break_step_ = 0;
    PHX_TRY(pins_.each_list([&](auto& l) {                                  // 6. add_pins, add_links, add_angles, add_sliders of the saved ones, with their break limits
        using P = typename std::decay_t<decltype(l)>::record;
        return pins_.adopt_device(s.units<P>(), s.unit_limits<P>(), s.unit_count<P>(), stream_);
    }));
    return exclusions_.adopt_device(s.exclusions(), s.exclusion_count(), stream_);      // 7. add_collision_exclusions of the saved ones (no manifold holds one)
}

int World::get_slab_state(const long long* global_index, int count, SlabState* out)
{
    if (count != nb()) { set_error("re-slab: %d scene indices for a world of %d bodies", count, nb()); return PHX_ERR_INVALID; }
    out->global_index.assign(global_index, global_index + count);
    out->bodies.resize((size_t)nb()); out->manifolds.resize((size_t)nm); out->cps.resize(2 * (size_t)nm); out->joints.resize((size_t)nj);
    PHX_TRY(download_bodies(out->bodies.data(), nb()));
    PHX_TRY(download_manifolds(out->manifolds.data(), nm));
    PHX_TRY(download_contact_points(out->cps.data(), 2 * nm));
    PHX_TRY(download_joints(out->joints.data(), nj));
    return PHX_OK;
}

int World::download_bodies(phx_rigid_body* out, int cap)
{
    const int n = nb();
    if (cap < n) { set_error("download_bodies: buffer too small"); return PHX_ERR_CAPACITY; }
    if (host_staged()) { if (n && out != host_bodies_.data()) std::memcpy(out, host_bodies_.data(), (size_t)n * sizeof(phx_rigid_body)); return PHX_OK; }
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before its results are read)
    PHX_TRY(refresh_records());
    PHX_HIP(hipStreamSynchronize(stream_));
    if (n) PHX_HIP(hipMemcpy(out, bodies_.records.p, (size_t)n * sizeof(phx_rigid_body), hipMemcpyDeviceToHost));
    return PHX_OK;
}

// ---- edits and gathers between steps ------------------------------------------------------------------------------------------
// The reference's application writes into its public RigidBody array before every Update (ref: main.cpp:337-346: the mouse drag).
// Here an edit is a batch of body indices with values from host memory: checked completely first (all of it or none of it), then
// either written into the host-staged records (bodies_dirty_: before the first step, after add_body / set_inverse_mass / set_static),
// or staged through pinned memory and scattered by one kernel queued on the stream — no host wait for a step still in flight.
// (`edit`: an edit — refused inside a step, every index at most once — rather than a gather)
int World::check_batch(const char* what, const int* bodies, const void* values, int count, bool edit)
{
    if (edit) PHX_TRY(refuse_mid_step(what));
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && (!bodies || !values)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = nb();
    for (int k = 0; k < count; ++k)
        if (bodies[k] < 0 || bodies[k] >= n) { set_error("%s: body index %d out of range [0, %d)", what, bodies[k], n); return PHX_ERR_INVALID; }
    if (!edit || count < 2) return PHX_OK;
    if (edit_seen_.size() < (size_t)n) { edit_seen_.assign((size_t)n, 0u); edit_epoch_ = 0; }
    if (++edit_epoch_ == 0) { std::fill(edit_seen_.begin(), edit_seen_.end(), 0u); edit_epoch_ = 1; }
    for (int k = 0; k < count; ++k) {
        unsigned& seen = edit_seen_[(size_t)bodies[k]];
        if (seen == edit_epoch_) { set_error("%s: body %d appears twice in one call", what, bodies[k]); return PHX_ERR_INVALID; }
        seen = edit_epoch_;
    }
    return PHX_OK;
}

// {indices | values} in one H2D copy (values only when `bodies` is null).  The pinned buffer is bump-allocated while earlier batches' copies are still queued (they may sit
// behind a step in flight) and reused from the start once stage_done_ has passed; an outgrown buffer is kept until the world goes.
int World::stage_batch(const int* bodies, const float* values, int count, int width, const int** d_bodies, const float** d_values)
{
    const size_t ib = bodies ? ((size_t)count * sizeof(int) + 15) & ~size_t(15) : 0, bytes = ib + (size_t)count * (size_t)width * sizeof(float);
    if (!stage_done_) PHX_HIP(hipEventCreateWithFlags(&stage_done_, hipEventDisableTiming));
    else if (stage_used_) {
        const hipError_t q = hipEventQuery(stage_done_);
        if (q == hipSuccess) stage_used_ = 0;
        else if (q != hipErrorNotReady) { set_error("staging: %s", hipGetErrorString(q)); return PHX_ERR_HIP; }
    }
    size_t off = (stage_used_ + 15) & ~size_t(15);
    if (off + bytes > stage_cap_) {
        const size_t cap = std::max<size_t>(std::max<size_t>(2 * bytes, 2 * stage_cap_), 64u << 10);
        if (stage_pin_) stage_retired_.push_back(stage_pin_);
        stage_pin_ = nullptr; stage_cap_ = 0;
        PHX_HIP(hipHostMalloc(reinterpret_cast<void**>(&stage_pin_), cap, hipHostMallocDefault));
        stage_cap_ = cap;
        off = 0;
    }
    if (bytes > edit_dev_.cap && edit_dev_.p) edit_dev_retired_.push_back(std::move(edit_dev_));
    PHX_TRY(edit_dev_.reserve(bytes));
    if (bodies) std::memcpy(stage_pin_ + off, bodies, (size_t)count * sizeof(int));
    if (width) std::memcpy(stage_pin_ + off + ib, values, bytes - ib);
    PHX_HIP(hipMemcpyAsync(edit_dev_.p, stage_pin_ + off, bytes, hipMemcpyHostToDevice, stream_));
    PHX_HIP(hipEventRecord(stage_done_, stream_));
    stage_used_ = off + bytes;
    *d_bodies = bodies ? reinterpret_cast<const int*>(edit_dev_.p) : nullptr;
    *d_values = reinterpret_cast<const float*>(edit_dev_.p + ib);
    return PHX_OK;
}

int World::edit(Edit kind, const int* bodies, const float* values, int count)
{
    static const char* const what[] = {"phx_world_add_accelerations", "phx_world_set_velocities", "phx_world_set_poses"};
    PHX_TRY(check_batch(what[kind], bodies, values, count, true));
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(bodies, count));
    const int width = kind == EDIT_POSES ? 6 : 3;
    if (host_staged()) {                                    // the host-staged records are the world: write into them
        for (int k = 0; k < count; ++k) {
            phx_rigid_body& b = host_bodies_[(size_t)bodies[k]];
            const float* v = values + (size_t)width * k;
            if (kind == EDIT_ACCELERATIONS) { b.acceleration.x += v[0]; b.acceleration.y += v[1]; b.angular_acceleration += v[2]; }
            else if (kind == EDIT_VELOCITIES) { b.velocity.x = v[0]; b.velocity.y = v[1]; b.angular_velocity = v[2]; }
            else { b.pos.x = v[0]; b.pos.y = v[1]; b.xvector.x = v[2]; b.xvector.y = v[3]; b.yvector.x = v[4]; b.yvector.y = v[5]; update_geom(b); }
        }
        return PHX_OK;
    }
    PHX_TRY(settle_on_device());
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_batch(bodies, values, count, width, &d_bodies, &d_values));
    if (kind == EDIT_ACCELERATIONS) {
        // the next IntegrateVelocity consumes accel_ (ref: World.cpp:44-53); the first edit after a step starts it from zero on the device
        if (!accel_pending_) {
            PHX_TRY(accel_.reserve((size_t)nb()));
            PHX_HIP(hipMemsetAsync(accel_.p, 0, (size_t)nb() * sizeof(float4), stream_));
            accel_pending_ = true;
        }
        hipLaunchKernelGGL(k_add_accelerations, dim3(wgrid(count)), dim3(256), 0, stream_, d_bodies, d_values, count, accel_.p, bodies_.records.p);
    } else if (kind == EDIT_VELOCITIES) {
        hipLaunchKernelGGL(k_set_velocities, dim3(wgrid(count)), dim3(256), 0, stream_, d_bodies, d_values, count, bodies_.vel.p);
        records_stale_ = true;
    } else {
        hipLaunchKernelGGL(k_set_poses, dim3(wgrid(count)), dim3(256), 0, stream_, d_bodies, d_values, count, resident());
        ++geom_epoch_;
        records_stale_ = true;
    }
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int World::get_body_states(const int* bodies, int count, phx_rigid_body* out)
{
    PHX_TRY(check_batch("phx_world_get_body_states", bodies, out, count, false));
    if (!count) return PHX_OK;
    if (host_staged()) {
        for (int k = 0; k < count; ++k) out[k] = host_bodies_[(size_t)bodies[k]];
        return PHX_OK;
    }
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before its results are read)
    const int* d_bodies = nullptr; const float* unused = nullptr;
    PHX_TRY(stage_batch(bodies, nullptr, count, 0, &d_bodies, &unused));
    PHX_TRY(gathered_.reserve((size_t)count));
    hipLaunchKernelGGL(k_gather_bodies, dim3(wgrid(count)), dim3(256), 0, stream_, resident(), (const phx_rigid_body*)bodies_.records.p, d_bodies, count, gathered_.p);
    PHX_HIP(hipGetLastError());
    PHX_TRY(rb_.add(out, gathered_.p, (size_t)count * sizeof(phx_rigid_body), stream_));
    return rb_.wait(stream_);
}

int World::get_poses(float* out, int cap)
{
    const int n = nb();
    if (cap < n) { set_error("phx_world_get_poses: room for %d bodies, the world has %d", cap, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    if (host_staged()) {
        for (int i = 0; i < n; ++i) {
            const phx_rigid_body& b = host_bodies_[(size_t)i];
            out[4 * i] = b.pos.x; out[4 * i + 1] = b.pos.y; out[4 * i + 2] = b.xvector.x; out[4 * i + 3] = b.xvector.y;
        }
        return PHX_OK;
    }
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    PHX_TRY(poses_.reserve((size_t)n));
    hipLaunchKernelGGL(k_world_poses, dim3(wgrid(n)), dim3(256), 0, stream_, resident(), n, poses_.p);
    PHX_HIP(hipGetLastError());
    PHX_TRY(rb_.add(out, poses_.p, (size_t)n * sizeof(float4), stream_));
    return rb_.wait(stream_);
}

int World::get_poses_device(void* d_out, int cap)
{
    const int n = nb();
    if (cap < n) { set_error("phx_world_get_poses_device: room for %d bodies, the world has %d", cap, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    if (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 15u)) { set_error("phx_world_get_poses_device: the output must be a 16-byte aligned device pointer"); return PHX_ERR_INVALID; }
    PHX_TRY(settle_on_device());                                            // (nothing is pending while the bodies are host-staged: every call that stages them settles first)
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    hipLaunchKernelGGL(k_world_poses, dim3(wgrid(n)), dim3(256), 0, stream_, resident(), n, static_cast<float4*>(d_out));
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// ---- the compaction of the contact cache (a removal, a change of collision filters, a new collision exclusion) ----------------------
// Kept manifolds and joints keep their old order: their new positions are exclusive scans of the keep predicate (world_kernels.h
// BodiesKept / FilterKept / ExclusionKept; rm_counts_[1], [2] receive the kept counts), and two kernels write them out of place into the spares, with
// the kept manifolds' pairs in rm_pairs_ (the new broadphase pair set).  Grid-strided over the OLD counts: no host count needed.
int World::compaction_scratch()
{
    PHX_TRY(rm_counts_.reserve(5));
    PHX_TRY(rm_mnew_.reserve((size_t)nm + 2)); PHX_TRY(rm_jnew_.reserve((size_t)nj + 2)); PHX_TRY(rm_pairs_.reserve(std::max<size_t>(nm, 1)));
    PHX_TRY(spare_.manifolds.reserve(std::max<size_t>(nm, 1))); PHX_TRY(spare_.cps.reserve(std::max<size_t>(2 * (size_t)nm, 1))); PHX_TRY(spare_.joints.reserve(std::max<size_t>(nj, 1)));
    return PHX_OK;
}

template <class Keep>
int World::scan_compaction(const Keep& kept)
{
    PHX_TRY(device_exclusive_scan_of(ManifoldKeepLoad<Keep>{d_manifolds_.p, kept}, rm_mnew_.p, nm, rm_counts_.p + 1, scan_tiles_, stream_));
    return device_exclusive_scan_of(JointKeepLoad<Keep>{d_joints_.p, d_manifolds_.p, kept}, rm_jnew_.p, nj, rm_counts_.p + 2, scan_tiles_, stream_);
}

template <class Keep>
int World::queue_compaction(const Keep& kept)
{
    if (nm) hipLaunchKernelGGL((k_remove_manifolds<Keep>), dim3(rgrid(nm)), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, (const phx_contact_point*)d_cps_.p, nm,
                               kept, (const unsigned*)rm_mnew_.p, (const unsigned*)rm_jnew_.p, (const unsigned*)(rm_counts_.p + 2), nj, spare_.manifolds.p, spare_.cps.p, rm_pairs_.p);
    if (nj) hipLaunchKernelGGL((k_remove_joints<Keep>), dim3(rgrid(nj)), dim3(256), 0, stream_, (const phx_contact_joint*)d_joints_.p, nj, (const phx_manifold*)d_manifolds_.p,
                               kept, (const unsigned*)rm_mnew_.p, (const unsigned*)rm_jnew_.p, spare_.joints.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// rm_counts_ as the round trip brought them back: [1] manifolds, [2] joints kept.  The compacted cache changes places with the world's,
// the pair set is reset to its pairs and the step history is forgotten, as set_state would.
int World::adopt_compaction(const unsigned got[5])
{
    std::swap(d_manifolds_, spare_.manifolds); std::swap(d_cps_, spare_.cps); std::swap(d_joints_, spare_.joints);
    nm = (int)got[1]; nj = (int)got[2];
    PHX_TRY(broadphase_.reset_pairs_device(rm_pairs_.p, nm));
    return forget_step_history();
}

// ---- removal between steps ------------------------------------------------------------------------------------------------------
// Defined as phx_world_set_state of the filtered state (include/phyx_amd.h); computed on the world's stream without the state
// crossing PCIe: keep flags per body (scattered from the staged list, or the box test on the resident AABBs), three exclusive scans
// (bodies; manifolds: both bodies kept; joints: their manifold kept), then the compaction kernels, out of place into the spare
// buffers, grid-strided over the OLD counts — all queued before the one host round trip that brings back the three new counts (and
// the remap if asked for).  The records are compacted as the truth and the resident arrays made from them by the upload's own
// conversion, so the result is set_state's by construction.
int World::remove(const char* what, const int* bodies, int count, const float* box, int* removed, int* remap)
{
    if (shard_count > 1 || comm_) { set_error("%s: a sharded world cannot remove bodies", what); return PHX_ERR_STATE; }
    if (box) {
        PHX_TRY(refuse_mid_step(what));
        for (int k = 0; k < 4; ++k)
            if (!std::isfinite(box[k])) { set_error("%s: the box is not finite", what); return PHX_ERR_INVALID; }
        if (!(box[0] <= box[2] && box[1] <= box[3])) { set_error("%s: the box's min exceeds its max", what); return PHX_ERR_INVALID; }
    } else PHX_TRY(check_batch(what, bodies, bodies, count, true));        // (no values: the indices stand in for them)
    const int n = nb();
    if (removed) *removed = 0;
    if ((!box && !count) || !n) {                                           // a true no-op: the cached schedule stays valid
        if (remap) for (int i = 0; i < n; ++i) remap[i] = i;
        return PHX_OK;
    }
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before anything moves)
    PHX_TRY(settle_breaks());
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    PHX_TRY(rm_keep_.reserve((size_t)n + 2)); PHX_TRY(rm_bnew_.reserve((size_t)n + 2)); PHX_TRY(rm_remap_.reserve((size_t)n));
    PHX_TRY(spare_.bodies.reserve((size_t)n));
    if (accel_pending_) PHX_TRY(spare_.accel.reserve((size_t)n));
    PHX_TRY(each_table([n](auto& t) { return t.reserve_spare((size_t)n); }));
    PHX_TRY(compaction_scratch());
    // 1. keep flags per body
    if (box) {
        hipLaunchKernelGGL(k_keep_inside, dim3(rgrid(n)), dim3(256), 0, stream_, (const float4*)bodies_.aabb.p, n, make_float4(box[0], box[1], box[2], box[3]), rm_keep_.p);
    } else {
        const int* d_bodies = nullptr; const float* unused = nullptr;
        PHX_TRY(stage_batch(bodies, nullptr, count, 0, &d_bodies, &unused));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rm_keep_.p), 1, (size_t)n, stream_));
        hipLaunchKernelGGL(k_remove_listed, dim3(rgrid(count)), dim3(256), 0, stream_, d_bodies, count, rm_keep_.p);
    }
    PHX_HIP(hipGetLastError());
    PHX_TRY(wake_named(nullptr, 0, rm_keep_.p));                            // (the sleeping components that lose a member wake before anything moves)
    // 2. where the kept bodies, manifolds and joints go (a zero count writes a zero total)
    PHX_TRY(device_exclusive_scan_of(BodyKeepLoad{rm_keep_.p}, rm_bnew_.p, n, rm_counts_.p, scan_tiles_, stream_));
    const BodiesKept kept{rm_keep_.p, rm_bnew_.p};
    PHX_TRY(scan_compaction(kept));
    PHX_HIP(hipMemsetAsync(rm_counts_.p + 3, 0, sizeof(unsigned), stream_));
    // 3. compaction into the spares
    hipLaunchKernelGGL(k_remove_bodies, dim3(rgrid(n)), dim3(256), 0, stream_, (const phx_rigid_body*)bodies_.records.p, resident(), n, records_stale_ ? 1 : 0,
                       (const unsigned*)rm_keep_.p, (const unsigned*)rm_bnew_.p, spare_.bodies.records.p, spare_.bodies.view(), rm_remap_.p, rm_counts_.p + 3,
                       columns(), spare_columns());
    PHX_TRY(queue_compaction(kept));
    PHX_HIP(hipGetLastError());
    PHX_TRY(contacts_.remap_baseline(rm_remap_.p, rm_counts_.p + 4, stream_));      // (the events' baseline through new[]: [4] its new size)
    // 4. the one round trip
    unsigned got[5] = {0, 0, 0, 0, 0};
    PHX_TRY(rb_.add(got, rm_counts_.p, sizeof got, stream_));
    if (remap) PHX_TRY(rb_.add(remap, rm_remap_.p, (size_t)n * sizeof(int), stream_));
    PHX_TRY(rb_.wait(stream_));
    const int kept_bodies = (int)got[0];
    if (removed) *removed = n - kept_bodies;
    if (kept_bodies == n) return PHX_OK;                                    // every body is inside the box: nothing changes (the spares are dropped)
    // 5. the compacted arrays become the world's
    std::swap(bodies_, spare_.bodies);
    if (accel_pending_) std::swap(accel_, spare_.accel);
    each_table([](auto& t) { t.adopt_spare(); return PHX_OK; });
    host_bodies_.resize((size_t)kept_bodies);                               // (only its size counts while the device copy is the world)
    ++geom_epoch_;
    ++contact_epoch_;
    contacts_.baseline_remapped(got[4]);
    records_stale_ = false;
    accel_pending_ = accel_pending_ && got[3] != 0;                         // (what the upload of the kept records would find)
    PHX_TRY(adopt_compaction(got));
    PHX_TRY(exclusions_.bodies_removed(rm_remap_.p, rb_, stream_));         // (the excluded pairs of the removed bodies go, the rest through new[])
    return pins_.bodies_removed(rm_remap_.p, rb_, stream_);                 // (the pins of the removed bodies go, the rest through new[])
}

// ---- spawn between steps ---------------------------------------------------------------------------------------------------------
// Appending bodies is add_body's record, `count` times over.  Before the first step (host-staged bodies) that is literally what runs.
// After it, the host builds each body's row from body_record — the frame and the two inverse masses, 40 bytes — and one kernel writes
// the records and the resident state behind whatever the stream holds.  The body buffers grow geometrically, keeping their contents
// (a buffer that grows waits for the stream once).  The new bodies are in no joint and no pair: the solver keeps its cached schedule
// and the broadphase its splitters (DeviceSolver::bodies_appended, DeviceBroadphase::bodies_appended).
constexpr int SPAWN_ROW = 10;      // {pos.x, pos.y, half x, half y, inv_mass, inv_inertia, xv.x, xv.y, yv.x, yv.y}

int World::add_bodies(const float* spawn, int count, int* first)
{
    static const char* const what = "phx_world_add_bodies";
    PHX_TRY(refuse_mid_step(what));
    if (shard_count > 1 || comm_) { set_error("%s: a sharded world cannot spawn bodies", what); return PHX_ERR_STATE; }
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && !spawn) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = nb();
    if ((long long)n + count > (long long)INT32_MAX) { set_error("%s: %d + %d bodies exceed the int32 range", what, n, count); return PHX_ERR_INVALID; }
    for (int k = 0; k < count; ++k) {
        const float* q = spawn + 5 * (size_t)k;
        for (int c = 0; c < 5; ++c)
            if (!std::isfinite(q[c])) { set_error("%s: body %d: value %d is not finite", what, k, c); return PHX_ERR_INVALID; }
        if (!(q[3] > 0.f && q[4] > 0.f)) { set_error("%s: body %d: half sizes must be positive", what, k); return PHX_ERR_INVALID; }
    }
    if (first) *first = n;
    if (!count) return PHX_OK;
    if (host_staged()) {                                    // host-staged: exactly `count` add_body calls
        host_bodies_.reserve((size_t)n + count);
        for (int k = 0; k < count; ++k) { const float* q = spawn + 5 * (size_t)k; add_body(q[0], q[1], q[2], q[3], q[4]); }
        return PHX_OK;
    }
    PHX_TRY(settle_on_device());
    spawn_rows_.resize((size_t)count * SPAWN_ROW);
    bool any_static = false;
    for (int k = 0; k < count; ++k) {
        const float* q = spawn + 5 * (size_t)k;
        const phx_rigid_body b = body_record(q[0], q[1], q[2], q[3], q[4]);
        float* r = spawn_rows_.data() + (size_t)SPAWN_ROW * k;
        r[0] = b.pos.x; r[1] = b.pos.y; r[2] = b.geom_size.x; r[3] = b.geom_size.y; r[4] = b.inv_mass; r[5] = b.inv_inertia;
        r[6] = b.xvector.x; r[7] = b.xvector.y; r[8] = b.yvector.x; r[9] = b.yvector.y;
        any_static |= b.inv_mass == 0.f && b.inv_inertia == 0.f;           // (sizes so large that the mass overflows: a static body)
    }
    const size_t total = (size_t)n + count;
    PHX_TRY(bodies_.reserve_keep(total, n, stream_));
    if (accel_pending_) PHX_TRY(accel_.reserve_keep(total, n, stream_));
    PHX_TRY(each_table([&](auto& t) { return t.grow(total, n, stream_); }));
    const int* unused = nullptr; const float* d_rows = nullptr;
    PHX_TRY(stage_batch(nullptr, spawn_rows_.data(), count, SPAWN_ROW, &unused, &d_rows));
    hipLaunchKernelGGL(k_spawn_bodies, dim3(wgrid(count)), dim3(256), 0, stream_, d_rows, count, n, resident(), bodies_.records.p, columns());
    PHX_HIP(hipGetLastError());
    host_bodies_.resize(total);                                             // (only its size counts while the device copy is the world)
    ++geom_epoch_;
    ++contact_epoch_;                                                       // (the index's offsets are sized by the bodies)
    if (any_static) joints_changed_ = true;                                 // (the static set is part of the schedule)
    PHX_TRY(solver_.bodies_appended(n, (int)total));
    broadphase_.bodies_appended(n, (int)total);
    return PHX_OK;
}

// body->invMass, body->invInertia of a batch (phx_world_set_inverse_masses): an edit that changes the schedule's static set
int World::set_inverse_masses(const int* bodies, const float* values, int count)
{
    static const char* const what = "phx_world_set_inverse_masses";
    PHX_TRY(check_batch(what, bodies, values, count, true));
    for (int k = 0; k < 2 * count; ++k)
        if (!std::isfinite(values[k]) || !(values[k] >= 0.f)) { set_error("%s: entry %d: inverse masses must be finite and >= 0", what, k / 2); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(bodies, count));                                     // (a sleeper's own masses come back first; the new values then apply)
    joints_changed_ = true;                                                 // which bodies are static is part of the schedule's topology
    pins_.statics_changed();
    if (host_staged()) {
        for (int k = 0; k < count; ++k) { phx_rigid_body& b = host_bodies_[(size_t)bodies[k]]; b.inv_mass = values[2 * k]; b.inv_inertia = values[2 * k + 1]; }
        return PHX_OK;
    }
    PHX_TRY(settle_on_device());
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_batch(bodies, values, count, 2, &d_bodies, &d_values));
    hipLaunchKernelGGL(k_set_inverse_masses, dim3(wgrid(count)), dim3(256), 0, stream_, d_bodies, d_values, count, bodies_.mpos.p, bodies_.records.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// ---- the optional columns' setters ---------------------------------------------------------------------------------------------
// One skeleton for the three (phx_world_set_collision_filters / set_materials / set_body_flags).  A sharded world is refused before anything else (also inside a step); then the batch and `rule` for
// every entry, all of it or none of it; a host-staged world's table is the host's (where `host_path_ok`), otherwise the batch is
// staged as 4-byte words (world_kernels.h) and scattered behind a settled solve.
template <class Column, class Rule>
int World::set_column(const char* what, BodyTable<Column>& table, const int32_t* bodies, const typename Column::api* values, int count, Rule rule, bool host_path_ok)
{
    PHX_TRY(refuse_sharded(what, Column::plural));
    PHX_TRY(check_batch(what, bodies, values, count, true));
    for (int k = 0; k < count; ++k) PHX_TRY(rule(k));
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(bodies, count));
    const int n = nb();
    if (host_staged() && host_path_ok) { table.set_host(bodies, values, count, n); return PHX_OK; }      // (the table goes up with the bodies)
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before the table changes)
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_batch(bodies, reinterpret_cast<const float*>(values), count, (int)(sizeof(typename Column::api) / sizeof(float)), &d_bodies, &d_values));
    return table.set_device(d_bodies, d_values, count, n, stream_);
}

// ---- collision filters ------------------------------------------------------------------------------------------------------------
// The rule and the defaults: include/phyx_amd.h COLLISION FILTERS, common.h collision_filter_pass.  The broadphase applies it inside the
// sweep (broadphase.hip FilteredSweepView), so a failing pair is never emitted; what a change of filters does to pairs that exist already
// is the removal's compaction of the contact cache with the filter as its keep predicate (FilterKept), bodies untouched.
int World::set_collision_filters(const int32_t* bodies, const phx_collision_filter* filters, int count, int* dropped)
{
    PHX_TRY(set_column("phx_world_set_collision_filters", filters_, bodies, filters, count, [](int) { return PHX_OK; }, !nm));      // (on the host while no pair exists to drop)
    if (dropped) *dropped = 0;
    if (!count || !nm) return PHX_OK;
    // the manifolds whose pair now fails go, with their slots and joints; the one round trip brings back the kept counts
    PHX_TRY(compaction_scratch());
    const FilterKept kept{filters_.dev.p};
    PHX_TRY(scan_compaction(kept));
    PHX_TRY(queue_compaction(kept));
    unsigned got[5] = {0, 0, 0, 0, 0};
    PHX_TRY(rb_.add(got, rm_counts_.p, sizeof got, stream_));
    PHX_TRY(rb_.wait(stream_));
    if (dropped) *dropped = nm - (int)got[1];
    if ((int)got[1] == nm) return PHX_OK;                                   // nothing dropped: a true no-op for the topology (the spares are dropped)
    ++contact_epoch_;                                                       // (the touch events' baseline stays: dropped pairs end)
    return adopt_compaction(got);
}

// ---- collision exclusions ---------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h COLLISION EXCLUSIONS; the set and its device side: exclusions.h.  The broadphase applies it inside the
// sweep behind the filter (broadphase.hip ExcludedSweepView); what an add does to pairs that exist already is set_collision_filters' own
// path with "the pair is not in the set" as the keep predicate (ExclusionKept).
// the checks of a pair list, all of them before anything changes; `keys`: the normalised keys in the call's order
int World::check_exclusion_pairs(const char* what, const int32_t* pairs, int count, std::vector<unsigned long long>* keys)
{
    PHX_TRY(refuse_sharded(what, "collision exclusions"));
    PHX_TRY(refuse_mid_step(what));
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && !pairs) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = nb();
    keys->clear();
    for (int k = 0; k < count; ++k) {
        const int a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
        if (a < 0 || a >= n || b < 0 || b >= n) { set_error("%s: pair %d: body index %d out of range [0, %d)", what, k, a < 0 || a >= n ? a : b, n); return PHX_ERR_INVALID; }
        if (a == b) { set_error("%s: pair %d names body %d twice", what, k, a); return PHX_ERR_INVALID; }
        keys->push_back(ps_unordered_key((unsigned)a, (unsigned)b));
    }
    if (count > 1) {
        std::vector<unsigned long long> sorted(*keys);
        std::sort(sorted.begin(), sorted.end());
        const auto twice = std::adjacent_find(sorted.begin(), sorted.end());
        if (twice != sorted.end()) {
            set_error("%s: the pair (%u, %u) appears twice in one call", what, (unsigned)(*twice >> 32), (unsigned)*twice);
            return PHX_ERR_INVALID;
        }
    }
    return PHX_OK;
}

int World::add_collision_exclusions(const int32_t* pairs, int count, int* dropped)
{
    static const char* const what = "phx_world_add_collision_exclusions";
    std::vector<unsigned long long> keys;
    PHX_TRY(check_exclusion_pairs(what, pairs, count, &keys));
    if (dropped) *dropped = 0;
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(pairs, 2 * count));
    const int before = exclusions_.count();
    exclusions_.add(keys);
    if (exclusions_.count() == before || !nm) return PHX_OK;               // nothing new, or no pair exists to drop: the device side follows at the next step
    // the manifolds whose pair is now excluded go, with their slots and joints; the one round trip brings back the kept counts
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before anything moves)
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    PHX_TRY(exclusions_.sync(nb(), stream_));
    PHX_TRY(compaction_scratch());
    const ExclusionKept kept{exclusions_.view()->table, exclusions_.view()->mask};
    PHX_TRY(scan_compaction(kept));
    PHX_TRY(queue_compaction(kept));
    unsigned got[5] = {0, 0, 0, 0, 0};
    PHX_TRY(rb_.add(got, rm_counts_.p, sizeof got, stream_));
    PHX_TRY(rb_.wait(stream_));
    if (dropped) *dropped = nm - (int)got[1];
    if ((int)got[1] == nm) return PHX_OK;                                   // nothing dropped: a true no-op for the topology (the spares are dropped)
    ++contact_epoch_;                                                       // (the touch events' baseline stays: dropped pairs end)
    return adopt_compaction(got);
}

int World::remove_collision_exclusions(const int32_t* pairs, int count)
{
    std::vector<unsigned long long> keys;
    PHX_TRY(check_exclusion_pairs("phx_world_remove_collision_exclusions", pairs, count, &keys));
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(pairs, 2 * count));
    exclusions_.remove(keys);                                               // (no manifold changes: an overlapping pair is new to the next step's UpdatePairs)
    return PHX_OK;
}

int World::clear_collision_exclusions()
{
    static const char* const what = "phx_world_clear_collision_exclusions";
    PHX_TRY(refuse_sharded(what, "collision exclusions"));
    PHX_TRY(refuse_mid_step(what));
    if (exclusions_.empty()) return PHX_OK;
    std::vector<int> named;
    for (const unsigned long long k : exclusions_.keys()) { named.push_back((int)(k >> 32)); named.push_back((int)(unsigned)k); }
    PHX_TRY(wake_named(named.data(), (int)named.size()));
    exclusions_.clear();
    return PHX_OK;
}

int World::get_collision_exclusions(int32_t* out, int cap, int32_t* count) const
{
    const int n = exclusions_.count();
    if (count) *count = n;
    if (cap < n) { set_error("phx_world_get_collision_exclusions: room for %d pairs, the set holds %d", cap, n); return PHX_ERR_CAPACITY; }
    for (int i = 0; i < n; ++i) { const unsigned long long k = exclusions_.keys()[(size_t)i]; out[2 * i] = (int32_t)(k >> 32); out[2 * i + 1] = (int32_t)(unsigned)k; }
    return PHX_OK;
}

int World::refuse_exclusions(const char* what) const
{
    if (exclusions_.empty()) return PHX_OK;
    set_error("%s: the world holds %d collision exclusions, which a sharded world does not carry", what, exclusions_.count());
    return PHX_ERR_STATE;
}

// the two getters: every body's value in the C ABI's form
template <class Column>
int World::get_table(const char* what, BodyTable<Column>& table, typename Column::api* out, int cap)
{
    const int n = nb();
    if (cap < n) { set_error("%s: room for %d bodies, the world has %d", what, cap, n); return PHX_ERR_CAPACITY; }
    return table.visit(n, host_staged(), device_, rb_, stream_, [out](int i, const typename Column::value& v) { out[i] = Column::shown(v); });
}
int World::get_collision_filters(phx_collision_filter* out, int cap) { return get_table("phx_world_get_collision_filters", filters_, out, cap); }
int World::get_materials(phx_material* out, int cap) { return get_table("phx_world_get_materials", materials_, out, cap); }

// the sharded modes (phx_world_set_shard, set_comm, reslab) carry no optional column: refused while some body's value is not the default
int World::refuse_tables(const char* what)
{
    if (sleep_.on()) { set_error("%s: sleeping is enabled, which a sharded world does not carry (phx_world_set_sleeping(w, NULL) first)", what); return PHX_ERR_STATE; }
    return each_table([&](auto& t) -> int {
        using Column = typename std::decay_t<decltype(t)>::column;
        if (!t.active) return PHX_OK;
        bool all_default = true;
        PHX_TRY(t.visit(nb(), host_staged(), device_, rb_, stream_, [&](int, const typename Column::value& v) { all_default &= Column::is_initial(v); }));
        if (!all_default) { set_error("%s: the world holds %s, which a sharded world does not carry", what, Column::plural); return PHX_ERR_STATE; }
        t.reset();                                                          // (every value is the default again: the plain kernels)
        return PHX_OK;
    });
}

// ---- materials --------------------------------------------------------------------------------------------------------------------
// The pair rule and the defaults: include/phyx_amd.h MATERIALS.  The table is read by the solver's material kernels only
// (solver_kernels.h k_pack_refresh_mat and the *_mat sweeps, island_kernel.h k_solve_islands_mat); nothing of the topology depends on it.
int World::set_materials(const int32_t* bodies, const phx_material* materials, int count)
{
    static const char* const what = "phx_world_set_materials";
    return set_column(what, materials_, bodies, materials, count, [=](int k) {      // (NaN fails both comparisons)
        const float f = materials[k].friction, e = materials[k].restitution;
        if (!(f >= 0.f && f <= 1e6f)) { set_error("%s: friction %g of body %d is not in [0, 1e6]", what, (double)f, bodies[k]); return PHX_ERR_INVALID; }
        if (!(e >= 0.f && e <= 1.f)) { set_error("%s: restitution %g of body %d is not in [0, 1]", what, (double)e, bodies[k]); return PHX_ERR_INVALID; }
        return PHX_OK;
    }, true);
}

// ---- body flags / sensors -----------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h BODY FLAGS / SENSORS.  The call writes the column and nothing else; the joint match of the next step
// (world_kernels.h BodySensors) is what takes a sensor manifold's joints away or lets them come back, and sets joints_changed_ when it does.
int World::set_body_flags(const int32_t* bodies, const uint32_t* flags, int count)
{
    static const char* const what = "phx_world_set_body_flags";
    return set_column(what, flags_col_, bodies, flags, count, [=](int k) {
        if (flags[k] & ~(uint32_t)PHX_BODY_SENSOR) { set_error("%s: flags 0x%x of body %d hold an unknown bit", what, flags[k], bodies[k]); return PHX_ERR_INVALID; }
        return PHX_OK;
    }, true);
}
int World::get_body_flags(uint32_t* out, int cap) { return get_table("phx_world_get_body_flags", flags_col_, out, cap); }

// ---- units: pins, links, angles and sliders --------------------------------------------------------------------------------------------------------
// The rules and the arithmetic: include/phyx_amd.h PINS, LINKS, ANGLES, SLIDERS; the lists, the schedule and the pass: pins.h.  One copy of the calls for
// both records (`P`; what differs is UnitKind<P>): they check everything first — inside a step, sharded, count, null, overflow, the
// entries in order — then change the list; the schedule follows lazily at the next step.
int World::refuse_pins(const char* what)
{
    if (!pins_.units()) return PHX_OK;
    const char* plural = nullptr;                                           // the first kind the world holds names the refusal
    pins_.each_list([&](auto& l) { if (!plural && l.count()) plural = UnitKind<typename std::decay_t<decltype(l)>::record>::plural; return PHX_OK; });
    set_error("%s: the world holds %s, which a sharded world does not carry", what, plural);
    return PHX_ERR_STATE;
}

template <class P>
int World::check_unit_indices(const char* what, const int32_t* which, const void* values, int count)
{
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(settle_breaks());
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && (!which || !values)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = pins_.list<P>().count();
    const char* const noun = UnitKind<P>::noun;
    std::vector<unsigned char> seen((size_t)n, 0);
    for (int k = 0; k < count; ++k) {
        if (which[k] < 0 || which[k] >= n) { set_error("%s: %s index %d out of range [0, %d)", what, noun, which[k], n); return PHX_ERR_INVALID; }
        if (seen[(size_t)which[k]]) { set_error("%s: %s %d appears twice in one call", what, noun, which[k]); return PHX_ERR_INVALID; }
        seen[(size_t)which[k]] = 1;
    }
    return PHX_OK;
}

// the body rules of entry k of an add (the record's own: UnitKind<P>::check)
int World::check_unit_bodies(const char* what, const char* noun, int k, int body1, int body2)
{
    const int n = nb();
    if (body1 < 0 || body1 >= n) { set_error("%s: %s %d: body1 %d out of range [0, %d)", what, noun, k, body1, n); return PHX_ERR_INVALID; }
    if (body2 < -1 || body2 >= n) { set_error("%s: %s %d: body2 %d is neither -1 nor in [0, %d)", what, noun, k, body2, n); return PHX_ERR_INVALID; }
    if (body1 == body2) { set_error("%s: %s %d: both ends on body %d", what, noun, k, body1); return PHX_ERR_INVALID; }
    return PHX_OK;
}

template <class P>
int World::add_units(const P* recs, int count, int* first)
{
    using Kind = UnitKind<P>;
    const char* const what = Kind::add;
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, Kind::plural));
    PHX_TRY(settle_breaks());
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && !recs) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    // (the schedule numbers the units, pins, links, angles and sliders together, in an int32)
    if ((long long)pins_.units() + count > (long long)INT32_MAX) { set_error("%s: %d + %d units exceed the int32 range", what, pins_.units(), count); return PHX_ERR_INVALID; }
    for (int k = 0; k < count; ++k) {
        PHX_TRY(check_unit_bodies(what, Kind::noun, k, recs[k].body1, recs[k].body2));
        PHX_TRY(Kind::check(what, k, recs[k]));
    }
    UnitList<P>& list = pins_.list<P>();
    if (first) *first = list.count();
    if (!count) return PHX_OK;
    if (sleep_col_.active) {                                                // (the new units' bodies)
        std::vector<int> named;
        for (int k = 0; k < count; ++k) { named.push_back(recs[k].body1); if (recs[k].body2 >= 0) named.push_back(recs[k].body2); }
        PHX_TRY(wake_named(named.data(), (int)named.size()));
    }
    PHX_TRY(settle_on_device());
    pins_.units_changed();
    return list.add(recs, count, stream_);
}

template <class P>
int World::remove_units(const int32_t* which, int count)
{
    PHX_TRY(check_unit_indices<P>(UnitKind<P>::remove, which, which, count));
    if (!count) return PHX_OK;
    PHX_TRY(wake_units<P>(which, count));
    PHX_TRY(settle_on_device());
    pins_.units_changed();
    return pins_.list<P>().remove(which, count, stream_);
}

template <class P, class Fields>
int World::set_unit_fields(const int32_t* which, const float* values, int count)
{
    if (!count) return PHX_OK;
    PHX_TRY(wake_units<P>(which, count));
    UnitList<P>& list = pins_.list<P>();
    const int* d_which = nullptr; const float* d_values = nullptr;
    if (list.on_device()) {
        PHX_TRY(settle_on_device());
        PHX_TRY(stage_batch(which, values, count, Fields::width, &d_which, &d_values));
    }
    return list.template set_fields<Fields>(which, values, count, d_which, d_values, stream_);
}

template <class P>
int World::set_unit_anchors(const int32_t* which, const float* anchors, int count)
{
    const char* const what = UnitKind<P>::set_anchors;
    PHX_TRY(check_unit_indices<P>(what, which, anchors, count));
    for (int k = 0; k < 4 * count; ++k)
        if (!std::isfinite(anchors[k])) { set_error("%s: entry %d: value %d is not finite", what, k / 4, k % 4); return PHX_ERR_INVALID; }
    return set_unit_fields<P, AnchorFields>(which, anchors, count);
}

int World::set_link_lengths(const int32_t* which, const float* lengths, int count)
{
    static const char* const what = "phx_world_set_link_lengths";
    PHX_TRY(check_unit_indices<phx_link>(what, which, lengths, count));
    const std::vector<phx_link>& links = pins_.list<phx_link>().host();     // (bodies, anchors, lengths, hertz: always current)
    for (int k = 0; k < count; ++k)
        PHX_TRY(UnitKind<phx_link>::check_lengths(what, k, lengths[2 * k], lengths[2 * k + 1], links[(size_t)which[k]].hertz));
    return set_unit_fields<phx_link, LengthFields>(which, lengths, count);
}

template <class P>
int World::set_unit_limits(const int32_t* which, const float* limits, int count)
{
    const char* const what = UnitKind<P>::set_limits;
    PHX_TRY(check_unit_indices<P>(what, which, limits, count));
    const std::vector<P>& units = pins_.list<P>().host();                   // (bodies, limits, hertz, motor: always current)
    for (int k = 0; k < count; ++k)
        PHX_TRY(check_limits<P>(what, k, limits[2 * k], limits[2 * k + 1], units[(size_t)which[k]].hertz));
    return set_unit_fields<P, LimitFields>(which, limits, count);
}

template <class P>
int World::set_unit_motors(const int32_t* which, const float* motors, int count)
{
    const char* const what = UnitKind<P>::set_motors;
    PHX_TRY(check_unit_indices<P>(what, which, motors, count));
    for (int k = 0; k < count; ++k) PHX_TRY(check_motor<P>(what, k, motors[2 * k], motors[2 * k + 1]));
    return set_unit_fields<P, MotorFields>(which, motors, count);
}

template <class P>
int World::get_units(P* out, int cap)
{
    PHX_TRY(settle_breaks());
    UnitList<P>& list = pins_.list<P>();
    const int n = list.count();
    if (cap < n) { set_error("%s: room for %d %s, the world has %d", UnitKind<P>::get, cap, UnitKind<P>::plural, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    return list.get(out, stream_);
}

template <class P>
int World::unit_count(int* out)
{
    PHX_TRY(settle_breaks());
    *out = pins_.list<P>().count();
    return PHX_OK;
}

// ---- breaks ---------------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h BREAKS; the test runs behind the pass (PinSet::solve) and is settled here, lazily.
int World::settle_breaks()
{
    if (mid_step_ || !pins_.breaks_pending()) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    return pins_.settle(rb_, stream_);
}

// f(a P*) for the record of `kind`
template <class F> static int with_kind(const char* what, int kind, F f)
{
    switch (kind) {
    case PHX_UNIT_PIN: return f((phx_pin*)nullptr);
    case PHX_UNIT_LINK: return f((phx_link*)nullptr);
    case PHX_UNIT_ANGLE: return f((phx_angle*)nullptr);
    case PHX_UNIT_SLIDER: return f((phx_slider*)nullptr);
    }
    set_error("%s: kind %d is none of PHX_UNIT_PIN ... PHX_UNIT_SLIDER [0, 3]", what, kind);
    return PHX_ERR_INVALID;
}

int World::set_break_limits(int kind, const int32_t* which, const float* limits, int count)
{
    static const char* const what = "phx_world_set_break_limits";
    PHX_TRY(refuse_mid_step(what));
    return with_kind(what, kind, [&](auto* tag) -> int {
        using P = std::remove_pointer_t<decltype(tag)>;
        PHX_TRY(check_unit_indices<P>(what, which, limits, count));
        for (int k = 0; k < count; ++k)
            if (!(limits[k] > 0.f)) { set_error("%s: %s %d: break limit %g is not > 0", what, UnitKind<P>::noun, k, (double)limits[k]); return PHX_ERR_INVALID; }
        if (!count) return PHX_OK;
        PHX_TRY(wake_units<P>(which, count));
        UnitList<P>& list = pins_.list<P>();
        const int* d_which = nullptr; const float* d_values = nullptr;
        if (list.on_device()) {
            PHX_TRY(settle_on_device());
            if (list.limited()) PHX_TRY(stage_batch(which, limits, count, 1, &d_which, &d_values));
        }
        return list.set_limits(which, limits, count, d_which, d_values, stream_);
    });
}

int World::get_break_limits(int kind, float* out, int cap)
{
    static const char* const what = "phx_world_get_break_limits";
    PHX_TRY(refuse_mid_step(what));
    return with_kind(what, kind, [&](auto* tag) -> int {
        using P = std::remove_pointer_t<decltype(tag)>;
        PHX_TRY(settle_breaks());
        const UnitList<P>& list = pins_.list<P>();
        if (cap < list.count()) { set_error("%s: room for %d %s, the world has %d", what, cap, UnitKind<P>::plural, list.count()); return PHX_ERR_CAPACITY; }
        list.get_limits(out);
        return PHX_OK;
    });
}

int World::break_events(phx_break_event* out, int cap, int64_t* total)
{
    static const char* const what = "phx_world_break_events";
    PHX_TRY(refuse_mid_step(what));
    if (cap < 0) { set_error("%s: negative cap %d", what, cap); return PHX_ERR_INVALID; }
    PHX_TRY(settle_breaks());
    std::vector<phx_break_event>& queue = pins_.break_queue();
    *total = (int64_t)queue.size();
    if ((int64_t)cap < *total) { set_error("%s: room for %d events, the queue holds %lld", what, cap, (long long)*total); return PHX_ERR_CAPACITY; }
    std::copy(queue.begin(), queue.end(), out);
    queue.clear();
    break_step_ = 0;
    return PHX_OK;
}

int World::set_pin_iterations(int n)
{
    PHX_TRY(refuse_mid_step("phx_world_set_pin_iterations"));
    if (n < 1 || n > PIN_MAX_ITERATIONS) { set_error("phx_world_set_pin_iterations: %d is not in [1, %d]", n, PIN_MAX_ITERATIONS); return PHX_ERR_INVALID; }
    pins_.iterations = n;
    return PHX_OK;
}

int World::pin_schedule(const Schedule** out)
{
    PHX_TRY(refuse_mid_step("phx_world_get_pin_schedule"));
    *out = nullptr;
    PHX_TRY(settle_breaks());
    if (!pins_.units()) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    PHX_TRY(settle_sleep_count());                                          // (bodies the last pass put to sleep or woke are part of the static set)
    PHX_TRY(pins_.prepare(bodies_.mpos.p, nb(), rb_, stream_));
    *out = &pins_.schedule();
    return PHX_OK;
}

// ---- sleeping ---------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h SLEEPING, tests/sleep_spec.py; the column, the pass and the wake by list: sleep.h.  Here: the calls, the
// place of the pass in the step, and how the host learns that the static set changed — the device counts the bodies the pass (or a wake)
// put to sleep or woke, and the next step's joint-count readback brings the count along (refresh_contact_joints), in front of the
// solve and of the pin pass, which are what consult the static set.
SleepGraph World::sleep_graph()
{
    SleepGraph g = {};
    g.manifolds = d_manifolds_.p; g.nm = nm; g.flags = flags_col_.ptr();
    int kind = 0;
    pins_.each_list([&](auto& l) {
        using P = typename std::decay_t<decltype(l)>::record;
        static_assert(offsetof(P, body1) == 0 && offsetof(P, body2) == 4, "a unit's record begins with its bodies");
        g.units[kind++] = SleepGraph::List{reinterpret_cast<const char*>(l.device()), (int)sizeof(P), l.count()};
        return PHX_OK;
    });
    return g;
}

int World::sleep_pass(float dt)
{
    if (!nb()) return PHX_OK;
    if (pins_.units()) PHX_TRY(pins_.upload(stream_));                      // (current already behind a pin pass: nothing is copied)
    PHX_TRY(sleep_.pass(resident(), bodies_.records.p, sleep_col_.dev.p, nb(), sleep_graph(), dt, stream_));
    sleep_count_pending_ = true;
    return PHX_OK;
}

void World::take_sleep_count(unsigned changed)
{
    sleep_count_pending_ = false;
    if (!changed) return;
    joints_changed_ = true;                                                 // which bodies are static is part of the schedule's topology
    pins_.statics_changed();
}

int World::settle_sleep_count()
{
    if (!sleep_count_pending_) return PHX_OK;
    unsigned changed = 0;
    PHX_TRY(rb_.add(&changed, sleep_.words() + SLEEP_CHANGED, sizeof changed, stream_));
    PHX_TRY(rb_.wait(stream_));
    take_sleep_count(changed);
    return PHX_OK;
}

int World::wake_named(const int* bodies, int count, const unsigned* d_keep, bool all)
{
    if (!sleep_col_.active || !nb() || (!all && !d_keep && !count)) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before masses change)
    PHX_TRY(settle_breaks());                                               // (a unit that broke in the last step is no edge any more)
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies and the column go up as the next step would take them)
    if (pins_.units()) PHX_TRY(pins_.upload(stream_));
    const int* d_list = nullptr; const float* unused = nullptr;
    if (!all && !d_keep) PHX_TRY(stage_batch(bodies, nullptr, count, 0, &d_list, &unused));
    PHX_TRY(sleep_.wake(resident(), bodies_.records.p, sleep_col_.dev.p, nb(), sleep_graph(), d_list, count, d_keep, all, stream_));
    sleep_count_pending_ = true;
    return PHX_OK;
}

template <class P>
int World::wake_units(const int32_t* which, int count)
{
    if (!sleep_col_.active || !count) return PHX_OK;
    const std::vector<P>& units = pins_.list<P>().host();                   // (the bodies: always current)
    std::vector<int> named;
    for (int k = 0; k < count; ++k) {
        const P& u = units[(size_t)which[k]];
        named.push_back(u.body1);
        if (u.body2 >= 0) named.push_back(u.body2);
    }
    return wake_named(named.data(), (int)named.size());
}

int World::set_sleeping(const phx_sleep_params* p)
{
    static const char* const what = "phx_world_set_sleeping";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, SleepColumn::plural));
    if (!p) {
        if (!sleep_.on()) return PHX_OK;
        PHX_TRY(wake_named(nullptr, 0, nullptr, true));                     // every mass is its own again, byte for byte
        sleep_.disable();
        sleep_col_.reset();
        return PHX_OK;
    }
    const float v[3] = {p->linear_tolerance, p->angular_tolerance, p->time_to_sleep};
    static const char* const names[3] = {"linear_tolerance", "angular_tolerance", "time_to_sleep"};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(v[k]) || !(v[k] >= 0.f)) { set_error("%s: %s %g must be finite and >= 0", what, names[k], (double)v[k]); return PHX_ERR_INVALID; }
    PHX_TRY(use_device(device_));
    if (!sleep_col_.active) {                                               // the column: every body awake, timer 0
        if (host_staged()) sleep_col_.host.assign((size_t)nb(), SleepColumn::initial());
        else {
            PHX_TRY(settle_on_device());
            PHX_TRY(sleep_col_.dev.reserve((size_t)std::max(nb(), 1)));
            PHX_TRY(sleep_.fill(sleep_col_.dev.p, nb(), stream_));
        }
        sleep_col_.active = true;
    }
    return sleep_.enable(*p, stream_);
}

int World::get_sleeping(phx_sleep_params* out, int32_t* enabled) const
{
    if (out) *out = sleep_.params();
    if (enabled) *enabled = sleep_.on() ? 1 : 0;
    return PHX_OK;
}

int World::get_sleep_states(phx_sleep_state* out, int cap)
{
    static const char* const what = "phx_world_get_sleep_states";
    PHX_TRY(refuse_mid_step(what));
    const int n = nb();
    if (cap < n) { set_error("%s: room for %d bodies, the world has %d", what, cap, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    PHX_TRY(sleep_out_.reserve((size_t)n));
    PHX_TRY(sleep_.states(bodies_.mpos.p, sleep_col_.ptr(), n, sleep_out_.p, stream_));
    PHX_TRY(rb_.add(out, sleep_out_.p, (size_t)n * sizeof(phx_sleep_state), stream_));
    return rb_.wait(stream_);
}

int World::wake_bodies(const int32_t* bodies, int count)
{
    static const char* const what = "phx_world_wake_bodies";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, SleepColumn::plural));
    PHX_TRY(check_batch(what, bodies, bodies, count, false));              // (no values: the indices stand in for them; a body may be named twice)
    return wake_named(bodies, count);
}

int World::sleep_counts(int32_t* asleep, int64_t* slept_total, int64_t* woken_total)
{
    PHX_TRY(refuse_mid_step("phx_world_sleep_counts"));
    unsigned long long totals[2] = {0, 0};
    if (sleep_.words()) {
        PHX_TRY(use_device(device_));
        PHX_TRY(solver_.synchronize());
        PHX_TRY(rb_.add(totals, sleep_.words() + SLEEP_SLEPT, sizeof totals, stream_));
        PHX_TRY(rb_.wait(stream_));
    }
    if (asleep) *asleep = (int32_t)(totals[0] - totals[1]);
    if (slept_total) *slept_total = (int64_t)totals[0];
    if (woken_total) *woken_total = (int64_t)totals[1];
    return PHX_OK;
}

int World::set_gravity(float g)
{
    if (sleep_.on()) {                                                      // a change of gravity disturbs every pile
        PHX_TRY(refuse_mid_step("phx_world_set_gravity"));
        PHX_TRY(wake_named(nullptr, 0, nullptr, true));
    }
    gravity = g;
    return PHX_OK;
}

// ---- force fields ---------------------------------------------------------------------------------------------------------------------
// The rules and the arithmetic: include/phyx_amd.h FORCE FIELDS; the list, its device copy and the launches: fields.h.  The world's part
// is the seam: the pass fills accel_, the dense pending accelerations the unchanged IntegrateVelocity consumes (fused into the
// broadphase's first kernel or on its own under phase timing), so no kernel of the step knows about fields.
int World::refuse_fields(const char* what) const
{
    if (!fields_.count()) return PHX_OK;
    set_error("%s: the world holds force fields, which a sharded world does not carry (phx_world_set_fields(w, NULL, 0) first)", what);
    return PHX_ERR_STATE;
}

int World::set_fields(const phx_field* fields, int count)
{
    static const char* const what = "phx_world_set_fields";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, "force fields"));
    PHX_TRY(phx_field_check(fields, count));
    const int* unused = nullptr; const float* d_fields = nullptr;
    if (count) {
        PHX_TRY(use_device(device_));
        PHX_TRY(stage_batch(nullptr, reinterpret_cast<const float*>(fields), count, (int)(sizeof(phx_field) / sizeof(float)), &unused, &d_fields));
    }
    return fields_.set(fields, count, reinterpret_cast<const phx_field*>(d_fields), stream_);
}

int World::get_fields(phx_field* out, int cap, int32_t* count) const
{
    const int n = fields_.count();
    if (count) *count = n;
    if (cap < n || (n && !out)) { set_error("phx_world_get_fields: room for %d fields, the world has %d", out ? cap : 0, n); return PHX_ERR_CAPACITY; }
    if (n) std::memcpy(out, fields_.list().data(), (size_t)n * sizeof(phx_field));
    return PHX_OK;
}

int World::field_pass(float dt)
{
    accel_from_fields_ = false;
    if (!fields_.count() || !nb()) return PHX_OK;
    // (pending accelerations fill accel_ for every body already; otherwise the kernel starts every slot from zero itself)
    if (!accel_pending_) PHX_TRY(accel_.reserve((size_t)nb()));
    PHX_TRY(fields_.apply(field_bodies(), accel_.p, accel_pending_, dt, stream_));
    accel_from_fields_ = !accel_pending_;
    accel_pending_ = true;
    return PHX_OK;
}

int World::pulse_fields(const phx_field* fields, int count)
{
    static const char* const what = "phx_world_pulse_fields";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, "force fields"));
    PHX_TRY(phx_field_check(fields, count));
    if (!count || !nb()) return PHX_OK;
    PHX_TRY(settle_on_device());
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    const int* unused = nullptr; const float* d_fields = nullptr;
    PHX_TRY(stage_batch(nullptr, reinterpret_cast<const float*>(fields), count, (int)(sizeof(phx_field) / sizeof(float)), &unused, &d_fields));
    records_stale_ = true;
    return DeviceFields::pulse(field_bodies(), reinterpret_cast<const phx_field*>(d_fields), count, field_traits(fields, count), stream_);
}

int World::apply_impulses(const int* bodies, const float* impulses, int count)
{
    static const char* const what = "phx_world_apply_impulses";
    PHX_TRY(check_batch(what, bodies, impulses, count, true));
    for (int k = 0; k < 4 * count; ++k)
        if (!std::isfinite(impulses[k])) { set_error("%s: entry %d: value %d is not finite", what, k / 4, k % 4); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(bodies, count));
    if (host_staged()) {                                    // the host-staged records are the world: the kernel's statements on them
        for (int k = 0; k < count; ++k) {
            phx_rigid_body& b = host_bodies_[(size_t)bodies[k]];
            if (!(b.inv_mass > 0.0f)) continue;
            const float* q = impulses + 4 * (size_t)k;
            const float rx = q[2] - b.pos.x, ry = q[3] - b.pos.y;
            b.velocity.x = b.velocity.x + b.inv_mass * q[0]; b.velocity.y = b.velocity.y + b.inv_mass * q[1];
            b.angular_velocity = b.angular_velocity - b.inv_inertia * (rx * q[1] - ry * q[0]);
        }
        return PHX_OK;
    }
    PHX_TRY(settle_on_device());
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_batch(bodies, impulses, count, 4, &d_bodies, &d_values));
    records_stale_ = true;
    return DeviceFields::impulses(field_bodies(), d_bodies, d_values, count, stream_);
}

// ---- queries ------------------------------------------------------------------------------------------------------------------------
// Answered on the world's stream from the resident arrays (query.h / query_kernels.h).  The host forms check everything first, stage the
// queries through the world's pinned staging and wait for their results; the device forms only queue.  Nothing of the world changes:
// the upload of host-staged bodies is the one the next step would make.
static int query_check(const char* what, const float* v, int count, int width, int flags, bool device, const void* out)
{
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (flags != 0 && flags != PHX_QUERY_SKIP_STATIC) { set_error("%s: flags %d (0 or PHX_QUERY_SKIP_STATIC)", what, flags); return PHX_ERR_INVALID; }
    if (count && (!v || !out)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    if (device) return PHX_OK;
    for (int k = 0; k < count; ++k) {
        const float* q = v + (size_t)width * k;
        for (int c = 0; c < width; ++c)
            if (!std::isfinite(q[c])) { set_error("%s: query %d: value %d is not finite", what, k, c); return PHX_ERR_INVALID; }
        if (width == 4 && !(q[0] <= q[2] && q[1] <= q[3])) { set_error("%s: box %d: min exceeds max", what, k); return PHX_ERR_INVALID; }
        if (width == 5 && !(q[4] >= 0.f)) { set_error("%s: ray %d: max_t < 0", what, k); return PHX_ERR_INVALID; }
        if (width == 5 && q[2] == 0.f && q[3] == 0.f) { set_error("%s: ray %d: zero direction", what, k); return PHX_ERR_INVALID; }
        if (width >= 8 && !(q[6] > 0.f && q[7] > 0.f)) { set_error("%s: box %d: half extents must be positive", what, k); return PHX_ERR_INVALID; }
        if (width == 11 && !(q[10] >= 0.f)) { set_error("%s: cast %d: max_t < 0", what, k); return PHX_ERR_INVALID; }
        if (width == 11 && q[8] == 0.f && q[9] == 0.f) { set_error("%s: cast %d: zero direction", what, k); return PHX_ERR_INVALID; }
    }
    return PHX_OK;
}

int World::query_prepare(bool host_wait)
{
    PHX_TRY(use_device(device_));
    if (host_wait || solver_.has_pending()) PHX_TRY(solver_.synchronize());      // (an unverified solve is settled before its results are read)
    return sync_bodies_to_device();                                         // (host-staged bodies go up as the next step would take them)
}

int World::query_aabb(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total)
{
    static const char* const what = "phx_world_query_aabb";
    PHX_TRY(query_check(what, boxes, count, 4, flags, false, boxes));
    if (!offsets || !total) { set_error("%s: null offsets / total", what); return PHX_ERR_INVALID; }
    if (hit_cap < 0 || (hit_cap > 0 && !hits)) { set_error("%s: bad hits buffer (cap %d)", what, hit_cap); return PHX_ERR_INVALID; }
    PHX_TRY(query_prepare(true));
    const float* d_boxes = nullptr;
    if (count && nb()) { const int* unused = nullptr; PHX_TRY(stage_batch(nullptr, boxes, count, 4, &unused, &d_boxes)); }
    return query_.aabb(query_view(), nb(), geom_epoch_, d_boxes, count, flags, offsets, hits, hit_cap, total, rb_, stream_);
}

int World::query_points(const float* points, int count, int flags, int32_t* body)
{
    static const char* const what = "phx_world_query_points";
    PHX_TRY(query_check(what, points, count, 2, flags, false, body));
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(true));
    if (!nb()) { for (int k = 0; k < count; ++k) body[k] = -1; return PHX_OK; }
    const int* unused = nullptr; const float* d_points = nullptr;
    PHX_TRY(stage_batch(nullptr, points, count, 2, &unused, &d_points));
    PHX_TRY(q_body_.reserve((size_t)count));
    PHX_TRY(query_.points(query_view(), nb(), geom_epoch_, d_points, count, flags, q_body_.p, stream_));
    PHX_TRY(rb_.add(body, q_body_.p, (size_t)count * sizeof(int), stream_));
    return rb_.wait(stream_);
}

int World::raycast(const float* rays, int count, int flags, phx_ray_hit* out)
{
    static const char* const what = "phx_world_raycast";
    PHX_TRY(query_check(what, rays, count, 5, flags, false, out));
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(true));
    if (!nb()) { std::memset(out, 0, (size_t)count * sizeof(phx_ray_hit)); for (int k = 0; k < count; ++k) out[k].body = -1; return PHX_OK; }
    const int* unused = nullptr; const float* d_rays = nullptr;
    PHX_TRY(stage_batch(nullptr, rays, count, 5, &unused, &d_rays));
    PHX_TRY(q_hits_.reserve((size_t)count));
    PHX_TRY(query_.rays(query_view(), nb(), geom_epoch_, d_rays, count, flags, q_hits_.p, stream_));
    PHX_TRY(rb_.add(out, q_hits_.p, (size_t)count * sizeof(phx_ray_hit), stream_));
    return rb_.wait(stream_);
}

int World::query_points_device(const void* d_points, int count, int flags, void* d_body)
{
    static const char* const what = "phx_world_query_points_device";
    PHX_TRY(query_check(what, static_cast<const float*>(d_points), count, 2, flags, true, d_body));
    if (count && ((reinterpret_cast<uintptr_t>(d_points) | reinterpret_cast<uintptr_t>(d_body)) & 3u)) { set_error("%s: the arrays must be 4-byte aligned", what); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(false));
    return query_.points(query_view(), nb(), geom_epoch_, static_cast<const float*>(d_points), count, flags, static_cast<int*>(d_body), stream_);
}

int World::raycast_device(const void* d_rays, int count, int flags, void* d_out)
{
    static const char* const what = "phx_world_raycast_device";
    PHX_TRY(query_check(what, static_cast<const float*>(d_rays), count, 5, flags, true, d_out));
    if (count && ((reinterpret_cast<uintptr_t>(d_rays) | reinterpret_cast<uintptr_t>(d_out)) & 3u)) { set_error("%s: the arrays must be 4-byte aligned", what); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(false));
    return query_.rays(query_view(), nb(), geom_epoch_, static_cast<const float*>(d_rays), count, flags, static_cast<phx_ray_hit*>(d_out), stream_);
}

int World::query_boxes(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total)
{
    static const char* const what = "phx_world_query_boxes";
    PHX_TRY(query_check(what, boxes, count, 8, flags, false, boxes));
    if (!offsets || !total) { set_error("%s: null offsets / total", what); return PHX_ERR_INVALID; }
    if (hit_cap < 0 || (hit_cap > 0 && !hits)) { set_error("%s: bad hits buffer (cap %d)", what, hit_cap); return PHX_ERR_INVALID; }
    PHX_TRY(query_prepare(true));
    const float* d_boxes = nullptr;
    if (count && nb()) { const int* unused = nullptr; PHX_TRY(stage_batch(nullptr, boxes, count, 8, &unused, &d_boxes)); }
    return query_.shapes(query_view(), nb(), geom_epoch_, d_boxes, count, flags, offsets, hits, hit_cap, total, rb_, stream_);
}

int World::cast_boxes(const float* casts, int count, int flags, phx_shape_hit* out)
{
    static const char* const what = "phx_world_cast_boxes";
    PHX_TRY(query_check(what, casts, count, 11, flags, false, out));
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(true));
    if (!nb()) { std::memset(out, 0, (size_t)count * sizeof(phx_shape_hit)); for (int k = 0; k < count; ++k) out[k].body = -1; return PHX_OK; }
    const int* unused = nullptr; const float* d_casts = nullptr;
    PHX_TRY(stage_batch(nullptr, casts, count, 11, &unused, &d_casts));
    PHX_TRY(q_shape_hits_.reserve((size_t)count));
    PHX_TRY(query_.casts(query_view(), nb(), geom_epoch_, d_casts, count, flags, q_shape_hits_.p, stream_));
    PHX_TRY(rb_.add(out, q_shape_hits_.p, (size_t)count * sizeof(phx_shape_hit), stream_));
    return rb_.wait(stream_);
}

int World::cast_boxes_device(const void* d_casts, int count, int flags, void* d_out)
{
    static const char* const what = "phx_world_cast_boxes_device";
    PHX_TRY(query_check(what, static_cast<const float*>(d_casts), count, 11, flags, true, d_out));
    if (count && ((reinterpret_cast<uintptr_t>(d_casts) | reinterpret_cast<uintptr_t>(d_out)) & 3u)) { set_error("%s: the arrays must be 4-byte aligned", what); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(false));
    return query_.casts(query_view(), nb(), geom_epoch_, static_cast<const float*>(d_casts), count, flags, static_cast<phx_shape_hit*>(d_out), stream_);
}

int World::query_index_build()
{
    PHX_TRY(query_prepare(false));
    return query_.ensure_index(query_view(), nb(), geom_epoch_, stream_);
}

// ---- contact reports ----------------------------------------------------------------------------------------------------------------
// Answered on the world's stream from the resident contact cache (contact.h / contact_kernels.h), between steps only: inside a step the
// manifolds are mid-update.  The host forms check everything first and wait for their results; the markers only queue.
int World::contact_prepare(const char* what, bool host_wait)
{
    PHX_TRY(refuse_mid_step(what));
    return query_prepare(host_wait);
}

int World::query_contacts(const int32_t* bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap, int64_t* total)
{
    static const char* const what = "phx_world_query_contacts";
    PHX_TRY(refuse_mid_step(what));
    if (flags != 0 && flags != PHX_QUERY_SKIP_STATIC) { set_error("%s: flags %d (0 or PHX_QUERY_SKIP_STATIC)", what, flags); return PHX_ERR_INVALID; }
    if (!offsets || !total) { set_error("%s: null offsets / total", what); return PHX_ERR_INVALID; }
    if (cap < 0 || (cap > 0 && !out)) { set_error("%s: bad output buffer (cap %d)", what, cap); return PHX_ERR_INVALID; }
    PHX_TRY(check_batch(what, bodies, bodies, count, false));               // (count >= 0, indices in range; repeats allowed)
    PHX_TRY(contact_prepare(what, true));
    const int* d_bodies = nullptr;
    if (count && nm) { const float* unused = nullptr; PHX_TRY(stage_batch(bodies, nullptr, count, 0, &d_bodies, &unused)); }
    return contacts_.contacts(contact_cache(), contact_epoch_, d_bodies, count, flags, offsets, out, cap, total, rb_, stream_);
}

int World::contact_events(int32_t* begin, int begin_cap, int64_t* begin_total, int32_t* end, int end_cap, int64_t* end_total)
{
    static const char* const what = "phx_world_contact_events";
    PHX_TRY(refuse_mid_step(what));
    if (shard_count > 1 || comm_) { set_error("%s: a sharded world has no touch events (a re-slab renumbers bodies)", what); return PHX_ERR_STATE; }
    if (!begin_total || !end_total) { set_error("%s: null totals", what); return PHX_ERR_INVALID; }
    if (begin_cap < 0 || end_cap < 0 || (begin_cap > 0 && !begin) || (end_cap > 0 && !end)) {
        set_error("%s: bad output buffers (caps %d, %d)", what, begin_cap, end_cap);
        return PHX_ERR_INVALID;
    }
    PHX_TRY(contact_prepare(what, true));
    return contacts_.events(contact_cache(), begin, begin_cap, begin_total, end, end_cap, end_total, rb_, stream_);
}

int World::contact_markers_device(void* d_out, int cap)
{
    static const char* const what = "phx_world_get_contact_markers_device";
    PHX_TRY(refuse_mid_step(what));
    if (cap < 0) { set_error("%s: negative cap %d", what, cap); return PHX_ERR_INVALID; }
    if (cap > 0 && (!d_out || (reinterpret_cast<uintptr_t>(d_out) & 7u))) { set_error("%s: the output must be an 8-byte aligned device pointer", what); return PHX_ERR_INVALID; }
    if ((long long)cap < 2ll * nm) { set_error("%s: room for %d markers, the world has %d contact-point slots", what, cap, 2 * nm); return PHX_ERR_CAPACITY; }
    PHX_TRY(contact_prepare(what, false));
    return contacts_.markers(contact_cache(), static_cast<phx_contact_marker*>(d_out), stream_);
}

int World::contact_index_build()
{
    PHX_TRY(contact_prepare("phx_world_contact_index", false));
    return contacts_.ensure_index(contact_cache(), contact_epoch_, stream_);
}

} // namespace phx

// ---- C ABI ------------------------------------------------------------------------------------------------
struct phx_world {
    phx::World impl;
    explicit phx_world(int d) : impl(d) {}
};

extern "C" {

int phx_world_create(phx_world** out, int device)
{
    PHX_REQUIRE(out, "null out");
    *out = nullptr;
    PHX_TRY(phx::use_device(device));
    phx_world* w = new (std::nothrow) phx_world(device);
    PHX_REQUIRE(w, "out of host memory");
    int st = w->impl.init();
    if (st != PHX_OK) { delete w; return st; }
    *out = w;
    return PHX_OK;
}

void phx_world_destroy(phx_world* w) { delete w; }

int phx_world_add_body(phx_world* w, float px, float py, float angle, float hx, float hy)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(hx > 0.f && hy > 0.f, "half sizes must be positive");
    return w->impl.add_body(px, py, angle, hx, hy);
}

int phx_world_set_body_static(phx_world* w, int32_t body)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(body >= 0 && body < w->impl.nb(), "body index out of range");
    return w->impl.set_static(body);
}

int phx_world_set_body_inverse_mass(phx_world* w, int32_t body, float inv_mass, float inv_inertia)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(body >= 0 && body < w->impl.nb(), "body index out of range");
    PHX_REQUIRE(inv_mass >= 0.f && inv_inertia >= 0.f, "inverse mass / inertia must not be negative");
    return w->impl.set_inverse_mass(body, inv_mass, inv_inertia);
}

int phx_world_set_gravity(phx_world* w, float g) { PHX_REQUIRE(w, "null handle"); return w->impl.set_gravity(g); }

int phx_world_set_shard(phx_world* w, int32_t shard, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(count >= 1 && shard >= 0 && shard < count, "bad shard");
    if (count > 1) PHX_TRY(w->impl.refuse_pins("phx_world_set_shard"));
    if (count > 1) PHX_TRY(w->impl.refuse_tables("phx_world_set_shard"));
    if (count > 1) PHX_TRY(w->impl.refuse_fields("phx_world_set_shard"));
    if (count > 1) PHX_TRY(w->impl.refuse_exclusions("phx_world_set_shard"));
    w->impl.shard = shard; w->impl.shard_count = count;
    PHX_TRY(w->impl.solver().set_shard(shard, count));
    return PHX_OK;
}

int phx_world_update(phx_world* w, float dt, const phx_config* cfg)
{
    PHX_REQUIRE(w && cfg, "null handle / config");
    return w->impl.update(dt, *cfg);
}

int phx_world_pre_solve(phx_world* w, float dt)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.pre_solve(dt);
}

int phx_world_finish_step(phx_world* w, float dt, const phx_config* cfg)
{
    PHX_REQUIRE(w && cfg, "null handle / config");
    return w->impl.finish_step(dt, *cfg);
}

int phx_world_step_begin(phx_world* w, float dt, const phx_config* cfg, size_t* segment_bytes)
{
    PHX_REQUIRE(w && cfg, "null handle / config");
    return w->impl.step_begin(dt, *cfg, segment_bytes);
}

int phx_world_step_end(phx_world* w, float dt)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.step_end(dt);
}

void* phx_world_stream(phx_world* w) { return w ? (void*)w->impl.stream() : nullptr; }

int phx_world_set_comm(phx_world* w, phx_comm* c)
{
    PHX_REQUIRE(w, "null handle");
    if (c) PHX_TRY(w->impl.refuse_pins("phx_world_set_comm"));
    if (c) PHX_TRY(w->impl.refuse_tables("phx_world_set_comm"));
    if (c) PHX_TRY(w->impl.refuse_fields("phx_world_set_comm"));
    if (c) PHX_TRY(w->impl.refuse_exclusions("phx_world_set_comm"));
    return w->impl.set_comm(c ? &c->impl : nullptr);
}

int phx_world_step_sharded(phx_world* w, float dt, const phx_config* cfg)
{
    PHX_REQUIRE(w && cfg, "null handle / config");
    return w->impl.step_sharded(dt, *cfg);
}

int phx_world_check_exchange(phx_world* w)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.check_exchange();
}

int phx_world_counts(phx_world* w, int32_t* nb, int32_t* nm, int32_t* ncp, int32_t* nj)
{
    PHX_REQUIRE(w, "null handle");
    if (nb) *nb = w->impl.nb();
    if (nm) *nm = w->impl.nm;
    if (ncp) *ncp = 2 * w->impl.nm;
    if (nj) *nj = w->impl.nj;
    return PHX_OK;
}

int phx_world_get_bodies(phx_world* w, phx_rigid_body* out, int32_t cap) { PHX_REQUIRE(w && out, "null handle / buffer"); return w->impl.download_bodies(out, cap); }
int phx_world_get_manifolds(phx_world* w, phx_manifold* out, int32_t cap) { PHX_REQUIRE(w && out, "null handle / buffer"); return w->impl.download_manifolds(out, cap); }
int phx_world_get_contact_points(phx_world* w, phx_contact_point* out, int32_t cap) { PHX_REQUIRE(w && out, "null handle / buffer"); return w->impl.download_contact_points(out, cap); }
int phx_world_get_joints(phx_world* w, phx_contact_joint* out, int32_t cap) { PHX_REQUIRE(w && out, "null handle / buffer"); return w->impl.download_joints(out, cap); }

int phx_world_add_accelerations(phx_world* w, const int32_t* bodies, const float* accel, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.edit(phx::World::EDIT_ACCELERATIONS, bodies, accel, count);
}

int phx_world_set_velocities(phx_world* w, const int32_t* bodies, const float* vel, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.edit(phx::World::EDIT_VELOCITIES, bodies, vel, count);
}

int phx_world_set_poses(phx_world* w, const int32_t* bodies, const float* pose, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.edit(phx::World::EDIT_POSES, bodies, pose, count);
}

int phx_world_set_fields(phx_world* w, const phx_field* fields, int32_t count) { PHX_REQUIRE(w, "null handle"); return w->impl.set_fields(fields, count); }
int phx_world_get_fields(phx_world* w, phx_field* out, int32_t cap, int32_t* count) { PHX_REQUIRE(w, "null handle"); return w->impl.get_fields(out, cap, count); }
int phx_world_pulse_fields(phx_world* w, const phx_field* fields, int32_t count) { PHX_REQUIRE(w, "null handle"); return w->impl.pulse_fields(fields, count); }
int phx_world_apply_impulses(phx_world* w, const int32_t* bodies, const float* impulses, int32_t count) { PHX_REQUIRE(w, "null handle"); return w->impl.apply_impulses(bodies, impulses, count); }
int phx_world_field_passes(phx_world* w, int64_t* passes) { PHX_REQUIRE(w && passes, "null handle / output"); *passes = w->impl.field_passes(); return PHX_OK; }

int phx_world_get_body_states(phx_world* w, const int32_t* bodies, int32_t count, phx_rigid_body* out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.get_body_states(bodies, count, out);
}

int phx_world_get_poses(phx_world* w, float* out, int32_t cap) { PHX_REQUIRE(w && out, "null handle / buffer"); return w->impl.get_poses(out, cap); }
int phx_world_get_poses_device(phx_world* w, void* d_out, int32_t cap) { PHX_REQUIRE(w, "null handle"); return w->impl.get_poses_device(d_out, cap); }

int phx_world_remove_bodies(phx_world* w, const int32_t* bodies, int32_t count, int32_t* remap)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove("phx_world_remove_bodies", bodies, count, nullptr, nullptr, remap);
}

int phx_world_remove_outside(phx_world* w, const float box[4], int32_t* removed, int32_t* remap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(box, "phx_world_remove_outside: null box");
    return w->impl.remove("phx_world_remove_outside", nullptr, 0, box, removed, remap);
}

int phx_world_add_bodies(phx_world* w, const float* spawn, int32_t count, int32_t* first)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_bodies(spawn, count, first);
}

int phx_world_set_inverse_masses(phx_world* w, const int32_t* bodies, const float* values, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_inverse_masses(bodies, values, count);
}

int phx_world_set_collision_filters(phx_world* w, const int32_t* bodies, const phx_collision_filter* filters, int32_t count, int32_t* dropped)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_collision_filters(bodies, filters, count, dropped);
}

int phx_world_get_collision_filters(phx_world* w, phx_collision_filter* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_collision_filters(out, cap);
}

int phx_world_add_collision_exclusions(phx_world* w, const int32_t* pairs, int32_t count, int32_t* dropped)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_collision_exclusions(pairs, count, dropped);
}

int phx_world_remove_collision_exclusions(phx_world* w, const int32_t* pairs, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove_collision_exclusions(pairs, count);
}

int phx_world_clear_collision_exclusions(phx_world* w)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.clear_collision_exclusions();
}

int phx_world_get_collision_exclusions(phx_world* w, int32_t* out, int32_t cap, int32_t* count)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap <= 0, "null buffer");
    return w->impl.get_collision_exclusions(out, cap, count);
}

int phx_world_set_materials(phx_world* w, const int32_t* bodies, const phx_material* materials, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_materials(bodies, materials, count);
}

int phx_world_get_materials(phx_world* w, phx_material* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_materials(out, cap);
}

int phx_world_set_body_flags(phx_world* w, const int32_t* bodies, const uint32_t* flags, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_body_flags(bodies, flags, count);
}

int phx_world_get_body_flags(phx_world* w, uint32_t* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_body_flags(out, cap);
}

int phx_world_query_aabb(phx_world* w, const float* boxes, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_aabb(boxes, count, flags, offsets, hits, hit_cap, total);
}

int phx_world_query_points(phx_world* w, const float* points, int32_t count, int32_t flags, int32_t* body)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_points(points, count, flags, body);
}

int phx_world_raycast(phx_world* w, const float* rays, int32_t count, int32_t flags, phx_ray_hit* out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.raycast(rays, count, flags, out);
}

int phx_world_query_points_device(phx_world* w, const void* d_points, int32_t count, int32_t flags, void* d_body)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_points_device(d_points, count, flags, d_body);
}

int phx_world_raycast_device(phx_world* w, const void* d_rays, int32_t count, int32_t flags, void* d_out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.raycast_device(d_rays, count, flags, d_out);
}

int phx_world_query_boxes(phx_world* w, const float* boxes, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_boxes(boxes, count, flags, offsets, hits, hit_cap, total);
}

int phx_world_cast_boxes(phx_world* w, const float* casts, int32_t count, int32_t flags, phx_shape_hit* out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.cast_boxes(casts, count, flags, out);
}

int phx_world_cast_boxes_device(phx_world* w, const void* d_casts, int32_t count, int32_t flags, void* d_out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.cast_boxes_device(d_casts, count, flags, d_out);
}

int phx_world_query_contacts(phx_world* w, const int32_t* bodies, int32_t count, int32_t flags, int32_t* offsets, phx_contact* out, int32_t cap, int64_t* total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_contacts(bodies, count, flags, offsets, out, cap, total);
}

int phx_world_contact_events(phx_world* w, int32_t* begin, int32_t begin_cap, int64_t* begin_total, int32_t* end, int32_t end_cap, int64_t* end_total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.contact_events(begin, begin_cap, begin_total, end, end_cap, end_total);
}

int phx_world_get_contact_markers_device(phx_world* w, void* d_out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.contact_markers_device(d_out, cap);
}

int phx_world_set_state(phx_world* w, const phx_rigid_body* bodies, int32_t body_count, const phx_manifold* manifolds, int32_t manifold_count,
                        const phx_contact_point* contact_points, int32_t contact_point_count, const phx_contact_joint* joints, int32_t joint_count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_state(bodies, body_count, manifolds, manifold_count, contact_points, contact_point_count, joints, joint_count);
}

// ---- re-slab (reslab.hip) ----
static int slab_transport(const phx_slab_transport* t, phx::World& world, phx::SlabTransport* out)
{
    out->rank = 0; out->size = 1; out->stream = world.stream();
    if (!t) return PHX_OK;
    PHX_REQUIRE(t->size >= 1 && t->rank >= 0 && t->rank < t->size, "bad rank / size");
    out->rank = t->rank; out->size = t->size; out->user = t->user;
    out->gather_fn = t->all_gather; out->max_fn = reinterpret_cast<int (*)(void*, long long*)>(t->all_reduce_max);
    if (t->comm) {
        PHX_REQUIRE(t->comm->impl.size() == t->size && t->comm->impl.rank() == t->rank, "the communicator's rank / size differ from the transport's");
        out->comm = &t->comm->impl;
    }
    return PHX_OK;
}

int phx_world_reslab_intervals(phx_world* w, const int64_t* global_index, int32_t body_count, int64_t* gi, double* lo, double* hi, int32_t cap, int32_t* count)
{
    PHX_REQUIRE(w && global_index && count, "null handle / arguments");
    phx::SlabState st;
    PHX_TRY(w->impl.get_slab_state(reinterpret_cast<const long long*>(global_index), body_count, &st));
    std::vector<long long> g; std::vector<double> l, h;
    PHX_TRY(phx::reslab_intervals(st, g, l, h));
    *count = (int32_t)g.size();
    if ((int)g.size() > cap) { phx::set_error("re-slab: %zu dynamic bodies, room for %d", g.size(), cap); return PHX_ERR_CAPACITY; }
    PHX_REQUIRE(g.empty() || (gi && lo && hi), "null output");
    for (size_t k = 0; k < g.size(); ++k) { gi[k] = g[k]; lo[k] = l[k]; hi[k] = h[k]; }
    return PHX_OK;
}

int phx_reslab_plan(int64_t* gi, double* lo, double* hi, int32_t n, int32_t nranks, double margin, int32_t* owner, double* bounds)
{
    PHX_REQUIRE(n >= 0 && nranks >= 1 && bounds && (n == 0 || (gi && lo && hi && owner)), "bad arguments");
    std::vector<long long> g(gi, gi + n); std::vector<double> l(lo, lo + n), h(hi, hi + n), b;
    std::vector<int> o;
    phx::reslab_plan(g, l, h, nranks, margin, o, b);
    for (int k = 0; k < n; ++k) { gi[k] = g[(size_t)k]; lo[k] = l[(size_t)k]; hi[k] = h[(size_t)k]; owner[k] = o[(size_t)k]; }
    for (int r = 0; r < 2 * nranks; ++r) bounds[r] = b[(size_t)r];
    return PHX_OK;
}

int phx_world_reslab(phx_world* w, const phx_slab_transport* transport, int64_t* global_index, int32_t capacity, int32_t* body_count, int32_t scene_size, double margin,
                     double bounds[2], int32_t* moved)
{
    PHX_REQUIRE(w && global_index && body_count && bounds && moved, "null handle / arguments");
    PHX_REQUIRE(scene_size >= *body_count && capacity >= *body_count, "bad sizes");
    PHX_TRY(w->impl.refuse_pins("phx_world_reslab"));
    PHX_TRY(w->impl.refuse_tables("phx_world_reslab"));
    PHX_TRY(w->impl.refuse_exclusions("phx_world_reslab"));
    phx::SlabTransport tp;
    PHX_TRY(slab_transport(transport, w->impl, &tp));
    phx::SlabState st;
    PHX_TRY(w->impl.get_slab_state(reinterpret_cast<const long long*>(global_index), *body_count, &st));
    int mv = 0;
    PHX_TRY(phx::reslab(tp, st, scene_size, margin, bounds, &mv));
    *moved = mv;
    if (!mv) return PHX_OK;                                   // nobody changes owner: the world stays as it is, only its slab's bounds are new
    if ((int)st.bodies.size() > capacity) { phx::set_error("re-slab: the new slab holds %zu bodies, room for %d scene indices", st.bodies.size(), capacity); return PHX_ERR_CAPACITY; }
    PHX_TRY(w->impl.set_state(st.bodies.data(), (int)st.bodies.size(), st.manifolds.data(), (int)st.manifolds.size(), st.cps.data(), (int)st.cps.size(),
                              st.joints.data(), (int)st.joints.size()));
    for (size_t k = 0; k < st.global_index.size(); ++k) global_index[k] = st.global_index[k];
    *body_count = (int32_t)st.bodies.size();
    return PHX_OK;
}

int phx_world_add_pins(phx_world* w, const phx_pin* pins, int32_t count, int32_t* first)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_units(pins, count, first);
}

int phx_world_remove_pins(phx_world* w, const int32_t* pins, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove_units<phx_pin>(pins, count);
}

int phx_world_set_pin_anchors(phx_world* w, const int32_t* pins, const float* anchors, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_anchors<phx_pin>(pins, anchors, count);
}

int phx_world_get_pins(phx_world* w, phx_pin* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_units(out, cap);
}

int phx_world_add_links(phx_world* w, const phx_link* links, int32_t count, int32_t* first)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_units(links, count, first);
}

int phx_world_remove_links(phx_world* w, const int32_t* links, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove_units<phx_link>(links, count);
}

int phx_world_set_link_anchors(phx_world* w, const int32_t* links, const float* anchors, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_anchors<phx_link>(links, anchors, count);
}

int phx_world_set_link_lengths(phx_world* w, const int32_t* links, const float* lengths, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_link_lengths(links, lengths, count);
}

int phx_world_get_links(phx_world* w, phx_link* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_units(out, cap);
}

int phx_world_link_count(phx_world* w, int32_t* count)
{
    PHX_REQUIRE(w && count, "null handle / output");
    return w->impl.unit_count<phx_link>(count);
}

int phx_world_add_angles(phx_world* w, const phx_angle* angles, int32_t count, int32_t* first)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_units(angles, count, first);
}

int phx_world_remove_angles(phx_world* w, const int32_t* angles, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove_units<phx_angle>(angles, count);
}

int phx_world_set_angle_limits(phx_world* w, const int32_t* angles, const float* limits, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_limits<phx_angle>(angles, limits, count);
}

int phx_world_set_angle_motors(phx_world* w, const int32_t* angles, const float* motors, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_motors<phx_angle>(angles, motors, count);
}

int phx_world_get_angles(phx_world* w, phx_angle* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_units(out, cap);
}

int phx_world_angle_count(phx_world* w, int32_t* count)
{
    PHX_REQUIRE(w && count, "null handle / output");
    return w->impl.unit_count<phx_angle>(count);
}

int phx_world_add_sliders(phx_world* w, const phx_slider* sliders, int32_t count, int32_t* first)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.add_units(sliders, count, first);
}

int phx_world_remove_sliders(phx_world* w, const int32_t* sliders, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.remove_units<phx_slider>(sliders, count);
}

int phx_world_set_slider_anchors(phx_world* w, const int32_t* sliders, const float* anchors, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_anchors<phx_slider>(sliders, anchors, count);
}

int phx_world_set_slider_limits(phx_world* w, const int32_t* sliders, const float* limits, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_limits<phx_slider>(sliders, limits, count);
}

int phx_world_set_slider_motors(phx_world* w, const int32_t* sliders, const float* motors, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_unit_motors<phx_slider>(sliders, motors, count);
}

int phx_world_get_sliders(phx_world* w, phx_slider* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_units(out, cap);
}

int phx_world_slider_count(phx_world* w, int32_t* count)
{
    PHX_REQUIRE(w && count, "null handle / output");
    return w->impl.unit_count<phx_slider>(count);
}

int phx_world_set_break_limits(phx_world* w, int32_t kind, const int32_t* units, const float* limits, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_break_limits(kind, units, limits, count);
}

int phx_world_get_break_limits(phx_world* w, int32_t kind, float* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_break_limits(kind, out, cap);
}

int phx_world_set_sleeping(phx_world* w, const phx_sleep_params* p) { PHX_REQUIRE(w, "null handle"); return w->impl.set_sleeping(p); }
int phx_world_get_sleeping(phx_world* w, phx_sleep_params* out, int32_t* enabled) { PHX_REQUIRE(w, "null handle"); return w->impl.get_sleeping(out, enabled); }
int phx_world_get_sleep_states(phx_world* w, phx_sleep_state* out, int32_t cap) { PHX_REQUIRE(w && (out || cap == 0), "null handle / buffer"); return w->impl.get_sleep_states(out, cap); }
int phx_world_wake_bodies(phx_world* w, const int32_t* bodies, int32_t count) { PHX_REQUIRE(w, "null handle"); return w->impl.wake_bodies(bodies, count); }
int phx_world_sleep_counts(phx_world* w, int32_t* asleep, int64_t* slept_total, int64_t* woken_total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.sleep_counts(asleep, slept_total, woken_total);
}

int phx_world_break_events(phx_world* w, phx_break_event* out, int32_t cap, int64_t* total)
{
    PHX_REQUIRE(w && total, "null handle / output");
    PHX_REQUIRE(out || cap <= 0, "null buffer");
    return w->impl.break_events(out, cap, total);
}

int phx_world_pin_count(phx_world* w, int32_t* count)
{
    PHX_REQUIRE(w && count, "null handle / output");
    return w->impl.unit_count<phx_pin>(count);
}

int phx_world_set_pin_iterations(phx_world* w, int32_t n)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_pin_iterations(n);
}

int phx_world_get_pin_iterations(phx_world* w, int32_t* n)
{
    PHX_REQUIRE(w && n, "null handle / output");
    *n = w->impl.pins().iterations;
    return PHX_OK;
}

int phx_world_pin_schedule_builds(phx_world* w, int64_t* builds)
{
    PHX_REQUIRE(w && builds, "null handle / output");
    *builds = w->impl.pins().builds();
    return PHX_OK;
}

int phx_world_get_pin_schedule(phx_world* w, int32_t* order, int32_t order_cap, int32_t* class_offsets, int32_t class_cap, int32_t* class_count,
                               int32_t* group_offsets, int32_t group_cap, int32_t* group_count, int32_t* lds_group_count)
{
    PHX_REQUIRE(w && class_count && group_count && lds_group_count, "null handle / output");
    const phx::Schedule* s = nullptr;
    PHX_TRY(w->impl.pin_schedule(&s));
    *class_count = s ? (int)s->colour_offsets.size() - 1 : 0;
    *group_count = s ? s->ngroups() : 0;
    *lds_group_count = s ? s->lds_groups : 0;
    if (!order && !class_offsets && !group_offsets) return PHX_OK;
    PHX_REQUIRE(class_offsets && group_offsets && (order || !s), "phx_world_get_pin_schedule: null output");
    const int n = s ? (int)s->order.size() : 0;
    if (order_cap < n || class_cap < *class_count + 1 || group_cap < *group_count + 1) { phx::set_error("phx_world_get_pin_schedule: arrays too small"); return PHX_ERR_CAPACITY; }
    class_offsets[0] = 0; group_offsets[0] = 0;
    if (!s) return PHX_OK;
    std::copy(s->order.begin(), s->order.end(), order);
    std::copy(s->colour_offsets.begin(), s->colour_offsets.end(), class_offsets);
    std::copy(s->group_offsets.begin(), s->group_offsets.end(), group_offsets);
    return PHX_OK;
}

int phx_world_save(phx_world* w, phx_snapshot* s)
{
    PHX_REQUIRE(w && s, "phx_world_save: null handle");
    return w->impl.save(s->impl);
}

int phx_world_load(phx_world* w, phx_snapshot* s)
{
    PHX_REQUIRE(w && s, "phx_world_load: null handle");
    return w->impl.load(s->impl);
}

int phx_world_get_solve_stats(phx_world* w, phx_solve_stats* out) { PHX_REQUIRE(w, "null handle"); return w->impl.solver().get_stats(out); }
int phx_world_get_broadphase_stats(phx_world* w, phx_broadphase_stats* out) { PHX_REQUIRE(w, "null handle"); return w->impl.broadphase().get_stats(out); }

phx_solver* phx_world_solver(phx_world* w) { return w ? &w->impl.solver_h : nullptr; }
phx_broadphase* phx_world_broadphase(phx_world* w) { return w ? &w->impl.broadphase_h : nullptr; }

int phx_world_synchronize(phx_world* w)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.synchronize();
}

int phx_world_debug_counters(phx_world* w, int64_t out4[4])
{
    PHX_REQUIRE(w && out4, "null handle / buffer");
    out4[0] = w->impl.deferred_packs; out4[1] = w->impl.deferred_pack_retries;
    out4[2] = (int64_t)w->impl.solver().replays(); out4[3] = (int64_t)w->impl.dropped_points;
    return PHX_OK;
}

int phx_world_build_counts(phx_world* w, int64_t out2[2])
{
    PHX_REQUIRE(w && out2, "null handle / buffer");
    w->impl.solver().build_counts(out2);
    return PHX_OK;
}

int phx_world_query_index(phx_world* w, int64_t* builds)
{
    PHX_REQUIRE(w, "null handle");
    PHX_TRY(w->impl.query_index_build());
    if (builds) *builds = w->impl.query_index_builds();
    return PHX_OK;
}

int phx_world_contact_index(phx_world* w, int64_t* builds)
{
    PHX_REQUIRE(w, "null handle");
    PHX_TRY(w->impl.contact_index_build());
    if (builds) *builds = w->impl.contact_index_builds();
    return PHX_OK;
}

int phx_world_x_extent(phx_world* w, float out2[2])
{
    PHX_REQUIRE(w && out2, "null handle / buffer");
    return w->impl.x_extent(out2);
}

int phx_world_set_phase_timing(phx_world* w, int32_t on)
{
    PHX_REQUIRE(w, "null handle");
    w->impl.phase_timing = on != 0;
    return PHX_OK;
}

int phx_world_get_phase_ms(phx_world* w, double out8[8])
{
    PHX_REQUIRE(w && out8, "null handle / buffer");
    for (int i = 0; i < 8; ++i) out8[i] = w->impl.phase_ms[i];
    return PHX_OK;
}

} // extern "C"
