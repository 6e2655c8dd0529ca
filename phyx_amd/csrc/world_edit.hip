// world_edit.hip — World (world.h): what changes bodies and their columns between steps: edits and gathers, removal, spawn, the optional
// columns (collision filters, materials, body flags, shapes), collision exclusions, and the contact cache's compaction behind them.
#include "world.h"
#include "device_scan.h"

namespace phx {

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
    PHX_TRY(stage_.indexed(bodies, values, count, width, stream_, &d_bodies, &d_values));
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
    const int* d_bodies = nullptr;
    PHX_TRY(stage_.indices(bodies, count, stream_, &d_bodies));
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
    if (nm) hipLaunchKernelGGL((k_remove_manifolds<Keep>), dim3(stream_grid(nm)), dim3(256), 0, stream_, (const phx_manifold*)d_manifolds_.p, (const phx_contact_point*)d_cps_.p, nm,
                               kept, (const unsigned*)rm_mnew_.p, (const unsigned*)rm_jnew_.p, (const unsigned*)(rm_counts_.p + 2), nj, spare_.manifolds.p, spare_.cps.p, rm_pairs_.p);
    if (nj) hipLaunchKernelGGL((k_remove_joints<Keep>), dim3(stream_grid(nj)), dim3(256), 0, stream_, (const phx_contact_joint*)d_joints_.p, nj, (const phx_manifold*)d_manifolds_.p,
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

// The tail of a call that narrows what may collide (a change of filters, a new exclusion): the manifolds whose pair `kept` rejects go,
// with their slots and joints; the one round trip brings back the kept counts.
template <class Keep>
int World::drop_manifolds(const Keep& kept, int* dropped)
{
    PHX_TRY(compaction_scratch());
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
    PHX_TRY(settle_breaks());
    PHX_TRY(settle_and_upload());                                           // (an unverified solve is settled before anything moves)
    PHX_TRY(rm_keep_.reserve((size_t)n + 2)); PHX_TRY(rm_bnew_.reserve((size_t)n + 2)); PHX_TRY(rm_remap_.reserve((size_t)n));
    PHX_TRY(spare_.bodies.reserve((size_t)n));
    if (accel_pending_) PHX_TRY(spare_.accel.reserve((size_t)n));
    PHX_TRY(each_table([n](auto& t) { return t.reserve_spare((size_t)n); }));
    PHX_TRY(compaction_scratch());
    // 1. keep flags per body
    if (box) {
        hipLaunchKernelGGL(k_keep_inside, dim3(stream_grid(n)), dim3(256), 0, stream_, (const float4*)bodies_.aabb.p, n, make_float4(box[0], box[1], box[2], box[3]), rm_keep_.p);
    } else {
        const int* d_bodies = nullptr;
        PHX_TRY(stage_.indices(bodies, count, stream_, &d_bodies));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(rm_keep_.p), 1, (size_t)n, stream_));
        hipLaunchKernelGGL(k_remove_listed, dim3(stream_grid(count)), dim3(256), 0, stream_, d_bodies, count, rm_keep_.p);
    }
    PHX_HIP(hipGetLastError());
    PHX_TRY(wake_named(nullptr, 0, rm_keep_.p));                            // (the sleeping components that lose a member wake before anything moves)
    // 2. where the kept bodies, manifolds and joints go (a zero count writes a zero total)
    PHX_TRY(device_exclusive_scan_of(BodyKeepLoad{rm_keep_.p}, rm_bnew_.p, n, rm_counts_.p, scan_tiles_, stream_));
    const BodiesKept kept{rm_keep_.p, rm_bnew_.p};
    PHX_TRY(scan_compaction(kept));
    PHX_HIP(hipMemsetAsync(rm_counts_.p + 3, 0, sizeof(unsigned), stream_));
    // 3. compaction into the spares
    hipLaunchKernelGGL(k_remove_bodies, dim3(stream_grid(n)), dim3(256), 0, stream_, (const phx_rigid_body*)bodies_.records.p, resident(), n, records_stale_ ? 1 : 0,
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
    sweep_.changed();                                                       // (the continuous bodies' list holds the old numbering)
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
    const float* d_rows = nullptr;
    PHX_TRY(stage_.values(spawn_rows_.data(), count, SPAWN_ROW, stream_, &d_rows));
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
    PHX_TRY(stage_.indexed(bodies, values, count, 2, stream_, &d_bodies, &d_values));
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
    PHX_TRY(settle_and_upload());                                           // (an unverified solve is settled before the table changes)
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_.indexed(bodies, reinterpret_cast<const float*>(values), count, (int)(sizeof(typename Column::api) / sizeof(float)), stream_, &d_bodies, &d_values));
    return table.set_device(d_bodies, d_values, count, n, stream_);
}

// ---- collision filters ------------------------------------------------------------------------------------------------------------
// The rule and the defaults: include/phyx_amd.h COLLISION FILTERS, common.h collision_filter_pass.  The broadphase applies it inside the
// sweep (broadphase_kernels.h FilteredSweepView), so a failing pair is never emitted; what a change of filters does to pairs that exist already
// is the removal's compaction of the contact cache with the filter as its keep predicate (FilterKept), bodies untouched.
int World::set_collision_filters(const int32_t* bodies, const phx_collision_filter* filters, int count, int* dropped)
{
    PHX_TRY(set_column("phx_world_set_collision_filters", filters_, bodies, filters, count, [](int) { return PHX_OK; }, !nm));      // (on the host while no pair exists to drop)
    if (dropped) *dropped = 0;
    if (!count || !nm) return PHX_OK;
    return drop_manifolds(FilterKept{filters_.dev.p}, dropped);             // the manifolds whose pair now fails
}

// ---- collision exclusions ---------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h COLLISION EXCLUSIONS; the set and its device side: exclusions.h.  The broadphase applies it inside the
// sweep behind the filter (broadphase_kernels.h ExcludedSweepView); what an add does to pairs that exist already is set_collision_filters' own
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
    PHX_TRY(settle_and_upload());                                           // (an unverified solve is settled before anything moves)
    PHX_TRY(exclusions_.sync(nb(), stream_));
    return drop_manifolds(ExclusionKept{exclusions_.view()->table, exclusions_.view()->mask}, dropped);      // the manifolds whose pair is now excluded
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

// ---- shapes -------------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h SHAPES.  The call is an edit of geom_size (the records and the resident size[], the AABB recomputed by
// set_poses' geom_aabb) and, once some call has named a circle or a capsule, a write of the kinds' column.  A call that names boxes only in a world
// without the column is the size edit alone: it activates nothing.  Inverse masses, manifolds, joints and the schedule stay.
int World::set_shapes(const int32_t* bodies, const phx_shape* shapes, int count)
{
    static const char* const what = "phx_world_set_shapes";
    PHX_TRY(refuse_sharded(what, "shapes"));
    PHX_TRY(check_batch(what, bodies, shapes, count, true));
    bool circle = false, capsule = false;                                   // (`circle`: some entry is not a box)
    for (int k = 0; k < count; ++k) {                                       // (NaN fails the comparisons)
        const phx_shape& s = shapes[k];
        if (s.kind != PHX_SHAPE_BOX && s.kind != PHX_SHAPE_CIRCLE && s.kind != PHX_SHAPE_CAPSULE) { set_error("%s: kind %d of body %d is none of PHX_SHAPE_BOX, PHX_SHAPE_CIRCLE, PHX_SHAPE_CAPSULE (a polygon is made by phx_world_set_polygons)", what, s.kind, bodies[k]); return PHX_ERR_INVALID; }
        if (!(std::isfinite(s.hx) && std::isfinite(s.hy) && s.hx > 0.f && s.hy > 0.f)) { set_error("%s: the size {%g, %g} of body %d is not finite and positive", what, (double)s.hx, (double)s.hy, bodies[k]); return PHX_ERR_INVALID; }
        if (s.kind == PHX_SHAPE_CIRCLE && s.hy != s.hx) { set_error("%s: body %d is a circle and hy %g is not its radius hx %g", what, bodies[k], (double)s.hy, (double)s.hx); return PHX_ERR_INVALID; }
        if (s.kind == PHX_SHAPE_CAPSULE && !(s.hx > s.hy)) { set_error("%s: body %d is a capsule and hx %g is not above its radius hy %g (hx == hy: use PHX_SHAPE_CIRCLE)", what, bodies[k], (double)s.hx, (double)s.hy); return PHX_ERR_INVALID; }
        circle = circle || s.kind != PHX_SHAPE_BOX;
        capsule = capsule || s.kind == PHX_SHAPE_CAPSULE;
    }
    if (!count) return PHX_OK;
    PHX_TRY(check_core_radii(what, bodies, shapes, nullptr, count));
    capsules_ = (capsules_ && shapes_.active) || capsule;                   // (a column that went away took the bit with it)
    PHX_TRY(wake_named(bodies, count));
    const int n = nb();
    const bool kinds = circle || shapes_.active;
    if (host_staged()) {                                    // the host-staged records are the world: write into them
        for (int k = 0; k < count; ++k) {
            phx_rigid_body& b = host_bodies_[(size_t)bodies[k]];
            b.geom_size.x = shapes[k].hx; b.geom_size.y = shapes[k].hy;
            update_geom(b);
        }
        if (kinds) shapes_.set_host(bodies, shapes, count, n);              // (the table goes up with the bodies)
        if (polys_.active) { const std::vector<phx_polygon> none((size_t)count); polys_.set_host(bodies, none.data(), count, n); }      // (a polygon named here is one no longer)
        return PHX_OK;
    }
    PHX_TRY(settle_and_upload());                                           // (an unverified solve is settled before the geometry changes)
    PHX_TRY(queue_shapes(bodies, shapes, count, kinds));
    if (polys_.active) { const std::vector<phx_polygon> none((size_t)count); PHX_TRY(queue_polygons(bodies, none.data(), count)); }
    return PHX_OK;
}

// the device path of set_shapes and set_polygons: the batch staged and scattered behind whatever the stream holds
int World::queue_shapes(const int32_t* bodies, const phx_shape* shapes, int count, bool kinds)
{
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_.indexed(bodies, reinterpret_cast<const float*>(shapes), count, (int)(sizeof(phx_shape) / sizeof(float)), stream_, &d_bodies, &d_values));
    if (kinds) PHX_TRY(shapes_.set_device(d_bodies, d_values, count, nb(), stream_));
    hipLaunchKernelGGL(k_set_shapes, dim3(wgrid(count)), dim3(256), 0, stream_, d_bodies, reinterpret_cast<const phx_shape*>(d_values), count, resident(), bodies_.records.p);
    PHX_HIP(hipGetLastError());
    ++geom_epoch_;                                                          // (the query index was built on the old AABBs)
    return PHX_OK;
}
int World::queue_polygons(const int32_t* bodies, const phx_polygon* polygons, int count)
{
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_.indexed(bodies, reinterpret_cast<const float*>(polygons), count, (int)(sizeof(phx_polygon) / sizeof(float)), stream_, &d_bodies, &d_values));
    return polys_.set_device(d_bodies, d_values, count, nb(), stream_);
}

// ---- polygons -----------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h POLYGONS.  Validity in fp32, by the expressions tests/polygon_spec.py poly_valid states; then the call is
// set_shapes of {PHX_SHAPE_POLYGON, the frame box} and a write of the polygon column, whose stored value (the normals) is formed by
// poly_record on either path.
static const char* polygon_fault(const phx_polygon& p)
{
    if (p.count < 3 || p.count > PHX_POLYGON_MAX_VERTICES) return "its vertex count is not in 3 .. 8";
    for (int k = 0; k < p.count; ++k)
        if (!(std::isfinite(p.v[k].x) && std::isfinite(p.v[k].y))) return "a coordinate is not finite";
    const PolyRec r = poly_record(p);
    for (int k = 0; k < p.count; ++k) {
        const int k1 = k + 1 < p.count ? k + 1 : 0, k2 = k1 + 1 < p.count ? k1 + 1 : 0;
        const V2 e0 = v2(p.v[k1]) - v2(p.v[k]), e1 = v2(p.v[k2]) - v2(p.v[k1]);
        if (!(e0.x * e1.y - e0.y * e1.x > 0.0f)) return "it is not strictly convex and counter-clockwise";
        if (!(dot(v2(r.n[2 * k], r.n[2 * k + 1]), v2(p.v[k])) > 0.0f)) return "the origin is not strictly inside";
    }
    return nullptr;
}

int World::set_polygons(const int32_t* bodies, const phx_polygon* polygons, int count)
{
    static const char* const what = "phx_world_set_polygons";
    PHX_TRY(refuse_sharded(what, "polygons"));
    PHX_TRY(check_batch(what, bodies, polygons, count, true));
    std::vector<phx_polygon> clean((size_t)count);                          // (unused slots are stored as +0)
    std::vector<phx_shape> frame((size_t)count);
    for (int k = 0; k < count; ++k) {
        if (const char* bad = polygon_fault(polygons[k])) { set_error("%s: the polygon of body %d is refused: %s", what, bodies[k], bad); return PHX_ERR_INVALID; }
        phx_polygon& c = clean[(size_t)k];
        c = phx_polygon{};
        c.count = polygons[k].count;
        float hx = 0.f, hy = 0.f;
        for (int j = 0; j < c.count; ++j) {
            c.v[j] = polygons[k].v[j];
            hx = fabsf(c.v[j].x) > hx ? fabsf(c.v[j].x) : hx; hy = fabsf(c.v[j].y) > hy ? fabsf(c.v[j].y) : hy;
        }
        frame[(size_t)k] = phx_shape{PHX_SHAPE_POLYGON, hx, hy};
    }
    if (!count) return PHX_OK;
    PHX_TRY(check_core_radii(what, bodies, frame.data(), clean.data(), count));
    capsules_ = capsules_ && shapes_.active;                                // (a column that went away took the bits with it)
    polygons_ = true;
    PHX_TRY(wake_named(bodies, count));
    const int n = nb();
    if (host_staged()) {                                    // the host-staged records are the world: write into them
        for (int k = 0; k < count; ++k) {
            phx_rigid_body& b = host_bodies_[(size_t)bodies[k]];
            b.geom_size.x = frame[(size_t)k].hx; b.geom_size.y = frame[(size_t)k].hy;
            update_geom(b);
        }
        shapes_.set_host(bodies, frame.data(), count, n);
        polys_.set_host(bodies, clean.data(), count, n);
        return PHX_OK;
    }
    PHX_TRY(settle_and_upload());
    PHX_TRY(queue_shapes(bodies, frame.data(), count, true));
    return queue_polygons(bodies, clean.data(), count);
}

// the listed bodies' polygons in the C ABI's form (count 0 and zeros for a body that is none)
int World::get_polygons(const int32_t* bodies, phx_polygon* out, int count)
{
    static const char* const what = "phx_world_get_polygons";
    PHX_TRY(refuse_mid_step(what));
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && (!bodies || !out)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = nb();
    for (int k = 0; k < count; ++k)
        if (bodies[k] < 0 || bodies[k] >= n) { set_error("%s: body index %d out of range [0, %d)", what, bodies[k], n); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    std::vector<phx_polygon> all((size_t)n);
    PHX_TRY(polys_.visit(n, host_staged(), device_, rb_, stream_, [&](int i, const PolyRec& v) { all[(size_t)i] = PolygonColumn::shown(v); }));
    for (int k = 0; k < count; ++k) out[k] = all[(size_t)bodies[k]];
    return PHX_OK;
}

// ---- continuous bodies ---------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h CONTINUOUS BODIES.  The call writes the column's core radii and nothing else; the next step's two launches
// (sweep.h) do the rest.  What is checked: the batch, every radius, and rc against the body's inradius about its origin.
static float inradius_of(const phx_shape& s, const phx_polygon* polygon)
{
    if (s.kind == PHX_SHAPE_CIRCLE) return s.hx;
    if (s.kind == PHX_SHAPE_CAPSULE) return s.hy;
    if (s.kind == PHX_SHAPE_POLYGON && polygon) {
        const PolyRec r = poly_record(*polygon);
        float least = INFINITY;
        for (int k = 0; k < r.count && k < PHX_POLYGON_MAX_VERTICES; ++k) {
            const float d = dot(v2(r.n[2 * k], r.n[2 * k + 1]), v2(r.v[2 * k], r.v[2 * k + 1]));
            least = d < least ? d : least;
        }
        return least;
    }
    return s.hx < s.hy ? s.hx : s.hy;
}

extern "C" int phx_continuous_check(const char* what, int32_t body, const phx_shape* shape, const phx_polygon* polygon, float rc)
{
    if (!what) what = "phx_continuous_check";
    if (!shape) { set_error("%s: null shape", what); return PHX_ERR_INVALID; }
    if (shape->kind == PHX_SHAPE_POLYGON && !polygon) { set_error("%s: body %d is a polygon and no polygon was given", what, body); return PHX_ERR_INVALID; }
    if (!(std::isfinite(rc) && rc >= 0.f)) { set_error("%s: the core radius %g of body %d is not finite and >= 0", what, (double)rc, body); return PHX_ERR_INVALID; }
    const float r = inradius_of(*shape, polygon);
    if (rc > 0.f && !(rc < r)) { set_error("%s: the core radius %g of body %d is not below its inradius %g", what, (double)rc, body, (double)r); return PHX_ERR_INVALID; }
    return PHX_OK;
}

int World::check_core_radii(const char* what, const int32_t* bodies, const phx_shape* shapes, const phx_polygon* polygons, int count)
{
    if (!sweep_col_.active || !count) return PHX_OK;
    std::vector<float> rc((size_t)nb());
    PHX_TRY(sweep_col_.visit(nb(), host_staged(), device_, rb_, stream_, [&](int i, const float4& v) { rc[(size_t)i] = v.x; }));
    for (int k = 0; k < count; ++k)
        if (rc[(size_t)bodies[k]] > 0.f) PHX_TRY(phx_continuous_check(what, bodies[k], shapes + k, polygons ? polygons + k : nullptr, rc[(size_t)bodies[k]]));
    return PHX_OK;
}

int World::set_continuous(const int32_t* bodies, const float* radii, int count)
{
    static const char* const what = "phx_world_set_continuous";
    PHX_TRY(refuse_sharded(what, SweepColumn::plural));
    PHX_TRY(check_batch(what, bodies, radii, count, true));
    for (int k = 0; k < count; ++k)
        if (!(std::isfinite(radii[k]) && radii[k] >= 0.f)) { set_error("%s: the core radius %g of body %d is not finite and >= 0", what, (double)radii[k], bodies[k]); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    const int n = nb();
    std::vector<phx_shape> shapes((size_t)n);
    PHX_TRY(get_shapes(shapes.data(), n));
    std::vector<phx_polygon> polys;
    if (polys_.active) {
        polys.resize((size_t)n);
        PHX_TRY(polys_.visit(n, host_staged(), device_, rb_, stream_, [&](int i, const PolyRec& v) { polys[(size_t)i] = PolygonColumn::shown(v); }));
    }
    for (int k = 0; k < count; ++k) {
        const phx_shape& s = shapes[(size_t)bodies[k]];
        if (s.kind == PHX_SHAPE_POLYGON && polys.empty()) { set_error("%s: body %d is a polygon without a record", what, bodies[k]); return PHX_ERR_STATE; }
        PHX_TRY(phx_continuous_check(what, bodies[k], &s, polys.empty() ? nullptr : &polys[(size_t)bodies[k]], radii[k]));
    }
    bool any = sweep_col_.active;
    for (int k = 0; k < count; ++k) any = any || radii[k] > 0.f;
    if (!any) return PHX_OK;                                                // (discrete bodies made discrete in a world without the column: nothing to write)
    PHX_TRY(settle_and_upload());                                           // (host-staged bodies go up first: the column lives beside the resident arrays)
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_.indexed(bodies, radii, count, 1, stream_, &d_bodies, &d_values));
    PHX_TRY(sweep_col_.set_device(d_bodies, d_values, count, n, stream_));
    sweep_.changed();
    return PHX_OK;
}

int World::get_continuous(float* out, int cap)
{
    static const char* const what = "phx_world_get_continuous";
    PHX_TRY(refuse_mid_step(what));
    if (nb() && !out) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    return get_table(what, sweep_col_, out, cap);
}

int World::sweep_hits(phx_sweep_hit* out, int cap, int64_t* total)
{
    static const char* const what = "phx_world_sweep_hits";
    PHX_TRY(refuse_mid_step(what));
    if (cap < 0 || (cap && !out)) { set_error("%s: bad capacity or null array", what); return PHX_ERR_INVALID; }
    PHX_TRY(settle_on_device());
    return sweep_.hits(out, cap, total, rb_, stream_);
}

int World::sweep_counts(int64_t* passes, int64_t* clamps_total)
{
    PHX_TRY(refuse_mid_step("phx_world_sweep_counts"));
    PHX_TRY(settle_on_device());
    return sweep_.counts(passes, clamps_total, rb_, stream_);
}

int World::sweep_timing(int enable, double* last_pass_ms)
{
    PHX_TRY(refuse_mid_step("phx_world_sweep_timing"));
    PHX_TRY(use_device(device_));
    if (last_pass_ms) PHX_TRY(sweep_.pass_ms(last_pass_ms));
    return sweep_.timing(enable != 0);
}

// every body's {kind, geom_size}: the kinds from the column (boxes while there is none), the sizes from wherever the bodies are
int World::get_shapes(phx_shape* out, int cap)
{
    static const char* const what = "phx_world_get_shapes";
    const int n = nb();
    if (cap < n) { set_error("%s: room for %d bodies, the world has %d", what, cap, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    PHX_TRY(shapes_.visit(n, host_staged(), device_, rb_, stream_, [out](int i, const uint32_t& kind) { out[i].kind = (int32_t)kind; }));
    if (host_staged()) {
        for (int i = 0; i < n; ++i) { out[i].hx = host_bodies_[(size_t)i].geom_size.x; out[i].hy = host_bodies_[(size_t)i].geom_size.y; }
        return PHX_OK;
    }
    PHX_TRY(use_device(device_));
    std::vector<float2> sizes((size_t)n);
    PHX_TRY(rb_.add(sizes.data(), bodies_.size.p, (size_t)n * sizeof(float2), stream_));
    PHX_TRY(rb_.wait(stream_));
    for (int i = 0; i < n; ++i) { out[i].hx = sizes[(size_t)i].x; out[i].hy = sizes[(size_t)i].y; }
    return PHX_OK;
}

} // namespace phx
