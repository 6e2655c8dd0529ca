// world_state.hip — World (world.h): the whole state out and in: the downloads, set_state, snapshots, the re-slab's hand-over.
#include "world.h"

namespace phx {

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
    capsules_ = false; polygons_ = false;
    sweep_.forget();                                                        // ... and no body is continuous
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
    PHX_TRY(settle_and_upload());
    PHX_TRY(settle_breaks());
    SnapshotWorld v = snapshot_view();
    v.counts.bodies = nb(); v.counts.manifolds = nm; v.counts.joints = nj; v.counts.baseline = contacts_.baseline_count();
    v.counts.columns = (filters_.active ? SNAP_HAS_FILTERS : 0) | (materials_.active ? SNAP_HAS_MATERIALS : 0) | (flags_col_.active ? SNAP_HAS_FLAGS : 0) |
                       (sweep_col_.active ? SNAP_HAS_SWEEP : 0);      // (the last: its section is not the kernel's, it rides beside the blob and joins it at export)
    v.accel_pending = accel_pending_;      // (while it is clear every record's accelerations are zero: IntegrateVelocity clears them)
    PHX_TRY(pins_.upload(stream_));
    PHX_TRY(exclusions_.sync(nb(), stream_));
    PHX_TRY(pins_.each_list([&](auto& l) { return s.reserve_units<typename std::decay_t<decltype(l)>::record>(l.count(), l.limited(), stream_); }));
    PHX_TRY(s.reserve_exclusions(exclusions_.count(), stream_));
    const int kinds = shapes_.active ? nb() : 0;                            // the shapes' kinds ride beside the blob too (the sizes are in the records)
    PHX_TRY(s.reserve_shapes(kinds, stream_));
    const int polys = polys_.active ? nb() : 0;                             // ... and the polygon records
    PHX_TRY(s.reserve_polygons(polys, stream_));
    const int cores = sweep_col_.active ? nb() : 0;                         // ... and the continuous bodies' column
    PHX_TRY(s.reserve_sweep(cores, stream_));
    PHX_TRY(s.save(v, stream_));
    PHX_TRY(pins_.each_list([&](auto& l) { return s.save_units(l.device(), l.device_limits(), l.count(), stream_); }));
    PHX_TRY(s.save_exclusions(exclusions_.device_pairs(), exclusions_.count(), stream_));
    PHX_TRY(s.save_shapes(shapes_.dev.p, kinds, capsules(), stream_));
    PHX_TRY(s.save_polygons(polys_.dev.p, polys, polygons(), stream_));
    return s.save_sweep(sweep_col_.dev.p, cores, stream_);
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
    if (s.shape_count()) PHX_TRY(shapes_.dev.reserve(std::max<size_t>(n, 1)));
    if (s.polygon_count()) PHX_TRY(polys_.dev.reserve(std::max<size_t>(n, 1)));
    if (s.sweep_count()) PHX_TRY(sweep_col_.dev.reserve(std::max<size_t>(n, 1)));
    PHX_TRY(contacts_.reserve_baseline((size_t)c.baseline));
    PHX_TRY(s.load(snapshot_view(), stream_));
    PHX_TRY(s.load_shapes(shapes_.dev.p, stream_));                         // phx_world_set_shapes of the saved kinds, if that column was active in s (the sizes came with the records)
    shapes_.active = s.shape_count() != 0;
    capsules_ = s.shape_capsules();
    PHX_TRY(s.load_polygons(polys_.dev.p, stream_));                        // ... and phx_world_set_polygons of the saved records
    polys_.active = s.polygon_count() != 0;
    polygons_ = s.polygons_named();
    PHX_TRY(s.load_sweep(sweep_col_.dev.p, stream_));                       // ... and phx_world_set_continuous of the saved core radii
    sweep_col_.active = s.sweep_count() != 0;
    sweep_.forget();
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

} // namespace phx
