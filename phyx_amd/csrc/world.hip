// world.hip — World (world.h): construction, host staging and the upload, and the step of ref: src/World.cpp:19-37.
//
// Per step: IntegrateVelocity (kernel) -> UpdateBroadphase + UpdatePairs (DeviceBroadphase) ->
// manifold creation + UpdateManifolds (narrowphase kernel) -> PackManifolds -> RefreshContactJoints (scan-based,
// order-preserving, world_kernels.h) -> SolveJoints (DeviceSolver) -> IntegratePosition (kernel).  What crosses
// PCIe per step is a handful of counters (new pairs, dead manifolds, new / dead joints) and, only when the joint
// topology changed, the body-pair list the host schedule builder needs.
#include "world.h"
#include "device_scan.h"

#include <chrono>

namespace phx {

constexpr int PRELABEL_EARLY_MANIFOLDS = 400000;      // worlds from this size on queue the side stream's share of the schedule rebuild before the joint match (refresh_contact_joints)

World::~World()
{
    if (hipSetDevice(device_) != hipSuccess) return;
    if (stream_) (void)hipStreamSynchronize(stream_);
    sweep_.release();
    stage_.release();                                                       // (only here: the device is current and no copy is queued any more)
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
phx_rigid_body body_record(float px, float py, float angle, float sx, float sy)
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

int World::settle_and_upload()
{
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());                                         // (an unverified solve is settled before its results are read or anything moves)
    return sync_bodies_to_device();                                         // (host-staged bodies go up as the next step would take them)
}

// The sharded modes carry no unit, no sleeping, no optional column, no force field and no collision exclusion: refused, in this order,
// while the world holds one.  (`fields`: phx_world_set_shard and set_comm; a re-slab hands bodies over and a field names none.)
int World::refuse_unsharded_state(const char* what, bool fields)
{
    if (pins_.units()) {
        const char* plural = nullptr;                                       // the first kind the world holds names the refusal
        pins_.each_list([&](auto& l) { if (!plural && l.count()) plural = UnitKind<typename std::decay_t<decltype(l)>::record>::plural; return PHX_OK; });
        set_error("%s: the world holds %s, which a sharded world does not carry", what, plural);
        return PHX_ERR_STATE;
    }
    if (sleep_.on()) { set_error("%s: sleeping is enabled, which a sharded world does not carry (phx_world_set_sleeping(w, NULL) first)", what); return PHX_ERR_STATE; }
    PHX_TRY(each_table([&](auto& t) -> int {                                // an optional column: refused while some body's value is not the default
        using Column = typename std::decay_t<decltype(t)>::column;
        if (!t.active) return PHX_OK;
        bool all_default = true;
        PHX_TRY(t.visit(nb(), host_staged(), device_, rb_, stream_, [&](int, const typename Column::value& v) { all_default &= Column::is_initial(v); }));
        if (!all_default) { set_error("%s: the world holds %s, which a sharded world does not carry", what, Column::plural); return PHX_ERR_STATE; }
        t.reset();                                                          // (every value is the default again: the plain kernels)
        return PHX_OK;
    }));
    if (fields && fields_.count()) { set_error("%s: the world holds force fields, which a sharded world does not carry (phx_world_set_fields(w, NULL, 0) first)", what); return PHX_ERR_STATE; }
    if (!exclusions_.empty()) { set_error("%s: the world holds %d collision exclusions, which a sharded world does not carry", what, exclusions_.count()); return PHX_ERR_STATE; }
    return PHX_OK;
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

// UpdateManifolds' kernel over manifolds [first, nm): the box/box instantiation, or the one that reads the kinds while the shape column
// is active (a null column pointer picks the plain instantiation: the kernel of a world that never made a circle), or the third, with
// the capsule routines, once some call has named a capsule
void World::queue_update_manifolds(int first, int nm_old, const uint2* new_pairs, const MailRide& ride)
{
    const uint32_t* const kinds = shapes_.ptr();
    // (the fourth, with the polygon routines and the polygon column, once some call has named a polygon)
    if (kinds && polygons()) hipLaunchKernelGGL(k_update_manifolds<BodyPolygons>, dim3(wgrid(nm - first)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p, pack_flags_.p,
                                                reinterpret_cast<int*>(counters_.p + 3), nm_old, new_pairs, first, counters_.p + 2, ride, BodyPolygons{kinds, polys_.ptr()});
    else if (kinds && capsules())hipLaunchKernelGGL(k_update_manifolds<BodyCapsules>, dim3(wgrid(nm - first)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p, pack_flags_.p,
                                                reinterpret_cast<int*>(counters_.p + 3), nm_old, new_pairs, first, counters_.p + 2, ride, BodyCapsules{kinds});
    else if (kinds) hipLaunchKernelGGL(k_update_manifolds<BodyShapes>, dim3(wgrid(nm - first)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p, pack_flags_.p,
                                  reinterpret_cast<int*>(counters_.p + 3), nm_old, new_pairs, first, counters_.p + 2, ride, BodyShapes{kinds});
    else hipLaunchKernelGGL(k_update_manifolds<AllBoxes>, dim3(wgrid(nm - first)), dim3(256), 0, stream_, d_manifolds_.p, nm, resident(), d_cps_.p, pack_flags_.p,
                            reinterpret_cast<int*>(counters_.p + 3), nm_old, new_pairs, first, counters_.p + 2, ride, AllBoxes{});
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
        queue_update_manifolds(0, nm, nullptr, old_ride_ ? *old_ride_ : MailRide{});
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
    queue_update_manifolds(first, nm - fresh_manifolds_, broadphase_.new_pairs_device(), MailRide{});
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
    if (sweep_col_.active) PHX_TRY(sweep_begin());                          // (the continuous bodies' start: positions do not move before the integrator)
    if (phase_timing) {                                                     // (per-phase host timing: settle the solve before the integrator)
        { RoctxRange r("SolveJoints"); PHX_TRY(solve(cfg, true)); lap(6); }
        RoctxRange r("IntegratePosition");
        ++geom_epoch_;
        if (nb()) hipLaunchKernelGGL(k_integrate_position, dim3(wgrid(nb())), dim3(256), 0, stream_, resident(), nb(), dt, (const unsigned long long*)nullptr, 0ull, MailRide{});
        PHX_HIP(hipGetLastError());
    } else PHX_TRY(solve_and_integrate(dt, cfg));
    records_stale_ = true;
    // (by now the integrator that counts, a repeat included, is queued: the continuous bodies' pass goes behind it, in front of the sleep pass)
    if (sweep_col_.active) PHX_TRY(sweep_pass());                           // (a world that never named a continuous body queues nothing here)
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

} // namespace phx
