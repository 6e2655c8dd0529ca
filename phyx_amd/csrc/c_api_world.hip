// c_api_world.hip — extern "C" surface of the World (include/phyx_amd.h): argument checks that need no world, then the call.
#include "world.h"

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
    if (count > 1) PHX_TRY(w->impl.refuse_unsharded_state("phx_world_set_shard", true));
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
    if (c) PHX_TRY(w->impl.refuse_unsharded_state("phx_world_set_comm", true));
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

int phx_world_set_shapes(phx_world* w, const int32_t* bodies, const phx_shape* shapes, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_shapes(bodies, shapes, count);
}

int phx_world_get_shapes(phx_world* w, phx_shape* out, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    PHX_REQUIRE(out || cap == 0, "null buffer");
    return w->impl.get_shapes(out, cap);
}

int phx_world_set_polygons(phx_world* w, const int32_t* bodies, const phx_polygon* polygons, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_polygons(bodies, polygons, count);
}

int phx_world_get_polygons(phx_world* w, const int32_t* bodies, phx_polygon* out, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.get_polygons(bodies, out, count);
}

int phx_world_set_continuous(phx_world* w, const int32_t* bodies, const float* radii, int32_t count)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.set_continuous(bodies, radii, count);
}

int phx_world_get_continuous(phx_world* w, float* out_radii, int32_t cap)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.get_continuous(out_radii, cap);
}

int phx_world_sweep_hits(phx_world* w, phx_sweep_hit* out, int32_t cap, int64_t* total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.sweep_hits(out, cap, total);
}

int phx_world_sweep_counts(phx_world* w, int64_t* passes, int64_t* clamps_total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.sweep_counts(passes, clamps_total);
}

int phx_world_sweep_timing(phx_world* w, int32_t enable, double* last_pass_ms)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.sweep_timing(enable, last_pass_ms);
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

int phx_world_query_circles(phx_world* w, const float* circles, int32_t count, int32_t flags, int32_t* offsets, int32_t* hits, int32_t hit_cap, int64_t* total)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_circles(circles, count, flags, offsets, hits, hit_cap, total);
}

int phx_world_cast_circles(phx_world* w, const float* casts, int32_t count, int32_t flags, phx_shape_hit* out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.cast_circles(casts, count, flags, out);
}

int phx_world_cast_circles_device(phx_world* w, const void* d_casts, int32_t count, int32_t flags, void* d_out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.cast_circles_device(d_casts, count, flags, d_out);
}

int phx_world_query_nearest(phx_world* w, const float* queries, int32_t count, int32_t flags, phx_near_hit* out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_nearest(queries, count, flags, out);
}

int phx_world_query_nearest_device(phx_world* w, const void* d_queries, int32_t count, int32_t flags, void* d_out)
{
    PHX_REQUIRE(w, "null handle");
    return w->impl.query_nearest_device(d_queries, count, flags, d_out);
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
    PHX_TRY(w->impl.refuse_unsharded_state("phx_world_reslab", false));      // (without fields: a field names no body, include/phyx_amd.h FORCE FIELDS)
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
