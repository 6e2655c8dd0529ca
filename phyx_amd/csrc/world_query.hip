// world_query.hip — World (world.h): what reads the world between steps and changes nothing: queries and contact reports.
#include "world.h"

namespace phx {

// ---- queries ------------------------------------------------------------------------------------------------------------------------
// Answered on the world's stream from the resident arrays (query.h / query_kernels.h).  The host forms check everything first, stage the
// queries through the world's pinned staging and wait for their results; the device forms only queue.  Nothing of the world changes:
// the upload of host-staged bodies is the one the next step would make.
static int flags_check(const char* what, int flags)      // (the queries' and the contact lists')
{
    if (flags != 0 && flags != PHX_QUERY_SKIP_STATIC) { set_error("%s: flags %d (0 or PHX_QUERY_SKIP_STATIC)", what, flags); return PHX_ERR_INVALID; }
    return PHX_OK;
}

// what a row of each kind of query holds (World::QueryRows): its width in floats, what the messages call it, and where the values
// with a rule of their own are (-1: none): an AABB's min <= max, an oriented box's half extents, a circle's radius, a direction, max_t, a
// nearest query's max_dist
struct RowRule { int width; const char* noun; bool ordered; int half, radius, dir, max_t, max_dist; };
static const RowRule ROW_RULES[] = {
    {2, "point", false, -1, -1, -1, -1, -1},      // ROWS_POINTS
    {4, "box", true, -1, -1, -1, -1, -1},         // ROWS_BOXES
    {5, "ray", false, -1, -1, 2, 4, -1},          // ROWS_RAYS
    {8, "box", false, 6, -1, -1, -1, -1},         // ROWS_SHAPES
    {11, "cast", false, 6, -1, 8, 10, -1},        // ROWS_CASTS
    {3, "circle", false, -1, 2, -1, -1, -1},      // ROWS_CIRCLES
    {6, "cast", false, -1, 2, 3, 5, -1},          // ROWS_CIRCLE_CASTS
    {3, "point", false, -1, -1, -1, -1, 2},       // ROWS_NEAR
};

static int query_check(const char* what, const float* v, int count, const RowRule& r, int flags, bool device, const void* out)
{
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    PHX_TRY(flags_check(what, flags));
    if (count && (!v || !out)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    if (device) return PHX_OK;
    for (int k = 0; k < count; ++k) {
        const float* q = v + (size_t)r.width * k;
        for (int c = 0; c < r.width; ++c)
            if (!std::isfinite(q[c])) { set_error("%s: query %d: value %d is not finite", what, k, c); return PHX_ERR_INVALID; }
        if (r.ordered && !(q[0] <= q[2] && q[1] <= q[3])) { set_error("%s: box %d: min exceeds max", what, k); return PHX_ERR_INVALID; }
        if (r.half >= 0 && !(q[r.half] > 0.f && q[r.half + 1] > 0.f)) { set_error("%s: box %d: half extents must be positive", what, k); return PHX_ERR_INVALID; }
        if (r.radius >= 0 && !(q[r.radius] > 0.f)) { set_error("%s: circle %d: the radius must be positive", what, k); return PHX_ERR_INVALID; }
        if (r.max_t >= 0 && !(q[r.max_t] >= 0.f)) { set_error("%s: %s %d: max_t < 0", what, r.noun, k); return PHX_ERR_INVALID; }
        if (r.max_dist >= 0 && !(q[r.max_dist] >= 0.f)) { set_error("%s: %s %d: max_dist < 0", what, r.noun, k); return PHX_ERR_INVALID; }
        if (r.dir >= 0 && q[r.dir] == 0.f && q[r.dir + 1] == 0.f) { set_error("%s: %s %d: zero direction", what, r.noun, k); return PHX_ERR_INVALID; }
    }
    return PHX_OK;
}

int World::query_prepare(bool host_wait)
{
    if (host_wait) return settle_and_upload();                              // (an unverified solve is settled before its results are read)
    PHX_TRY(settle_on_device());
    return sync_bodies_to_device();                                         // (host-staged bodies go up as the next step would take them)
}

// one result per query, to the host: check, prepare, `miss` for every query of an empty world, stage, reserve, run, read back
template <class Hit>
int World::query_rows(const char* what, const float* rows, int count, QueryRows kind, int flags, Hit* out, const Hit& miss, DevBuf<Hit>& buf, QueryRun<Hit> run)
{
    const RowRule& rule = ROW_RULES[kind];
    PHX_TRY(query_check(what, rows, count, rule, flags, false, out));
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(true));
    if (!nb()) { std::fill(out, out + count, miss); return PHX_OK; }
    const float* d_rows = nullptr;
    PHX_TRY(stage_.values(rows, count, rule.width, stream_, &d_rows));
    PHX_TRY(buf.reserve((size_t)count));
    PHX_TRY((query_.*run)(query_view(), nb(), geom_epoch_, d_rows, count, flags, buf.p, stream_));
    PHX_TRY(rb_.add(out, buf.p, (size_t)count * sizeof(Hit), stream_));
    return rb_.wait(stream_);
}

// ... on caller-owned device memory: only queued
template <class Hit>
int World::query_rows_device(const char* what, const void* d_rows, int count, QueryRows kind, int flags, void* d_out, QueryRun<Hit> run)
{
    PHX_TRY(query_check(what, static_cast<const float*>(d_rows), count, ROW_RULES[kind], flags, true, d_out));
    if (count && ((reinterpret_cast<uintptr_t>(d_rows) | reinterpret_cast<uintptr_t>(d_out)) & 3u)) { set_error("%s: the arrays must be 4-byte aligned", what); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(query_prepare(false));
    return (query_.*run)(query_view(), nb(), geom_epoch_, static_cast<const float*>(d_rows), count, flags, static_cast<Hit*>(d_out), stream_);
}

// the overlap lists (offsets, ascending hits, total): DeviceQuery waits for them itself
int World::query_overlaps(const char* what, const float* boxes, int count, QueryRows kind, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total, OverlapRun run)
{
    const RowRule& rule = ROW_RULES[kind];
    PHX_TRY(query_check(what, boxes, count, rule, flags, false, boxes));
    if (!offsets || !total) { set_error("%s: null offsets / total", what); return PHX_ERR_INVALID; }
    if (hit_cap < 0 || (hit_cap > 0 && !hits)) { set_error("%s: bad hits buffer (cap %d)", what, hit_cap); return PHX_ERR_INVALID; }
    PHX_TRY(query_prepare(true));
    const float* d_boxes = nullptr;
    if (count && nb()) PHX_TRY(stage_.values(boxes, count, rule.width, stream_, &d_boxes));
    return (query_.*run)(query_view(), nb(), geom_epoch_, d_boxes, count, flags, offsets, hits, hit_cap, total, rb_, stream_);
}

static const phx_ray_hit RAY_MISS = {-1, 0.f, {0.f, 0.f}, {0.f, 0.f}};      // (include/phyx_amd.h: no hit: body -1, every other field 0)
static const phx_shape_hit SHAPE_MISS = {-1, 0.f, {0.f, 0.f}};
static const phx_near_hit NEAR_MISS = {-1, 0.f, {0.f, 0.f}, {0.f, 0.f}};

int World::query_aabb(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total)
{
    return query_overlaps("phx_world_query_aabb", boxes, count, ROWS_BOXES, flags, offsets, hits, hit_cap, total, &DeviceQuery::aabb);
}
int World::query_boxes(const float* boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total)
{
    return query_overlaps("phx_world_query_boxes", boxes, count, ROWS_SHAPES, flags, offsets, hits, hit_cap, total, &DeviceQuery::shapes);
}
int World::query_circles(const float* circles, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap, int64_t* total)
{
    return query_overlaps("phx_world_query_circles", circles, count, ROWS_CIRCLES, flags, offsets, hits, hit_cap, total, &DeviceQuery::discs);
}
int World::query_points(const float* points, int count, int flags, int32_t* body) { return query_rows<int>("phx_world_query_points", points, count, ROWS_POINTS, flags, body, -1, q_body_, &DeviceQuery::points); }
int World::raycast(const float* rays, int count, int flags, phx_ray_hit* out) { return query_rows("phx_world_raycast", rays, count, ROWS_RAYS, flags, out, RAY_MISS, q_hits_, &DeviceQuery::rays); }
int World::cast_boxes(const float* casts, int count, int flags, phx_shape_hit* out) { return query_rows("phx_world_cast_boxes", casts, count, ROWS_CASTS, flags, out, SHAPE_MISS, q_shape_hits_, &DeviceQuery::casts); }
int World::cast_circles(const float* casts, int count, int flags, phx_shape_hit* out) { return query_rows("phx_world_cast_circles", casts, count, ROWS_CIRCLE_CASTS, flags, out, SHAPE_MISS, q_shape_hits_, &DeviceQuery::disc_casts); }
int World::query_nearest(const float* queries, int count, int flags, phx_near_hit* out) { return query_rows("phx_world_query_nearest", queries, count, ROWS_NEAR, flags, out, NEAR_MISS, q_near_hits_, &DeviceQuery::near); }
int World::query_points_device(const void* d_points, int count, int flags, void* d_body) { return query_rows_device<int>("phx_world_query_points_device", d_points, count, ROWS_POINTS, flags, d_body, &DeviceQuery::points); }
int World::raycast_device(const void* d_rays, int count, int flags, void* d_out) { return query_rows_device<phx_ray_hit>("phx_world_raycast_device", d_rays, count, ROWS_RAYS, flags, d_out, &DeviceQuery::rays); }
int World::cast_boxes_device(const void* d_casts, int count, int flags, void* d_out) { return query_rows_device<phx_shape_hit>("phx_world_cast_boxes_device", d_casts, count, ROWS_CASTS, flags, d_out, &DeviceQuery::casts); }
int World::cast_circles_device(const void* d_casts, int count, int flags, void* d_out) { return query_rows_device<phx_shape_hit>("phx_world_cast_circles_device", d_casts, count, ROWS_CIRCLE_CASTS, flags, d_out, &DeviceQuery::disc_casts); }
int World::query_nearest_device(const void* d_queries, int count, int flags, void* d_out) { return query_rows_device<phx_near_hit>("phx_world_query_nearest_device", d_queries, count, ROWS_NEAR, flags, d_out, &DeviceQuery::near); }

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
    PHX_TRY(refuse_mid_step(what));                                         // (first: it wins over every complaint about the arguments)
    PHX_TRY(flags_check(what, flags));
    if (!offsets || !total) { set_error("%s: null offsets / total", what); return PHX_ERR_INVALID; }
    if (cap < 0 || (cap > 0 && !out)) { set_error("%s: bad output buffer (cap %d)", what, cap); return PHX_ERR_INVALID; }
    PHX_TRY(check_batch(what, bodies, bodies, count, false));               // (count >= 0, indices in range; repeats allowed)
    PHX_TRY(query_prepare(true));                                           // (contact_prepare less the refusal made above)
    const int* d_bodies = nullptr;
    if (count && nm) PHX_TRY(stage_.indices(bodies, count, stream_, &d_bodies));
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
