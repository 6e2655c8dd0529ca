// world_kernels.h — the stages of World::Update that sit around the two hot halves, as HIP kernels, so that the
// whole step runs on HBM-resident arrays.
//
//   IntegrateVelocity / IntegratePosition        ref: src/World.cpp:39-70
//   manifold creation for new pairs              ref: src/Collider.cpp:313-316
//   UpdateManifolds (SAT + contact generation)   ref: src/Collider.cpp:368-377 -> narrowphase.h
//   PackManifolds                                ref: src/Collider.cpp:379-416
//   RefreshContactJoints                         ref: src/World.cpp:72-149
//
// The last two are written sequentially in the reference (swap-remove while scanning forward), and the ORDER they
// leave behind is semantics: joint order is solve order.  The parallel form reproduces that order exactly.  Scanning
// i upward and replacing every dead a[i] by the current last element (re-examining i) ends with: survivors count
// n' = n - dead; every dead position below n' (a "hole"), taken in ascending order, receives the live elements that
// sat at positions >= n' (the "movers"), taken in DESCENDING order; everything else stays where it was.
#pragma once

#include "common.h"
#include "narrowphase.h"
#include "sleep.h"
#include "pair_set.h"

namespace phx {

// ---- 128-byte records <-> the World's resident arrays (body_view.h record_to_world / world_record): upload after construction, download
// for the getters -------
static __global__ void __launch_bounds__(256) k_bodies_to_world(const phx_rigid_body* __restrict__ bodies, int n, WorldBodies w)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) record_to_world(bodies[i], w, i);
}

static __global__ void __launch_bounds__(256) k_world_to_bodies(WorldBodies w, int n, phx_rigid_body* __restrict__ bodies)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) world_record(w, i, bodies[i]);
}

// the records of the listed bodies only (phx_world_get_body_states): what k_world_to_bodies would leave in records[idx[k]]
static __global__ void __launch_bounds__(256) k_gather_bodies(WorldBodies w, const phx_rigid_body* __restrict__ records, const int* __restrict__ idx, int count,
                                                              phx_rigid_body* __restrict__ out)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        phx_rigid_body b = records[i];
        world_record(w, i, b);
        out[k] = b;
    }
}

// {pos.x, pos.y, xVector.x, xVector.y} of every body (phx_world_get_poses / _device)
static __global__ void __launch_bounds__(256) k_world_poses(WorldBodies w, int n, float4* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 m = w.s.mpos[i], f = w.frame[i];
        out[i] = make_float4(m.z, m.w, f.x, f.y);
    }
}

// ---- edits between steps (phx_world_add_accelerations / set_velocities / set_poses): one lane per listed body.  The host has
// checked that the indices are in range and distinct, so no two lanes touch the same body.
// `acceleration += a` (ref: main.cpp:343-346) on the pending accelerations the next IntegrateVelocity consumes (`accel`, zeroed by
// the first edit after a step), mirrored into the records so that the getters show it until that step (ref: World.cpp:50, 53)
static __global__ void __launch_bounds__(256) k_add_accelerations(const int* __restrict__ idx, const float* __restrict__ a, int count, float4* __restrict__ accel,
                                                                  phx_rigid_body* __restrict__ records)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        float4 s = accel[i];
        s.x += a[3 * k]; s.y += a[3 * k + 1]; s.z += a[3 * k + 2];
        accel[i] = s;
        records[i].acceleration.x = s.x; records[i].acceleration.y = s.y; records[i].angular_acceleration = s.z;
    }
}

// velocity = {v.x, v.y}, angularVelocity = v.z
static __global__ void __launch_bounds__(256) k_set_velocities(const int* __restrict__ idx, const float* __restrict__ v, int count, float4* __restrict__ vel)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        float4 o = vel[i];
        o.x = v[3 * k]; o.y = v[3 * k + 1]; o.z = v[3 * k + 2];
        vel[i] = o;
    }
}

// coords = {pos, xVector, yVector}, then UpdateGeom (ref: RigidBody.h:38-42, Geom.h:79-85): the frame is given, not an angle
static __global__ void __launch_bounds__(256) k_set_poses(const int* __restrict__ idx, const float* __restrict__ p, int count, WorldBodies w)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        const float* q = p + 6 * k;
        float4 m = w.s.mpos[i];
        m.z = q[0]; m.w = q[1];
        const float2 sz = w.size[i];
        float4 box;
        geom_aabb(v2(q[0], q[1]), v2(q[2], q[3]), v2(q[4], q[5]), v2(sz.x, sz.y), box.x, box.y, box.z, box.w);
        w.s.mpos[i] = m;
        w.frame[i] = make_float4(q[2], q[3], q[4], q[5]);
        w.aabb[i] = box;
    }
}

// body->invMass = v[0], body->invInertia = v[1] (phx_world_set_inverse_masses): the resident {invMass, invInertia} and the records,
// whose inverse masses are what the upload left there (world_record does not refresh them)
static __global__ void __launch_bounds__(256) k_set_inverse_masses(const int* __restrict__ idx, const float* __restrict__ v, int count, float4* __restrict__ mpos,
                                                                   phx_rigid_body* __restrict__ records)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        float4 m = mpos[i];
        m.x = v[2 * k]; m.y = v[2 * k + 1];
        mpos[i] = m;
        records[i].inv_mass = m.x; records[i].inv_inertia = m.y;
    }
}

// ---- the optional per-body columns ---------------------------------------------------------------------------------------------------
// A column holds one value per body and exists only once some body's value was set (world.h BodyTable); until then every body has
// the column's default and the step runs the kernels it always ran.  A column states its stored type, its default, and the conversions
// between the stored value and the C ABI's struct, which is also the form a batch is staged in.
struct FilterColumn {                  // include/phyx_amd.h COLLISION FILTERS; the rule: common.h collision_filter_pass
    using value = uint4;               // {category, mask, group, 0}
    using api = phx_collision_filter;
    static constexpr const char* plural = "collision filters";
    static __host__ __device__ value initial() { return make_uint4(FILTER_DEFAULT_CATEGORY, FILTER_DEFAULT_MASK, 0u, 0u); }
    static __host__ __device__ value stored(const api& f) { return make_uint4(f.category, f.mask, (unsigned)f.group, 0u); }
    static api shown(const value& v) { return api{v.x, v.y, (int32_t)v.z}; }
    static bool is_initial(const value& v) { return v.x == FILTER_DEFAULT_CATEGORY && v.y == FILTER_DEFAULT_MASK && v.z == 0u; }
};
struct MaterialColumn {                // include/phyx_amd.h MATERIALS; the pair rule: solver_kernels.h material_mu / material_e
    using value = float2;              // {friction, restitution}
    using api = phx_material;
    static constexpr const char* plural = "materials";
    static __host__ __device__ value initial() { return make_float2(MATERIAL_DEFAULT_FRICTION, MATERIAL_DEFAULT_RESTITUTION); }
    static __host__ __device__ value stored(const api& m) { return make_float2(m.friction, m.restitution); }
    static api shown(const value& v) { return api{v.x, v.y}; }
    static bool is_initial(const value& v) { return v.x == MATERIAL_DEFAULT_FRICTION && v.y == MATERIAL_DEFAULT_RESTITUTION; }
};
struct FlagsColumn {                   // include/phyx_amd.h BODY FLAGS / SENSORS; the rule: BodySensors below, in the joint match
    using value = uint32_t;            // PHX_BODY_* bits
    using api = uint32_t;
    static constexpr const char* plural = "body flags";
    static __host__ __device__ value initial() { return 0u; }
    static __host__ __device__ value stored(const api& f) { return f; }
    static api shown(const value& v) { return v; }
    static bool is_initial(const value& v) { return v == 0u; }
};
struct ShapeColumn {                   // include/phyx_amd.h SHAPES; the rule: narrowphase.h update_manifold, query_kernels.h
    using value = uint32_t;            // PHX_SHAPE_BOX, PHX_SHAPE_CIRCLE or PHX_SHAPE_CAPSULE (the size lives where it always did: the records and size[])
    using api = phx_shape;
    static constexpr const char* plural = "circles, capsules or polygons";
    static __host__ __device__ value initial() { return (uint32_t)PHX_SHAPE_BOX; }
    static __host__ __device__ value stored(const api& s) { return (uint32_t)s.kind; }
    static bool is_initial(const value& v) { return v == (uint32_t)PHX_SHAPE_BOX; }
    // (no `shown`: the getter joins the kind with the size, World::get_shapes)
};
struct PolygonColumn {                 // include/phyx_amd.h POLYGONS; the rule: narrowphase.h polygon_contact, query_kernels.h
    using value = PolyRec;             // {count, v[8], n[8]}: 132 B per body, paid only once some call named a polygon; count 0: not a polygon
    using api = phx_polygon;
    static constexpr const char* plural = "polygons";
    static __host__ __device__ value initial() { phx_polygon none = {}; return poly_record(none); }
    static __host__ __device__ value stored(const api& p) { return poly_record(p); }
    static api shown(const value& v)
    {
        api p = {};
        p.count = v.count;
        for (int k = 0; k < v.count; ++k) { p.v[k].x = v.v[2 * k]; p.v[k].y = v.v[2 * k + 1]; }
        return p;
    }
    static bool is_initial(const value& v) { return v.count == 0; }
};
struct SweepColumn {                   // include/phyx_amd.h CONTINUOUS BODIES; the rule: sweep_kernels.h k_sweep_bodies
    using value = float4;              // {rc, start.x, start.y, 0}: the core radius (0: a discrete body) and where the body stood before the step's integrator ran
    using api = float;                 // the core radius
    static constexpr const char* plural = "continuous bodies";
    static __host__ __device__ value initial() { return make_float4(0.f, 0.f, 0.f, 0.f); }
    static __host__ __device__ value stored(const api& rc) { return make_float4(rc, 0.f, 0.f, 0.f); }
    static api shown(const value& v) { return v.x; }
    static bool is_initial(const value& v) { return v.x == 0.f; }
};
static_assert(sizeof(phx_polygon) == 17 * sizeof(float), "a batch is staged as 4-byte words");
static_assert(sizeof(phx_collision_filter) == 3 * sizeof(float) && sizeof(phx_material) == 2 * sizeof(float) && sizeof(uint32_t) == sizeof(float) &&
              sizeof(phx_shape) == 3 * sizeof(float), "a batch is staged as 4-byte words");

// geom_size = {hx, hy} of the listed bodies (phx_world_set_shapes), then UpdateGeom's AABB as k_set_poses computes it: the resident size[]
// and aabb[], and the records, whose geom_size is what the upload left there (world_record does not refresh it).  The kinds go into
// their column by k_scatter_column<ShapeColumn>, where the column exists.
static __global__ void __launch_bounds__(256) k_set_shapes(const int* __restrict__ idx, const phx_shape* __restrict__ v, int count, WorldBodies w,
                                                           phx_rigid_body* __restrict__ records)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        const float4 m = w.s.mpos[i], f = w.frame[i];
        const V2 size = v2(v[k].hx, v[k].hy);
        float4 box;
        geom_aabb(v2(m.z, m.w), v2(f.x, f.y), v2(f.z, f.w), size, box.x, box.y, box.z, box.w);
        w.size[i] = make_float2(size.x, size.y);
        w.aabb[i] = box;
        records[i].geom_size = pv(size);
        records[i].aabb_min.x = box.x; records[i].aabb_min.y = box.y; records[i].aabb_max.x = box.z; records[i].aabb_max.y = box.w;
    }
}

// a column that becomes active is filled with its default, then the staged batch {indices | values} is scattered into it
template <class Column>
static __global__ void __launch_bounds__(256) k_fill_column(typename Column::value* __restrict__ column, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) column[i] = Column::initial();
}
template <class Column>
static __global__ void __launch_bounds__(256) k_scatter_column(const int* __restrict__ idx, const typename Column::api* __restrict__ v, int count,
                                                               typename Column::value* __restrict__ column)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) column[idx[k]] = Column::stored(v[k]);
}

// what the spawn and the removal move beside the records and the resident arrays: the pending accelerations (consumed by the next
// IntegrateVelocity) and the columns above.  Null = absent.  A new column (the shapes' kinds were the last) is one member here, one line in each of the two kernels, and its table in the World's
// each_table / columns() / spare_columns() (world.h), which is what fills the member.
struct BodyColumns {
    float4* accel;
    uint4* filters;
    float2* materials;
    uint32_t* flags;
    SleepCell* sleep;
    uint32_t* shapes;
    PolyRec* polygons;
    float4* sweep;
};

// spawn (phx_world_add_bodies): body first + k from row k = {pos, half size, invMass, invInertia, xVector, yVector}, which the host built
// as AddBody does (world.hip body_record); only the AABB is computed here, by the UpdateGeom of set_poses (ref: Geom.h:79-85).  The
// record is AddBody's byte for byte, the resident state has zero velocities, a pending acceleration slot starts at zero and every
// column that exists gets its default.
static __global__ void __launch_bounds__(256) k_spawn_bodies(const float* __restrict__ rows, int count, int first, WorldBodies w,
                                                             phx_rigid_body* __restrict__ records, BodyColumns cols)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const float* q = rows + 10 * (size_t)k;
        const int i = first + k;
        const V2 pos = v2(q[0], q[1]), size = v2(q[2], q[3]), xv = v2(q[6], q[7]), yv = v2(q[8], q[9]);
        float4 box;
        geom_aabb(pos, xv, yv, size, box.x, box.y, box.z, box.w);
        phx_rigid_body b = {};
        b.index = (uint32_t)i;
        b.geom_size = pv(size); b.geom_xvector = pv(xv); b.geom_yvector = pv(yv); b.geom_pos = pv(pos);
        b.aabb_min.x = box.x; b.aabb_min.y = box.y; b.aabb_max.x = box.z; b.aabb_max.y = box.w;
        b.inv_mass = q[4]; b.inv_inertia = q[5];
        b.xvector = pv(xv); b.yvector = pv(yv); b.pos = pv(pos);
        records[i] = b;
        w.s.vel[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.s.dvel[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.s.mpos[i] = make_float4(q[4], q[5], pos.x, pos.y);
        w.frame[i] = make_float4(xv.x, xv.y, yv.x, yv.y);
        w.aabb[i] = box;
        w.size[i] = make_float2(size.x, size.y);
        if (cols.accel) cols.accel[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        if (cols.filters) cols.filters[i] = FilterColumn::initial();
        if (cols.materials) cols.materials[i] = MaterialColumn::initial();
        if (cols.flags) cols.flags[i] = FlagsColumn::initial();
        if (cols.sleep) cols.sleep[i] = SleepColumn::initial();      // (awake, timer 0)
        if (cols.shapes) cols.shapes[i] = ShapeColumn::initial();    // (a box)
        if (cols.polygons) cols.polygons[i] = PolygonColumn::initial();
        if (cols.sweep) cols.sweep[i] = SweepColumn::initial();      // (a discrete body)
    }
}

// IntegrateVelocity (ref: World.cpp:39-55).  The reference zeroes both accelerations at the end of every IntegrateVelocity
// (World.cpp:49-52) and nothing on the path sets them, so the resident world carries no acceleration arrays: they are zero
// whenever this runs — except in the FIRST step after an upload of records that came with accelerations (phx_world_set_state /
// set_bodies of a foreign or handed-over state): `accel` = {acceleration.x, .y, angularAcceleration} per body for that one step,
// null otherwise.  The arithmetic is body_view.h integrate_velocity, which a broadphase update's first kernel takes along instead
// whenever the World lets it (broadphase.h StepPrologue).
// (first kernel of a step: it also clears the step's four counters)
static __global__ void __launch_bounds__(256) k_integrate_velocity(float4* __restrict__ vel, const float4* __restrict__ mpos, int n, float gravity, float dt,
                                                                   unsigned* __restrict__ counters, const float4* __restrict__ accel)
{
    if (blockIdx.x == 0 && threadIdx.x < 8) counters[threadIdx.x] = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        vel[i] = integrate_velocity(vel[i], accel ? accel[i] : make_float4(0.f, 0.f, 0.f, 0.f), mpos[i].x, gravity, dt);
}

// the records' accelerations once IntegrateVelocity has consumed them (ref: World.cpp:50, 53)
static __global__ void __launch_bounds__(256) k_clear_accelerations(phx_rigid_body* __restrict__ bodies, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        bodies[i].acceleration.x = 0.f; bodies[i].acceleration.y = 0.f; bodies[i].angular_acceleration = 0.f;
    }
}

// Vector2::Rotate (ref: Vector2.h:48-56); the reference's unqualified cos/sin resolve to the double overloads
__device__ __forceinline__ void rotate_vec(float& vx, float& vy, float c, float s)
{
    const V2 x = v2(vx, vy), y = perp(x);
    const V2 delta = (x * c + y * s) - x;
    vx = vx + delta.x; vy = vy + delta.y;
}

// IntegratePosition (ref: World.cpp:57-70) on the resident arrays: reads 72 bytes per body, writes 64.
// `gate` (may be null): the control word of the solve queued in front; if it differs from `expected` that solve
// committed nothing (stale or spoiled schedule, solver.hip) and neither does this — the host repeats both.
// `ride`: the settle's mailbox post, taken along by the first workgroup (common.h post_mail_block) — before the gate: the settle reads it.
static __global__ void __launch_bounds__(256) k_integrate_position(WorldBodies w, int n, float dt,
                                                                   const unsigned long long* __restrict__ gate, unsigned long long expected, MailRide ride)
{
    if (ride.args.count && blockIdx.x == 0) post_mail_block(ride.args, ride.host_words, ride.host_seq);
    if (gate && *gate != expected) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 v = w.s.vel[i], d = w.s.dvel[i];
        float4 m = w.s.mpos[i], f = w.frame[i];
        const float2 sz = w.size[i];
        m.z += d.x + v.x * dt;
        m.w += d.y + v.y * dt;
        const float ang = -(d.z + v.z * dt);
        const float c = (float)cos((double)ang), s = (float)sin((double)ang);
        rotate_vec(f.x, f.y, c, s);
        rotate_vec(f.z, f.w, c, s);
        float4 box;
        geom_aabb(v2(m.z, m.w), v2(f.x, f.y), v2(f.z, f.w), v2(sz.x, sz.y), box.x, box.y, box.z, box.w);
        w.s.mpos[i] = m;
        w.frame[i] = f;
        w.s.dvel[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        w.aabb[i] = box;
    }
}

// x-extent of the dynamic bodies' AABBs (ownership-sharded worlds, dist.py: a rank's bodies must stay inside its slab): the floats
// are kept as order-preserving unsigned keys so that atomicMin / atomicMax work; out[0] = min key, out[1] = max key
__device__ __forceinline__ unsigned float_key(float f) { const unsigned u = __float_as_uint(f); return (u & 0x80000000u) ? ~u : (u | 0x80000000u); }
static __global__ void __launch_bounds__(256) k_x_extent(WorldBodies w, int n, unsigned* __restrict__ out)
{
    unsigned lo = 0xFFFFFFFFu, hi = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 m = w.s.mpos[i];
        if (m.x == 0.f && m.y == 0.f) continue;                            // static bodies belong to every slab
        const float4 a = w.aabb[i];
        lo = min(lo, float_key(a.x)); hi = max(hi, float_key(a.z));
    }
    for (int off = 32; off > 0; off >>= 1) { lo = min(lo, (unsigned)__shfl_down(lo, off)); hi = max(hi, (unsigned)__shfl_down(hi, off)); }
    if ((threadIdx.x & 63) == 0) { if (lo != 0xFFFFFFFFu) atomicMin(&out[0], lo); if (hi) atomicMax(&out[1], hi); }
}

// The bodies' kinds (include/phyx_amd.h SHAPES) are a parameter of UpdateManifolds' kernel: AllBoxes (a world without an active shape
// column) gives the constant PHX_SHAPE_BOX, so update_manifold's dispatch folds away and the kernel is the box/box code it always was;
// BodyShapes reads one 4-byte word per body and knows boxes and circles; BodyCapsules (a world in which some call named a capsule) reads
// the same word and compiles the capsule routines in, so that they cost a circle world no register; BodyPolygons (a world in which some
// call named a polygon) carries the polygon column's pointer too and is the only one in which NpBody::poly is set or read.
struct AllBoxes {
    static constexpr bool capsules = false, polygons = false;
    __device__ unsigned operator()(int) const { return (unsigned)PHX_SHAPE_BOX; }
    __device__ const PolyRec* poly(int) const { return nullptr; }
};
struct BodyShapes {
    static constexpr bool capsules = false, polygons = false;
    const uint32_t* kind;              // per body (ShapeColumn)
    __device__ unsigned operator()(int i) const { return kind[i]; }
    __device__ const PolyRec* poly(int) const { return nullptr; }
};
struct BodyCapsules {
    static constexpr bool capsules = true, polygons = false;
    const uint32_t* kind;
    __device__ unsigned operator()(int i) const { return kind[i]; }
    __device__ const PolyRec* poly(int) const { return nullptr; }
};
struct BodyPolygons {
    static constexpr bool capsules = true, polygons = true;
    const uint32_t* kind;
    const PolyRec* polys;              // per body (PolygonColumn)
    __device__ unsigned operator()(int i) const { return kind[i]; }
    __device__ const PolyRec* poly(int i) const { return polys + i; }
};

template <class Shapes>
__device__ __forceinline__ NpBody np_load(const WorldBodies& w, int i, const Shapes& shapes)
{
    const float4 m = w.s.mpos[i], f = w.frame[i];
    const float2 sz = w.size[i];
    NpBody b;
    b.pos = v2(m.z, m.w); b.xv = v2(f.x, f.y); b.yv = v2(f.z, f.w); b.size = v2(sz.x, sz.y);
    b.kind = shapes(i);
    b.poly = shapes.poly(i);
    return b;
}

// ref: Collider.cpp:368-377; also flags the manifolds PackManifolds will drop (ref: Collider.cpp:387).
// Manifolds [nm_old, nm) are the pairs UpdatePairs has just found (ref: Collider.cpp:313-316 — Manifold(index_i, index_j,
// manifolds.size * kMaxContactPoints), contact slots blank): they are created here, in the lane that updates them, instead of
// by an append kernel of their own in front of this one.
template <class Shapes>
static __global__ void __launch_bounds__(256) k_update_manifolds(phx_manifold* __restrict__ manifolds, int nm, WorldBodies bodies,
                                                                 phx_contact_point* __restrict__ cps, unsigned* __restrict__ dead, int* __restrict__ dropped,
                                                                 int nm_old, const uint2* __restrict__ new_pairs, int first, unsigned* __restrict__ dead_count,
                                                                 MailRide ride, Shapes shapes)
{
    // (`ride`: the broadphase's new-pair count goes to the host with this launch's first workgroup — common.h post_mail_block)
    if (ride.args.count && blockIdx.x == 0) post_mail_block(ride.args, ride.host_words, ride.host_seq);
    // (`dead_count`: the step's dead-manifold counter, world.hip — dead manifolds are rare, and a count taken here lets PackManifolds'
    //  scan over all manifolds run only in the steps that have one)
    // (`first`: manifolds [first, nm) — the old manifolds are updated while the host waits for the new-pair count, the new ones
    //  in a launch of their own once it is known, world.hip)
    for (int i = first + blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        phx_manifold m;
        if (i >= nm_old) {
            const uint2 pr = new_pairs[i - nm_old];
            m.body1 = (int)pr.x; m.body2 = (int)pr.y; m.point_count = 0; m.point_index = 2 * i;
            phx_contact_point blank;
            blank.delta1.x = blank.delta1.y = blank.delta2.x = blank.delta2.y = blank.normal.x = blank.normal.y = 0.f;
            blank.is_merged = 0; blank.is_newly_created = 0; blank.pad_[0] = 0; blank.pad_[1] = 0; blank.solver_index = -1;
            cps[2 * i] = blank; cps[2 * i + 1] = blank;
        } else m = manifolds[i];
        // (two bodies = 2 x 40 bytes of the resident arrays; the 128-byte records cost 2 x 128 for the same fields)
        const NpBody b1 = np_load(bodies, m.body1, shapes), b2 = np_load(bodies, m.body2, shapes);
        if (update_manifold<Shapes::capsules, Shapes::polygons>(m, b1, b2, cps + m.point_index)) atomicAdd(dropped, 1);
        manifolds[i] = m;
        const bool gone = m.point_count == 0 && !aabb_intersects(bodies.aabb[m.body1], bodies.aabb[m.body2]);
        dead[i] = gone ? 1u : 0u;
        if (gone) atomicAdd(dead_count, 1u);
    }
}

// ---- hole-filling compaction ---------------------------------------------------------------------------
// dead_before = exclusive scan of the dead flags; D = total dead; n' = n - D.
// mover_pos[r] = position of the r-th live element counted from the end (only those at positions >= n').
// (`n_flagged`: dead_before[] covers positions [0, n_flagged); positions beyond it were appended after the flags were
//  taken — new joints — and are alive, with every dead element before them)
__device__ __forceinline__ void compact_movers(int block, int blocks, const unsigned* __restrict__ dead_before, const unsigned* __restrict__ dead_total,
                                               int n, int n_flagged, int* __restrict__ mover_pos)
{
    const int D = (int)*dead_total, live = n - D;
    for (int p = live + block * (int)blockDim.x + (int)threadIdx.x; p < n; p += blocks * (int)blockDim.x) {
        const int here = p < n_flagged ? (int)dead_before[p] : D;
        const int next = (p + 1 < n_flagged) ? (int)dead_before[p + 1] : D;
        if (next != here) continue;                                      // p itself is dead
        const int dead_after = D - here;
        mover_pos[(n - 1 - p) - dead_after] = p;
    }
}

static __global__ void __launch_bounds__(256) k_compact_movers(const unsigned* __restrict__ dead_before, const unsigned* __restrict__ dead_total,
                                                               int n, int n_flagged, int* __restrict__ mover_pos)
{
    compact_movers((int)blockIdx.x, (int)gridDim.x, dead_before, dead_total, n, n_flagged, mover_pos);
}

// ref: Collider.cpp:385-410.  Every dead manifold's pair is listed for removal from the pair set; holes take movers.
static __global__ void __launch_bounds__(256) k_pack_manifolds(phx_manifold* __restrict__ manifolds, phx_contact_point* __restrict__ cps, int nm,
                                                               const unsigned* __restrict__ dead_before, const unsigned* __restrict__ dead_total,
                                                               const int* __restrict__ mover_pos, uint2* __restrict__ erased)
{
    const int D = (int)*dead_total, live = nm - D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const int h = (int)dead_before[i];
        const int next = (i + 1 < nm) ? (int)dead_before[i + 1] : D;
        if (next == h) continue;                                          // live: stays
        const phx_manifold gone = manifolds[i];
        erased[h] = make_uint2((unsigned)gone.body1, (unsigned)gone.body2);
        if (i >= live) continue;                                          // dead in the tail: just dropped
        const phx_manifold me = manifolds[mover_pos[h]];
        for (int k = 0; k < me.point_count; ++k) cps[2 * i + k] = cps[me.point_index + k];
        phx_manifold m = me;
        m.point_index = 2 * i;
        manifolds[i] = m;
    }
}

// ---- RefreshContactJoints (ref: World.cpp:72-149) -----------------------------------------------------------
// The reference resets every joint's contact point, lets the live points re-attach theirs and deletes what stayed reset.
// Here a joint is alive iff its `seen` stamp carries this step's epoch (no reset pass), and the dead-joint flags are the LOADER
// of their scan (device_scan.h) instead of a kernel of their own.
// Match, pass 1: matched points re-attach their joint and stamp it; count the points that need a new joint.  (A kernel of its
// own: as the loader of its scan it was slower — 25 us against 9 + 5 at 2e5 manifolds, 112 us at 1e6: a scan workgroup is 1024
// lanes of four items each, too few lanes in flight for this chain of dependent gathers.)
//
// Sensors (include/phyx_amd.h BODY FLAGS / SENSORS): a manifold one of whose bodies has PHX_BODY_SENSOR keeps its contact points and gets
// no joints.  The match writes -1 into its live slots and counts no fresh point there, so a joint it had stays unstamped and the clean-up
// deletes it as it deletes any dead joint; the create pass skips it.  The rule is a parameter of the two kernels: NoSensors (a world
// without an active flags column) is the code these kernels always were, BodySensors reads two 4-byte flag words per manifold.
struct NoSensors {
    static constexpr bool active = false;
    using cps_pointer = const phx_contact_point*;
    __device__ bool operator()(const phx_manifold&) const { return false; }
};
struct BodySensors {
    static constexpr bool active = true;
    using cps_pointer = phx_contact_point*;
    const uint32_t* flags;             // per body (FlagsColumn)
    __device__ bool operator()(const phx_manifold& m) const { return ((flags[m.body1] | flags[m.body2]) & PHX_BODY_SENSOR) != 0u; }
};

template <class Sensors>
static __global__ void __launch_bounds__(256) k_joints_match(const phx_manifold* __restrict__ manifolds, int nm, typename Sensors::cps_pointer __restrict__ cps,
                                                             phx_contact_joint* __restrict__ joints, unsigned* __restrict__ seen, unsigned epoch,
                                                             unsigned* __restrict__ new_count, Sensors sensors)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        unsigned fresh = 0;
        if constexpr (Sensors::active) {
            if (sensors(m)) {
                for (int k = 0; k < m.point_count; ++k) cps[m.point_index + k].solver_index = -1;
                new_count[i] = 0u;
                continue;
            }
        }
        for (int k = 0; k < m.point_count; ++k) {
            const int si = cps[m.point_index + k].solver_index;
            if (si < 0) ++fresh;
            else { joints[si].contact_point_index = m.point_index + k; seen[si] = epoch; }
        }
        new_count[i] = fresh;
    }
}

// loader of the 'dead joints before joint i' scan (queued behind the match)
struct JointDeadLoad {
    static constexpr bool in_place = false;
    const unsigned* seen; unsigned epoch;
    __device__ unsigned operator()(int i) const { return seen[i] != epoch ? 1u : 0u; }
    __device__ bool load4(int base, uint4& out) const      // (base is a multiple of four: device_scan.h; a dead joint is the rare case)
    {
        if (reinterpret_cast<uintptr_t>(seen) & 15u) return false;
        const uint4 s = *reinterpret_cast<const uint4*>(seen + base);
        if (s.x == epoch && s.y == epoch && s.z == epoch && s.w == epoch) { out = make_uint4(0u, 0u, 0u, 0u); return true; }
        out = make_uint4((*this)(base), (*this)(base + 1), (*this)(base + 2), (*this)(base + 3));
        return true;
    }
};

// Match, pass 2: new joints appended in manifold order, then point order (ref: World.cpp:108-114)
// (the movers of the clean-up behind it do not depend on the new joints: when there are dead joints too, the last `mover_blocks`
//  workgroups of the same launch compute them — one dispatch instead of two)
template <class Sensors>
static __global__ void __launch_bounds__(256) k_joints_create(const phx_manifold* __restrict__ manifolds, int nm, phx_contact_point* __restrict__ cps,
                                                              phx_contact_joint* __restrict__ joints, int nj_old, const unsigned* __restrict__ new_before,
                                                              int mover_blocks, const unsigned* __restrict__ dead_before, const unsigned* __restrict__ dead_total,
                                                              int total, int* __restrict__ mover_pos, Sensors sensors)
{
    const int create_blocks = (int)gridDim.x - mover_blocks;
    if ((int)blockIdx.x >= create_blocks) {
        compact_movers((int)blockIdx.x - create_blocks, mover_blocks, dead_before, dead_total, total, nj_old, mover_pos);
        return;
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += create_blocks * blockDim.x) {
        const phx_manifold m = manifolds[i];
        if (sensors(m)) continue;                                         // (its slots are -1 and stay so)
        int at = nj_old + (int)new_before[i];
        for (int k = 0; k < m.point_count; ++k) {
            phx_contact_point& cp = cps[m.point_index + k];
            if (cp.solver_index >= 0) continue;
            cp.solver_index = at;
            phx_contact_joint j;
            j.contact_point_index = m.point_index + k; j.body1 = m.body1; j.body2 = m.body2;
            j.normal_accumulated_impulse = 0.f; j.friction_accumulated_impulse = 0.f;
            joints[at++] = j;
        }
    }
}

// Cleanup (ref: World.cpp:125-143): holes take movers
// (a joint that moves takes its contact point's back-pointer along, ref: World.cpp:139 — every other live joint's contact point
//  points at it already: the match re-attached it, or k_joints_create has just made it.  Rounds 1-3 rewrote all nj back-pointers
//  in a kernel of their own behind this one: 8 us at cfg 2, 24 us at cfg 4, for a few hundred moved joints.)
static __global__ void __launch_bounds__(256) k_joints_fill(phx_contact_joint* __restrict__ joints, int nj, int n_flagged, const unsigned* __restrict__ dead_before,
                                                            const unsigned* __restrict__ dead_total, const int* __restrict__ mover_pos,
                                                            phx_contact_point* __restrict__ cps)
{
    const int D = (int)*dead_total, live = nj - D;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < live; i += gridDim.x * blockDim.x) {
        if (i >= n_flagged) continue;                                     // appended after the flags were taken: alive
        const int h = (int)dead_before[i];
        const int next = (i + 1 < n_flagged) ? (int)dead_before[i + 1] : D;
        if (next == h) continue;
        const phx_contact_joint moved = joints[mover_pos[h]];
        joints[i] = moved;
        cps[moved.contact_point_index].solver_index = i;
    }
}

// ---- removal of bodies between steps (phx_world_remove_bodies / remove_outside) -----------------------------------------------
// The result is defined as what phx_world_set_state would make of the filtered state (include/phyx_amd.h): kept bodies, manifolds
// and joints stay in their old order, so every new position is an exclusive scan of keep flags.  keep[] holds one word per body;
// the manifold and joint flags are the LOADERS of their scans (device_scan.h), and the compaction kernels recompute them.  Every
// kernel is a grid-stride pass over the OLD counts, writing out of place into the world's spare buffers: nothing here needs a
// count from the host.

// keep[i] = 0 for the listed bodies (keep[] was filled with 1; the host has checked the indices: in range, each at most once)
static __global__ void __launch_bounds__(256) k_remove_listed(const int* __restrict__ idx, int count, unsigned* __restrict__ keep)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) keep[idx[k]] = 0u;
}

// keep[i] = body i's AABB overlaps the closed box {min.x, min.y, max.x, max.y} (a NaN AABB overlaps nothing)
static __global__ void __launch_bounds__(256) k_keep_inside(const float4* __restrict__ aabb, int n, float4 box, unsigned* __restrict__ keep)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = aabb[i];
        keep[i] = (a.x <= box.z && a.z >= box.x && a.y <= box.w && a.w >= box.y) ? 1u : 0u;
    }
}

// The compaction of the contact cache is shared by three callers, which differ in the KEEP PREDICATE: which manifolds stay, and where
// their bodies go.  A removal keeps a manifold iff both of its bodies are kept and renumbers bodies through new[]; a change of collision
// filters (phx_world_set_collision_filters) keeps it iff its pair passes the filters and leaves the bodies where they are.
struct BodiesKept {
    const unsigned* keep; const unsigned* bnew;
    __device__ bool operator()(const phx_manifold& m) const { return (keep[m.body1] & keep[m.body2]) != 0u; }
    __device__ int body(int b) const { return (int)bnew[b]; }
};
struct FilterKept {
    const uint4* filters;      // per body {category, mask, group, 0}
    __device__ bool operator()(const phx_manifold& m) const { return collision_filter_pass(filters[m.body1], filters[m.body2]); }
    __device__ int body(int b) const { return b; }
};
// ... and a new collision exclusion (phx_world_add_collision_exclusions) keeps it iff its pair is not in the set (exclusions.h)
struct ExclusionKept {
    const unsigned long long* table; unsigned mask;      // the exclusions' keys (pair_set.h)
    __device__ bool operator()(const phx_manifold& m) const { return !ps_contains(table, mask, ps_unordered_key((unsigned)m.body1, (unsigned)m.body2)); }
    __device__ int body(int b) const { return b; }
};

// loaders of the three scans: a body is kept by its flag, a manifold by the predicate, a joint iff its manifold is
struct BodyKeepLoad {
    static constexpr bool in_place = false;
    const unsigned* keep;
    __device__ unsigned operator()(int i) const { return keep[i]; }
    __device__ bool load4(int base, uint4& out) const
    {
        if (reinterpret_cast<uintptr_t>(keep) & 15u) return false;
        out = *reinterpret_cast<const uint4*>(keep + base);
        return true;
    }
};
template <class Keep> struct ManifoldKeepLoad {
    static constexpr bool in_place = false;
    const phx_manifold* manifolds; Keep kept;
    __device__ unsigned operator()(int i) const { return kept(manifolds[i]) ? 1u : 0u; }
};
template <class Keep> struct JointKeepLoad {
    static constexpr bool in_place = false;
    const phx_contact_joint* joints; const phx_manifold* manifolds; Keep kept;
    __device__ unsigned operator()(int j) const { return kept(manifolds[joints[j].contact_point_index >> 1]) ? 1u : 0u; }
};

// element i's flag from the exclusive scan of the flags (`total`: their sum)
__device__ __forceinline__ bool scanned_flag(const unsigned* __restrict__ before, const unsigned* __restrict__ total, int i, int n)
{
    return ((i + 1 < n) ? before[i + 1] : *total) != before[i];
}

// Bodies: kept record i goes to out[to], to = bnew[i], as one 128-byte line, with `index` = to; the resident arrays (and the pending
// accelerations) at `to` are made from it by the upload's own conversion (record_to_world), as phx_world_set_state would make them.
// `refresh` (the records are stale): the record is first brought up to date from the resident arrays (world_record), as the getter
// would.  remap[i] = to, or -1.  accel_nonzero counts the kept records with an acceleration (the upload's test, world.hip).  The columns
// that exist in `cols` move with the bodies into `out_cols` (whose accelerations, if pending, are made from the record).
static __global__ void __launch_bounds__(256) k_remove_bodies(const phx_rigid_body* __restrict__ records, WorldBodies w, int n, int refresh,
                                                              const unsigned* __restrict__ keep, const unsigned* __restrict__ bnew,
                                                              phx_rigid_body* __restrict__ out_records, WorldBodies out, int* __restrict__ remap,
                                                              unsigned* __restrict__ accel_nonzero, BodyColumns cols, BodyColumns out_cols)
{
    static_assert(sizeof(phx_rigid_body) == 8 * sizeof(float4), "a record is one 128-byte line");
    unsigned nonzero = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const int to = keep[i] ? (int)bnew[i] : -1;
        remap[i] = to;
        if (to < 0) continue;
        const float4* src = reinterpret_cast<const float4*>(records) + 8 * (size_t)i;
        float4 line[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) line[k] = src[k];
        phx_rigid_body b;
        __builtin_memcpy(&b, line, sizeof b);
        if (refresh) world_record(w, i, b);
        b.index = (uint32_t)to;
        __builtin_memcpy(line, &b, sizeof b);
        float4* dst = reinterpret_cast<float4*>(out_records) + 8 * (size_t)to;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = line[k];
        record_to_world(b, out, to);
        if (cols.filters) out_cols.filters[to] = cols.filters[i];
        if (cols.materials) out_cols.materials[to] = cols.materials[i];
        if (cols.flags) out_cols.flags[to] = cols.flags[i];
        if (cols.sleep) out_cols.sleep[to] = cols.sleep[i];
        if (cols.shapes) out_cols.shapes[to] = cols.shapes[i];
        if (cols.polygons) out_cols.polygons[to] = cols.polygons[i];
        if (cols.sweep) out_cols.sweep[to] = cols.sweep[i];
        if (out_cols.accel) {
            out_cols.accel[to] = make_float4(b.acceleration.x, b.acceleration.y, b.angular_acceleration, 0.f);
            if (b.acceleration.x != 0.f || b.acceleration.y != 0.f || b.angular_acceleration != 0.f) ++nonzero;
        }
    }
    for (int off = 32; off > 0; off >>= 1) nonzero += __shfl_down(nonzero, off);
    if ((threadIdx.x & 63) == 0 && nonzero) atomicAdd(accel_nonzero, nonzero);
}

// Manifolds with their two contact-point slots (32 bytes each, moved as two 16-byte halves): kept manifold i goes to to = mnew[i]
// with its bodies remapped and point_index = 2 * to; a live slot's solver_index follows its joint (-1 if the joint goes), a dead
// slot is copied as it is.  pairs[to] = the remapped body pair (the new broadphase pair set).
template <class Keep>
static __global__ void __launch_bounds__(256) k_remove_manifolds(const phx_manifold* __restrict__ manifolds, const phx_contact_point* __restrict__ cps, int nm,
                                                                 Keep kept, const unsigned* __restrict__ mnew, const unsigned* __restrict__ jnew,
                                                                 const unsigned* __restrict__ jtotal, int nj, phx_manifold* __restrict__ out_manifolds,
                                                                 phx_contact_point* __restrict__ out_cps, uint2* __restrict__ pairs)
{
    static_assert(sizeof(phx_contact_point) == 2 * sizeof(float4), "a contact point is two 16-byte halves");
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        if (!kept(m)) continue;
        const int to = (int)mnew[i];
        phx_manifold o;
        o.body1 = kept.body(m.body1); o.body2 = kept.body(m.body2); o.point_count = m.point_count; o.point_index = 2 * to;
        out_manifolds[to] = o;
        pairs[to] = make_uint2((unsigned)o.body1, (unsigned)o.body2);
        const float4* src = reinterpret_cast<const float4*>(cps) + 4 * (size_t)i;
        float4* dst = reinterpret_cast<float4*>(out_cps) + 4 * (size_t)to;
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            float4 half[2] = {src[2 * k], src[2 * k + 1]};
            if (k < m.point_count) {
                phx_contact_point cp;
                __builtin_memcpy(&cp, half, sizeof cp);
                const int si = cp.solver_index;
                if (si >= 0 && si < nj) cp.solver_index = scanned_flag(jnew, jtotal, si, nj) ? (int)jnew[si] : -1;
                __builtin_memcpy(half, &cp, sizeof cp);
            }
            dst[2 * k] = half[0]; dst[2 * k + 1] = half[1];
        }
    }
}

// Joints: kept joint j goes to jnew[j] with its bodies remapped and contact_point_index = 2 * (its manifold's new index) + old % 2;
// the warm-start impulses are unchanged
template <class Keep>
static __global__ void __launch_bounds__(256) k_remove_joints(const phx_contact_joint* __restrict__ joints, int nj, const phx_manifold* __restrict__ manifolds,
                                                              Keep kept, const unsigned* __restrict__ mnew, const unsigned* __restrict__ jnew,
                                                              phx_contact_joint* __restrict__ out)
{
    for (int j = blockIdx.x * blockDim.x + threadIdx.x; j < nj; j += gridDim.x * blockDim.x) {
        phx_contact_joint q = joints[j];
        const int mi = q.contact_point_index >> 1;
        if (!kept(manifolds[mi])) continue;
        q.contact_point_index = 2 * (int)mnew[mi] + (q.contact_point_index & 1);
        q.body1 = kept.body(q.body1); q.body2 = kept.body(q.body2);
        out[jnew[j]] = q;
    }
}

} // namespace phx
