// body_view.h — the RESIDENT layout of body state in HBM: structure of arrays, one 16-byte granule per
// body and array, so that every kernel of the step reads exactly the fields it needs with coalesced 16-byte loads.
//
// The reference keeps a 128-byte AoS RigidBody (ref: src/RigidBody.h:12-57) and stages a solver-side copy on every call
// (PrepareBodies / FinishBodies, ref: Solver.cpp:456-494: SolveBody {velocity, angularVelocity, lastIteration} and
// SolveBodyParams {invMass, invInertia, coords}).  Here that staged form IS the resident form: the World keeps bodies as
// the arrays below for the whole simulation, the solver reads and writes them in place, and the 128-byte records exist
// only at the C-ABI edge (phx_world_get_bodies, phx_solver_solve*: converted by the two kernels at the bottom).
//
//   vel[b]   = {velocity.x, velocity.y, angularVelocity, 0}                          solver in/out, integrators
//   dvel[b]  = {displacingVelocity.x, .y, displacingAngularVelocity, 0}              solver in/out, IntegratePosition
//   mpos[b]  = {invMass, invInertia, pos.x, pos.y}                                   solver in (ref SolveBodyParams), narrowphase
//   (World only)  frame[b] = {xVector.x, xVector.y, yVector.x, yVector.y},  aabb[b] = {min.x, min.y, max.x, max.y},
//                 size[b]  = {geom.size.x, geom.size.y}
#pragma once

#include "common.h"

namespace phx {

struct BodyView {
    float4* vel;
    float4* dvel;
    float4* mpos;
};

// a polygon body's stored record (include/phyx_amd.h POLYGONS; formed by narrowphase.h poly_record): the body-local vertices and the unit
// outward normal of each edge v_k -> v_(k+1), as {x, y} pairs; count 0: the body is no polygon
struct PolyRec { int32_t count; float v[2 * PHX_POLYGON_MAX_VERTICES]; float n[2 * PHX_POLYGON_MAX_VERTICES]; };      // {count, v[8], n[8]}: 33 words
static_assert(sizeof(PolyRec) == 132, "a polygon record is 33 words");

// everything the World keeps per body: the solver's view + frame, AABB and half size
struct WorldBodies {
    BodyView s;
    float4* frame;      // {xVector.x, xVector.y, yVector.x, yVector.y}
    float4* aabb;       // {min.x, min.y, max.x, max.y}
    float2* size;       // geom.size
    const struct SleepCell* sleep;      // the queries only (query_kernels.h q_static): the sleep column (sleep.h), null while sleeping is off and in every other view
    const uint32_t* kinds;              // the queries only (query_kernels.h q_circle): the shape column (world_kernels.h ShapeColumn), null while no body is a circle and in every other view
    const PolyRec* polys;        // the queries only: the polygon column (world_kernels.h PolygonColumn), null unless some call named a polygon: picks the kernels' polygon instantiations (query.hip)
    uint32_t capsules;                  // the queries only, read by the host alone: a kind may be PHX_SHAPE_CAPSULE, which picks the kernels' capsule instantiations (query.hip)
};

// IntegrateVelocity (ref: World.cpp:39-55) of one body: its vel granule after `dt` under `accel` = {acceleration.x, .y,
// angularAcceleration} (zero where the body carries none) and gravity, which only a body with an inverse mass (mpos.x) feels.  The
// statements keep the reference's form (x + 0 * dt is not x for x = -0).  Its users: k_integrate_velocity (world_kernels.h) and the two
// first kernels of a broadphase update that take the velocity step along, k_build_keys<true> and k_keys_buckets<true, *>.
__device__ __forceinline__ float4 integrate_velocity(float4 v, float4 accel, float inv_mass, float gravity, float dt)
{
    const float ax = accel.x, aa = accel.z;
    float ay = accel.y;
    if (inv_mass > 0.0f) ay += gravity;
    v.x += ax * dt; v.y += ay * dt;
    v.z += aa * dt;
    return v;
}

// 16-byte non-temporal store (results that nobody re-reads before the kernel ends: they should not wait in L2 for the
// end-of-kernel write-back)
typedef float f4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(float4* p, float x, float y, float z, float w)
{
    f4v v; v.x = x; v.y = y; v.z = z; v.w = w;
    __builtin_nontemporal_store(v, reinterpret_cast<f4v*>(p));
}

// ---- 128-byte records <-> everything the World keeps (world_kernels.h, snapshot_kernels.h) ------------------------
// the upload's conversion: body i's resident granules from its record
__device__ __forceinline__ void record_to_world(const phx_rigid_body& b, const WorldBodies& w, int i)
{
    w.s.vel[i] = make_float4(b.velocity.x, b.velocity.y, b.angular_velocity, 0.f);
    w.s.dvel[i] = make_float4(b.displacing_velocity.x, b.displacing_velocity.y, b.displacing_angular_velocity, 0.f);
    w.s.mpos[i] = make_float4(b.inv_mass, b.inv_inertia, b.pos.x, b.pos.y);
    w.frame[i] = make_float4(b.xvector.x, b.xvector.y, b.yvector.x, b.yvector.y);
    w.aabb[i] = make_float4(b.aabb_min.x, b.aabb_min.y, b.aabb_max.x, b.aabb_max.y);
    w.size[i] = make_float2(b.geom_size.x, b.geom_size.y);
}

// everything a step changes goes back into the records (inverse masses, size, index, the vestigial fields and the accelerations —
// zero after every IntegrateVelocity, ref: World.cpp:49-52, or what phx_world_add_accelerations left pending — are what the upload
// left there): body i's record `b` from the resident arrays
__device__ __forceinline__ void world_record(const WorldBodies& w, int i, phx_rigid_body& b)
{
    const float4 v = w.s.vel[i], d = w.s.dvel[i], m = w.s.mpos[i], f = w.frame[i], a = w.aabb[i];
    b.velocity.x = v.x; b.velocity.y = v.y; b.angular_velocity = v.z;
    b.displacing_velocity.x = d.x; b.displacing_velocity.y = d.y; b.displacing_angular_velocity = d.z;
    b.pos.x = m.z; b.pos.y = m.w;
    b.xvector.x = f.x; b.xvector.y = f.y; b.yvector.x = f.z; b.yvector.y = f.w;
    b.geom_xvector = b.xvector; b.geom_yvector = b.yvector; b.geom_pos = b.pos;      // UpdateGeom (ref: RigidBody.h:38-42)
    b.aabb_min.x = a.x; b.aabb_min.y = a.y; b.aabb_max.x = a.z; b.aabb_max.y = a.w;
}

// ---- the C-ABI edge: 128-byte records <-> resident arrays (solver fields only) ------------------------------------
// PrepareBodies (ref: Solver.cpp:456-480) for callers that hand over the reference's records
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_bodies_to_view(const phx_rigid_body* __restrict__ bodies, int n, BodyView out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const phx_rigid_body& b = bodies[i];
        out.vel[i] = make_float4(b.velocity.x, b.velocity.y, b.angular_velocity, 0.f);
        out.dvel[i] = make_float4(b.displacing_velocity.x, b.displacing_velocity.y, b.displacing_angular_velocity, 0.f);
        out.mpos[i] = make_float4(b.inv_mass, b.inv_inertia, b.pos.x, b.pos.y);
    }
}

// FinishBodies (ref: Solver.cpp:482-494): the four velocity fields back into the records.  `gate` (may be null): the control
// word of the solve queued in front; if it differs from `expected` that solve committed nothing and neither does this.
__attribute__((unused)) static __global__ void __launch_bounds__(256) k_view_to_bodies(BodyView in, int n, phx_rigid_body* __restrict__ bodies,
                                                               const unsigned long long* __restrict__ gate, unsigned long long expected)
{
    if (gate && *gate != expected) return;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 a = in.vel[i], d = in.dvel[i];
        phx_rigid_body& b = bodies[i];
        b.velocity.x = a.x; b.velocity.y = a.y; b.angular_velocity = a.z;
        b.displacing_velocity.x = d.x; b.displacing_velocity.y = d.y; b.displacing_angular_velocity = d.z;
    }
}

} // namespace phx
