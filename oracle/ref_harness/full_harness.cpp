// full_harness.cpp — extern "C" driver over the REAL reference World / Collider / Solver (the hot path's .cpp files).
//
// Test infrastructure.  oracle/Makefile's `ref_full` target builds this file together with World.cpp, Solver.cpp, Collider.cpp
// and base/WorkQueue.cpp AS THEY LIE, straight from $(REF)/src, whenever that tree exists.  Those files include
// "microprofile.h", a submodule the reference does not ship; ref_harness/profiler_off/microprofile.h, our own no-op header,
// stands in for it (it touches no program state; see there).  Two flavours land in the git-ignored oracle/_ref/: "strict"
// (the oracle's IEEE flags, bit-comparable) and "fast" (the reference's own flags, linked without crtfastmath so that loading
// it leaves the process's FTZ/DAZ bits alone).  oracle/_ref/ travels with the working tree to the GPU machine, where
// tests/test_reference_gpu.py loads it; nothing there reads the reference tree itself.
//
// Every step of World::Update (ref: World.cpp:19-37) is reachable through public members, so the harness can stop between
// the stages and hand out the solver's inputs, the grouping, and the outputs.  workers = 0 => deterministic.
//
// Pair paths.  World::Update with 0 workers takes Collider::UpdatePairsSerial, whose manifoldMap.insert can admit a pair
// that is already in the set when a tombstone lies ahead of it in the probe chain.  The reference's
// real configuration runs workers, hence UpdatePairsParallel, which filters with contains() (it walks the whole chain).
// The *_pairs entry points choose: PAIRS_SERIAL = 0 or PAIRS_PARALLEL = 1 (on the 0-worker queue: one buffer, body order).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <xmmintrin.h>

#include "World.h"
#include "Configuration.h"
#include "base/WorkQueue.h"

namespace {
struct Harness {
    World world;
    WorkQueue queue;
    int colliderMark;        // manifold count before the last reff_collider_update
    Harness() : queue(0), colliderMark(0) {}
};

// The reference's own program is linked with -ffast-math, so crtfastmath.o runs it with flush-to-zero and denormals-are-zero.
// The fast flavour (__FAST_MATH__) is linked without it, so as not to switch the loading process; instead every entry point that
// computes sets FTZ | DAZ for its own duration and puts the caller's MXCSR back on return.  The strict flavour leaves MXCSR alone.
struct FpEnv {
#ifdef __FAST_MATH__
    unsigned int saved;
    FpEnv() : saved(_mm_getcsr()) { _mm_setcsr(saved | 0x8040u); }
    ~FpEnv() { _mm_setcsr(saved); }
#endif
};

enum { PAIRS_SERIAL = 0, PAIRS_PARALLEL = 1 };

void update_pairs(Harness* h, int pairs)
{
    World& w = h->world;
    if (pairs == PAIRS_PARALLEL)
        w.collider.UpdatePairsParallel(h->queue, w.bodies.data, w.bodies.size);
    else
        w.collider.UpdatePairsSerial(w.bodies.data, w.bodies.size);
}

Configuration make_config(int solve_mode, int island_mode, int contact_iters, int penetration_iters)
{
    Configuration c;
    c.solveMode = (Configuration::SolveMode)solve_mode;
    c.islandMode = (Configuration::IslandMode)island_mode;
    c.contactIterationsCount = contact_iters;
    c.penetrationIterationsCount = penetration_iters;
    return c;
}

template <typename T>
int copy_out(const AlignedArray<T>& a, void* out, int cap_elements)
{
    if (out && cap_elements >= a.size && a.size > 0) memcpy(out, a.data, (size_t)a.size * sizeof(T));
    return a.size;
}
} // namespace

extern "C" {

void* reff_world_create(float gravity)
{
    Harness* h = new Harness();
    h->world.gravity = gravity;
    return h;
}

void reff_world_destroy(void* p) { delete static_cast<Harness*>(p); }

// World::AddBody (ref: World.cpp:11-17); is_static: main.cpp:91-93 (invMass = invInertia = 0)
int reff_world_add_body(void* p, float px, float py, float angle, float sx, float sy, int is_static)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    RigidBody* b = h->world.AddBody(Coords2f(Vector2f(px, py), angle), Vector2f(sx, sy));
    if (is_static) { b->invMass = 0.f; b->invInertia = 0.f; }
    return (int)b->index;
}

// a body pinned the way the reference's demo pins shelves: invMass = 0 only, its invInertia stays (ref: main.cpp:176-177)
void reff_world_pin_body(void* p, int index)
{
    Harness* h = static_cast<Harness*>(p);
    if (index >= 0 && index < (int)h->world.bodies.size) h->world.bodies[index].invMass = 0.f;
}

// move a body between steps the way the demo's code would: coords, then UpdateGeom (ref: RigidBody.h:38-42).
// frame6 = {pos.x, pos.y, xVector.x, xVector.y, yVector.x, yVector.y}
void reff_world_set_pose(void* p, int index, const float* frame6)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    if (index < 0 || index >= (int)h->world.bodies.size) return;
    RigidBody& b = h->world.bodies[index];
    b.coords.pos = Vector2f(frame6[0], frame6[1]);
    b.coords.xVector = Vector2f(frame6[2], frame6[3]);
    b.coords.yVector = Vector2f(frame6[4], frame6[5]);
    b.UpdateGeom();
}

// v3 = {velocity.x, velocity.y, angularVelocity}
void reff_world_set_velocity(void* p, int index, const float* v3)
{
    Harness* h = static_cast<Harness*>(p);
    if (index < 0 || index >= (int)h->world.bodies.size) return;
    RigidBody& b = h->world.bodies[index];
    b.velocity = Vector2f(v3[0], v3[1]);
    b.angularVelocity = v3[2];
}

// the whole step (ref: World.cpp:19-37), through World::Update itself (0 workers: the serial pair path)
void reff_world_update(void* p, float dt, int solve_mode, int island_mode, int contact_iters, int penetration_iters)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    h->world.Update(h->queue, dt, make_config(solve_mode, island_mode, contact_iters, penetration_iters));
}

// everything of World::Update that precedes Solver::SolveJoints (ref: World.cpp:25-32), pair path chosen by `pairs`
void reff_world_pre_solve_pairs(void* p, float dt, int pairs)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    World& w = h->world;
    w.IntegrateVelocity(h->queue, dt);
    w.collider.UpdateBroadphase(w.bodies.data, w.bodies.size);
    update_pairs(h, pairs);
    w.collider.UpdateManifolds(h->queue, w.bodies.data);
    w.collider.PackManifolds(w.bodies.data);
    w.RefreshContactJoints();
}

// World::Update's stages in its order, pair path chosen by `pairs` (PAIRS_SERIAL is the same step as reff_world_update)
void reff_world_update_pairs(void* p, float dt, int solve_mode, int island_mode, int contact_iters, int penetration_iters, int pairs)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    World& w = h->world;
    reff_world_pre_solve_pairs(p, dt, pairs);
    w.solver.SolveJoints(h->queue, w.bodies.data, w.bodies.size, w.collider.contactPoints.data, make_config(solve_mode, island_mode, contact_iters, penetration_iters));
    w.IntegratePosition(h->queue, dt);
}

// the serial pair path, as World::Update takes it with 0 workers
void reff_world_pre_solve(void* p, float dt) { reff_world_pre_solve_pairs(p, dt, PAIRS_SERIAL); }

// The collider alone over a caller's body array (only the AABBs are read): UpdateBroadphase, then the chosen pair path, into
// this harness's own Collider, whose pair set persists from call to call.  Returns the number of pairs the call added; they
// are the last entries of reff_manifolds, in emission order, and reff_broadphase_{sorted,entries} hold this call's sort.
int reff_collider_update(void* p, const void* bodies, int count, int pairs)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    Collider& c = h->world.collider;
    RigidBody* b = const_cast<RigidBody*>(static_cast<const RigidBody*>(bodies));
    h->colliderMark = c.manifolds.size;
    c.UpdateBroadphase(b, (size_t)count);
    if (pairs == PAIRS_PARALLEL)
        c.UpdatePairsParallel(h->queue, b, (size_t)count);
    else
        c.UpdatePairsSerial(b, (size_t)count);
    return c.manifolds.size - h->colliderMark;
}

// Solver::SolveJoints alone (ref: World.cpp:34)
void reff_world_solve(void* p, int solve_mode, int island_mode, int contact_iters, int penetration_iters)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    World& w = h->world;
    w.solver.SolveJoints(h->queue, w.bodies.data, w.bodies.size, w.collider.contactPoints.data, make_config(solve_mode, island_mode, contact_iters, penetration_iters));
}

void reff_world_integrate_position(void* p, float dt)
{
    FpEnv fp;
    Harness* h = static_cast<Harness*>(p);
    h->world.IntegratePosition(h->queue, dt);
}

// state getters: return the element count; copy when `out` holds at least that many elements
int reff_bodies(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.bodies, out, cap); }
int reff_manifolds(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.collider.manifolds, out, cap); }
int reff_contact_points(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.collider.contactPoints, out, cap); }
int reff_joints(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.solver.contactJoints, out, cap); }
int reff_joint_index(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.solver.joint_index, out, cap); }
int reff_island_offset(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.solver.island_offset, out, cap); }
int reff_island_size(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.solver.island_size, out, cap); }
int reff_broadphase_entries(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.collider.broadphase, out, cap); }
int reff_broadphase_sorted(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.collider.broadphaseSort[1], out, cap); }
int reff_solve_bodies_impulse(void* p, void* out, int cap) { return copy_out(static_cast<Harness*>(p)->world.solver.solveBodiesImpulse, out, cap); }
// the refreshed / solved joint blocks (ContactJointPacked<N>: 35 words per joint, AoSoA of N lanes)
int reff_joint_packed(void* p, int n, void* out, int cap)
{
    Solver& s = static_cast<Harness*>(p)->world.solver;
    return n == 8 ? copy_out(s.joint_packed8, out, cap) : n == 4 ? copy_out(s.joint_packed4, out, cap) : copy_out(s.joint_packed1, out, cap);
}
void reff_island_stats(void* p, int* count, int* max_size)
{
    Solver& s = static_cast<Harness*>(p)->world.solver;
    *count = s.islandCount; *max_size = s.islandMaxSize;
}

} // extern "C"
