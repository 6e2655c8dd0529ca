// sleep_kernels.h — the kernels of the sleep pass and of the wake by list (sleep.h; the definition: tests/sleep_spec.py).
// All grid-stride over bodies, manifolds or a unit list; the labels come from k_cc_compress_window / k_cc_compress
// (schedule_kernels.h) behind the linking launches here — the launch boundary between linking and compressing is what makes the
// eight XCDs' links visible to the walks.
#pragma once

#include "sleep.h"

namespace phx {

constexpr unsigned SLEEP_HAS_AWAKE = 1u, SLEEP_HAS_SLEEPER = 2u, SLEEP_STRUCK = 4u;

__device__ __forceinline__ bool sleep_dynamic(float4 m) { return m.x != 0.f || m.y != 0.f; }      // k_cc_init's test, negated

// 1. timers; parent[i] = mobile ? i : -1; the per-root words and the struck flags cleared; the changed count cleared
static __global__ void __launch_bounds__(256) k_sleep_begin(const float4* __restrict__ mpos, const float4* __restrict__ vel, SleepCell* __restrict__ cells, int n,
                                                            float lin2, float ang2, float dt, int* __restrict__ parent, unsigned char* __restrict__ skip,
                                                            unsigned char* __restrict__ struck, unsigned* __restrict__ root_bits, unsigned* __restrict__ root_timer,
                                                            unsigned* __restrict__ words)
{
    if (blockIdx.x == 0 && threadIdx.x == 0) words[SLEEP_CHANGED] = 0u;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const bool dynamic = sleep_dynamic(mpos[i]);
        const bool asleep = cells[i].asleep != 0;
        if (dynamic && !asleep) {
            const float4 v = vel[i];
            const float l = v.x * v.x + v.y * v.y, a = v.z * v.z;          // (products and sums round on their own: -ffp-contract=off)
            cells[i].timer = (l <= lin2 && a <= ang2) ? cells[i].timer + dt : 0.f;
        }
        const bool mobile = dynamic || asleep;
        parent[i] = mobile ? i : -1;
        skip[i] = mobile ? 0 : 1;
        struck[i] = 0;
        root_bits[i] = 0u;
        root_timer[i] = 0xFFFFFFFFu;
    }
}

// the wake by list: the graph is the sleepers' subgraph
static __global__ void __launch_bounds__(256) k_sleep_wake_begin(const SleepCell* __restrict__ cells, int n, int* __restrict__ parent, unsigned char* __restrict__ skip,
                                                                 unsigned* __restrict__ root_bits)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const bool asleep = cells[i].asleep != 0;
        parent[i] = asleep ? i : -1;
        skip[i] = asleep ? 0 : 1;
        root_bits[i] = 0u;
    }
}

// k_cc_link's linking step: the smaller root wins, whatever order the links run in
__device__ __forceinline__ void sleep_link(int* parent, unsigned u, unsigned v)
{
    int hi = (int)(u > v ? u : v), lo = (int)(u > v ? v : u);
    while (true) {
        const int old = atomicMin(parent + hi, lo);
        if (old == hi || old == lo) break;
        hi = old > lo ? old : lo; lo = old > lo ? lo : old;
    }
}

// 2. the manifolds' edges (point_count > 0, both bodies in the graph, neither a sensor) and the struck flags (`struck` null: the wake
// by list, which has none): a sleeper that shares such a manifold with a body outside the mobile set whose velocity has a nonzero word
static __global__ void __launch_bounds__(256) k_sleep_link_manifolds(const phx_manifold* __restrict__ manifolds, int nm, int nb, int* parent,
                                                                     const unsigned char* __restrict__ skip, const uint32_t* __restrict__ flags,
                                                                     unsigned char* __restrict__ struck, const SleepCell* __restrict__ cells, const float4* __restrict__ vel)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        if (m.point_count <= 0) continue;
        const unsigned u = (unsigned)m.body1, v = (unsigned)m.body2;
        if (u >= (unsigned)nb || v >= (unsigned)nb || u == v) continue;
        const bool su = skip[u] != 0, sv = skip[v] != 0;
        if (!su && !sv) {
            if (flags && ((flags[u] | flags[v]) & PHX_BODY_SENSOR)) continue;
            sleep_link(parent, u, v);
        } else if (struck && su != sv) {
            const unsigned in = su ? v : u, out = su ? u : v;                  // `out` is not mobile
            if (cells[in].asleep == 0) continue;
            const float4 w = vel[out];
            if ((__float_as_uint(w.x) | __float_as_uint(w.y) | __float_as_uint(w.z)) != 0u) struck[in] = 1;      // (every writer stores the same 1)
        }
    }
}

// ... and a unit list's: records of `stride` bytes that begin with body1, body2 (body2 == -1: the world, no edge)
static __global__ void __launch_bounds__(256) k_sleep_link_units(const char* __restrict__ records, int stride, int count, int nb, int* parent,
                                                                 const unsigned char* __restrict__ skip)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int2 b = *reinterpret_cast<const int2*>(records + (size_t)k * (size_t)stride);
        const unsigned u = (unsigned)b.x, v = (unsigned)b.y;
        if (u >= (unsigned)nb || v >= (unsigned)nb || u == v) continue;       // (body2 == -1 is out of range as an unsigned)
        if (skip[u] || skip[v]) continue;
        sleep_link(parent, u, v);
    }
}

// 4. per root: has-awake, has-sleeper, struck by atomicOr; the awake bodies' smallest timer by atomicMin on the float's bits (timers
// are >= 0, so their bits order as unsigned).  Same-address atomics are what this costs (2e5 of them on one word: milliseconds), so a
// wave first reduces the lanes that hang under one root — root by root, up to SLEEP_WAVE_ROOTS of them, which covers a wave that lies
// across the border of two piles — and its leader looks before it sends: the words only ever gain bits and lose value inside this
// launch, so a word that holds the wave's bits already, or a timer no larger than the wave's, needs no atomic, however old the
// value read is.  Or and min commute: the result does not depend on which waves sent theirs.
constexpr int SLEEP_WAVE_ROOTS = 4;
__device__ __forceinline__ void sleep_send(unsigned* __restrict__ root_bits, unsigned* __restrict__ root_timer, int r, unsigned bits, unsigned timer)
{
    if (bits && (__hip_atomic_load(&root_bits[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bits) != bits) atomicOr(&root_bits[r], bits);
    if (timer != 0xFFFFFFFFu && __hip_atomic_load(&root_timer[r], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) > timer) atomicMin(&root_timer[r], timer);
}
static __global__ void __launch_bounds__(256) k_sleep_reduce(const int* __restrict__ parent, const SleepCell* __restrict__ cells, const unsigned char* __restrict__ struck,
                                                             int n, unsigned* __restrict__ root_bits, unsigned* __restrict__ root_timer)
{
    const int lane = threadIdx.x & 63;
    const int rounds = (n + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);      // (whole waves stay together for the shuffles)
    for (int round = 0; round < rounds; ++round) {
        const int i = round * (int)(gridDim.x * blockDim.x) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
        int r = -1;
        unsigned bits = 0u, timer = 0xFFFFFFFFu;
        if (i < n) {
            r = parent[i];
            if (r >= 0) {
                const SleepCell c = cells[i];
                if (c.asleep) bits = SLEEP_HAS_SLEEPER | (struck[i] ? SLEEP_STRUCK : 0u);
                else { bits = SLEEP_HAS_AWAKE; timer = __float_as_uint(c.timer); }
            }
        }
        for (int pass = 0; pass < SLEEP_WAVE_ROOTS; ++pass) {
            // the root of the lowest lane that still has one to send (-1: nobody has)
            int first = r >= 0 ? lane : 64;
            for (int off = 32; off > 0; off >>= 1) first = min(first, __shfl_xor(first, off));
            if (first == 64) break;                                        // (uniform: every lane holds the same minimum)
            const int root = __shfl(r, first);
            const bool mine = r == root;
            unsigned b = mine ? bits : 0u, t = mine ? timer : 0xFFFFFFFFu;
            for (int off = 32; off > 0; off >>= 1) { b |= (unsigned)__shfl_xor((int)b, off); t = min(t, (unsigned)__shfl_xor((int)t, off)); }
            if (lane == first) sleep_send(root_bits, root_timer, root, b, t);
            if (mine) r = -1;
        }
        if (r >= 0) sleep_send(root_bits, root_timer, r, bits, timer);     // (a wave over many small components: distinct words)
    }
}

__device__ __forceinline__ void sleep_restore(int i, SleepCell& c, float4* __restrict__ mpos, phx_rigid_body* __restrict__ records)
{
    float4 m = mpos[i];
    m.x = c.inv_mass; m.y = c.inv_inertia;
    mpos[i] = m;
    records[i].inv_mass = m.x; records[i].inv_inertia = m.y;
    c.asleep = 0;
}

// the counts of a wave, reduced first: one atomic per wave and word
__device__ __forceinline__ void sleep_count(unsigned slept, unsigned woken, unsigned* __restrict__ words)
{
    for (int off = 32; off > 0; off >>= 1) { slept += __shfl_xor(slept, off); woken += __shfl_xor(woken, off); }
    if ((threadIdx.x & 63) != 0 || !(slept | woken)) return;
    atomicAdd(&words[SLEEP_CHANGED], slept + woken);
    if (slept) atomicAdd(reinterpret_cast<unsigned long long*>(words + SLEEP_SLEPT), (unsigned long long)slept);
    if (woken) atomicAdd(reinterpret_cast<unsigned long long*>(words + SLEEP_WOKEN), (unsigned long long)woken);
}

// 5. apply: a component with a sleeper and an awake body or a struck sleeper wakes (masses restored, every timer 0); one without a
// sleeper whose smallest timer has reached time_to_sleep sleeps (masses saved, then zeroed; velocities +0)
static __global__ void __launch_bounds__(256) k_sleep_apply(const int* __restrict__ parent, SleepCell* __restrict__ cells, int n, float4* __restrict__ mpos,
                                                            float4* __restrict__ vel, phx_rigid_body* __restrict__ records, const unsigned* __restrict__ root_bits,
                                                            const unsigned* __restrict__ root_timer, float time_to_sleep, unsigned* __restrict__ words)
{
    const int rounds = (n + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);
    for (int round = 0; round < rounds; ++round) {
        const int i = round * (int)(gridDim.x * blockDim.x) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
        unsigned slept = 0u, woken = 0u;
        const int r = i < n ? parent[i] : -1;
        if (r >= 0) {
            const unsigned bits = root_bits[r];
            if ((bits & SLEEP_HAS_SLEEPER) && (bits & (SLEEP_HAS_AWAKE | SLEEP_STRUCK))) {
                SleepCell c = cells[i];
                if (c.asleep) { sleep_restore(i, c, mpos, records); woken = 1u; }
                c.timer = 0.f;
                cells[i] = c;
            } else if (!(bits & SLEEP_HAS_SLEEPER) && __uint_as_float(root_timer[r]) >= time_to_sleep) {
                SleepCell c = cells[i];
                float4 m = mpos[i], v = vel[i];
                c.asleep = 1; c.inv_mass = m.x; c.inv_inertia = m.y;
                m.x = 0.f; m.y = 0.f;
                v.x = 0.f; v.y = 0.f; v.z = 0.f;
                cells[i] = c; mpos[i] = m; vel[i] = v;
                records[i].inv_mass = 0.f; records[i].inv_inertia = 0.f;
                slept = 1u;
            }
        }
        sleep_count(slept, woken, words);
    }
}

// the wake by list: the root of every named sleeper is marked (`keep` non-null: the named bodies are those whose word is 0) ...
static __global__ void __launch_bounds__(256) k_sleep_name(const int* __restrict__ list, int count, const unsigned* __restrict__ keep, int nb,
                                                           const int* __restrict__ parent, unsigned* __restrict__ root_bits)
{
    const int n = keep ? nb : count;
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < n; k += gridDim.x * blockDim.x) {
        if (keep && keep[k]) continue;
        const int b = keep ? k : list[k];
        if ((unsigned)b >= (unsigned)nb) continue;
        const int r = parent[b];
        if (r >= 0) root_bits[r] = 1u;                                         // (every writer stores the same 1)
    }
}

// ... and every sleeper under a marked root (`all`: every sleeper) wakes
static __global__ void __launch_bounds__(256) k_sleep_wake_apply(const int* __restrict__ parent, SleepCell* __restrict__ cells, int n, float4* __restrict__ mpos,
                                                                 phx_rigid_body* __restrict__ records, const unsigned* __restrict__ root_bits, int all,
                                                                 unsigned* __restrict__ words)
{
    const int rounds = (n + (int)(gridDim.x * blockDim.x) - 1) / (int)(gridDim.x * blockDim.x);
    for (int round = 0; round < rounds; ++round) {
        const int i = round * (int)(gridDim.x * blockDim.x) + (int)(blockIdx.x * blockDim.x + threadIdx.x);
        unsigned woken = 0u;
        if (i < n) {
            SleepCell c = cells[i];
            if (c.asleep && (all || (parent[i] >= 0 && root_bits[parent[i]]))) {
                sleep_restore(i, c, mpos, records);
                c.timer = 0.f;
                cells[i] = c;
                woken = 1u;
            }
        }
        sleep_count(0u, woken, words);
    }
}

static __global__ void __launch_bounds__(256) k_sleep_fill(SleepCell* __restrict__ cells, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) cells[i] = SleepColumn::initial();
}

// phx_world_get_sleep_states: the body's own masses whether asleep or not
static __global__ void __launch_bounds__(256) k_sleep_states(const float4* __restrict__ mpos, const SleepCell* __restrict__ cells, int n, phx_sleep_state* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 m = mpos[i];
        const SleepCell c = cells ? cells[i] : SleepColumn::initial();
        phx_sleep_state s;
        s.asleep = c.asleep ? 1 : 0; s.timer = c.timer;
        s.inv_mass = c.asleep ? c.inv_mass : m.x; s.inv_inertia = c.asleep ? c.inv_inertia : m.y;
        out[i] = s;
    }
}

} // namespace phx
