// sweep_kernels.h — the device side of the continuous bodies' pass (include/phyx_amd.h CONTINUOUS BODIES; tests/sweep_spec.py is the
// definition, byte for byte).  A continuous body's core disc {start, rc} is cast along the translation d = pos - start that the step's
// IntegratePosition gave it, against every static body it collides with; the earliest entry puts the body back to the point of first
// touch.  Boxes, circles and capsules are met by the circle casts' own routines (query_kernels.h q_cast_aabb, q_cast_disc,
// q_cast_disc_normal); a polygon's true outline by sweep_cast_polygon below.  Every operation fp32 and rounded on its own.
#pragma once

#include "sweep.h"
#include "query_kernels.h"
#include "narrowphase.h"
#include "pair_set.h"

namespace phx {

// One workgroup walks [0, n) in order and keeps the items `pred` accepts: write(i, rank) with rank the number of accepted items in
// front of i; *count = their number.  (A single group: the lists this makes change rarely — the continuous bodies — or are asked for
// on demand — the hits.)
template <class Pred, class Write>
__device__ __forceinline__ void sweep_ordered_compact(int n, unsigned* __restrict__ count, Pred pred, Write write)
{
    __shared__ unsigned wave_count[4];
    unsigned base = 0;
    const int wave = threadIdx.x >> 6;
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const bool take = i < n && pred(i);
        const unsigned long long mask = __ballot(take);
        if ((threadIdx.x & 63) == 0) wave_count[wave] = (unsigned)__popcll(mask);
        __syncthreads();
        unsigned before = base, total = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) { before += k < wave ? wave_count[k] : 0u; total += wave_count[k]; }
        if (take) write(i, before + (unsigned)__popcll(mask & q_lanes_below()));
        base += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *count = base;
}

// the compact list of the continuous bodies, ascending: the bodies whose core radius is above 0
static __global__ void __launch_bounds__(256) k_sweep_list(const float4* __restrict__ cells, int n, int* __restrict__ list, unsigned* __restrict__ count)
{
    sweep_ordered_compact(n, count, [&](int i) { return cells[i].x > 0.f; }, [&](int i, unsigned at) { list[at] = i; });
}

// start := pos of the listed bodies, before the step's integrator is queued
static __global__ void __launch_bounds__(256) k_sweep_start(const int* __restrict__ list, int count, const float4* __restrict__ mpos, float4* __restrict__ cells)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = list[k];
        const float4 m = mpos[i];
        cells[i] = make_float4(cells[i].x, m.z, m.w, 0.f);
    }
}

// the clamps of a pass, ascending by body: the slots (one per listed body, body -1: no clamp) compacted in order
static __global__ void __launch_bounds__(256) k_sweep_hits(const phx_sweep_hit* __restrict__ slots, int count, phx_sweep_hit* __restrict__ out, unsigned* __restrict__ total)
{
    sweep_ordered_compact(count, total, [&](int k) { return slots[k].body >= 0; }, [&](int k, unsigned at) { out[at] = slots[k]; });
}

// The skin, rc / 64 (include/phyx_amd.h CONTINUOUS BODIES, "the skin", says why).  It enters the rule in two places, both in
// k_sweep_bodies: a hit counts only if the step approaches the target by more than the skin (dot(normal, d) < -skin), and a clamped body
// is put back a skin short of the first touch (t - skin / approach, not below 0).
__device__ __forceinline__ float sweep_skin(float rc) { return rc * 0.015625f; }

// The disc {o, rc} cast along d over t in [0, 1] against a polygon's outline, in the polygon's frame (o', d' as in the ray rule).
//   start overlap (the discrete contact owns the pair: no hit): s_k = dot(n_k, o' - v_k), k the largest, the first on a tie; s <= 0; or,
//     with e = v_(k+1) - v_k and u = dot(o' - v_k, e): u < 0 picks q = v_k, u > dot(e, e) picks q = v_(k+1), there h = o' - q and
//     dot(h, h) < rc*rc; otherwise s < rc.
//   faces, k in index order: den = dot(n_k, d') < 0; t = (dot(n_k, v_k - o') + rc) / den in [0, 1]; p = o' + d'*t, u = dot(p - v_k, e) with
//     0 <= u <= dot(e, e); the normal n_k.
//   vertices, k in index order: the ray/disc rule (q_ray_disc) about v_k with radius rc and max_t 1, tin >= 0; the normal (nx, ny) / rc.
//   The smallest t wins, the first candidate in this order on a tie.  The normal comes back in the frame.
__device__ __forceinline__ bool sweep_cast_polygon(float sx, float sy, float rc, float dx, float dy, float4 m, float4 f, const PolyRec* __restrict__ poly,
                                                   float& t_out, float& nx_out, float& ny_out)
{
    const float rx = sx - m.z, ry = sy - m.w;
    const float ox = rx * f.x + ry * f.y, oy = rx * f.z + ry * f.w;
    const float dxp = dx * f.x + dy * f.y, dyp = dx * f.z + dy * f.w;
    const int n = poly->count;
    {
        int k = 0;
        float s = poly->n[0] * (ox - poly->v[0]) + poly->n[1] * (oy - poly->v[1]);
        for (int j = 1; j < n; ++j) {
            const float c = poly->n[2 * j] * (ox - poly->v[2 * j]) + poly->n[2 * j + 1] * (oy - poly->v[2 * j + 1]);
            if (c > s) { s = c; k = j; }
        }
        if (s <= 0.f) return false;
        const int k1 = k + 1 < n ? k + 1 : 0;
        const float vx = poly->v[2 * k], vy = poly->v[2 * k + 1], wx = poly->v[2 * k1], wy = poly->v[2 * k1 + 1];
        const float ex = wx - vx, ey = wy - vy;
        const float u = (ox - vx) * ex + (oy - vy) * ey;
        const bool lo = u < 0.f, hi = !lo && u > ex * ex + ey * ey;
        if (lo || hi) {
            const float hx = ox - (lo ? vx : wx), hy = oy - (lo ? vy : wy);
            if (hx * hx + hy * hy < rc * rc) return false;
        } else if (s < rc) return false;
    }
    bool hit = false;
    float best = 0.f, bnx = 0.f, bny = 0.f;
    for (int k = 0; k < n; ++k) {
        const int k1 = k + 1 < n ? k + 1 : 0;
        const float nx = poly->n[2 * k], ny = poly->n[2 * k + 1], vx = poly->v[2 * k], vy = poly->v[2 * k + 1];
        const float den = nx * dxp + ny * dyp;
        if (!(den < 0.f)) continue;
        const float t = ((nx * (vx - ox) + ny * (vy - oy)) + rc) / den;
        if (!(t >= 0.f && t <= 1.f)) continue;
        const float ex = poly->v[2 * k1] - vx, ey = poly->v[2 * k1 + 1] - vy;
        const float px = ox + dxp * t, py = oy + dyp * t;
        const float u = (px - vx) * ex + (py - vy) * ey;
        if (!(u >= 0.f && u <= ex * ex + ey * ey)) continue;
        if (!hit || t < best) { hit = true; best = t; bnx = nx; bny = ny; }
    }
    for (int k = 0; k < n; ++k) {
        float tin, nx, ny;
        if (!q_ray_disc(ox - poly->v[2 * k], oy - poly->v[2 * k + 1], dxp, dyp, 1.0f, rc, tin, nx, ny)) continue;
        if (tin < 0.f) continue;
        if (!hit || tin < best) { hit = true; best = tin; bnx = nx / rc; bny = ny / rc; }
    }
    t_out = best; nx_out = bnx; ny_out = bny;
    return hit;
}

// one target: the cast by its kind; t in [0, 1] and the world normal.  A start inside the widened shape (tin < 0: the core overlaps the
// target at t = 0) is no hit.
template <int SHAPES>
__device__ __forceinline__ bool sweep_cast(const QDiscCast& c, unsigned kind, float4 a, float4 m, float4 f, float2 h, const PolyRec* __restrict__ poly, float& t, float& nx, float& ny)
{
    constexpr int CAPS = SHAPES == SWEEP_POLYGONS ? 2 : (SHAPES == SWEEP_CAPSULES ? 1 : 0);
    if (SHAPES == SWEEP_POLYGONS && kind == (unsigned)PHX_SHAPE_POLYGON) {
        float lx, ly;
        if (!sweep_cast_polygon(c.c.cx, c.c.cy, c.c.r, c.dx, c.dy, m, f, poly, t, lx, ly)) return false;
        nx = f.x * lx + f.z * ly; ny = f.y * lx + f.w * ly;
        return true;
    }
    QCastDisc cd;
    if (!q_cast_disc<CAPS>(c, kind, m, f, h, cd)) return false;
    if (cd.tin < 0.f) return false;
    const float2 nn = q_cast_disc_normal<CAPS>(cd, f, h, c.c.r);
    t = cd.tin > 0.f ? cd.tin : 0.f; nx = nn.x; ny = nn.y;
    return true;
}

// The pass: one wave per continuous body, the lanes stride over all bodies.  The cheap rejects first — the target is static (both inverse
// masses read 0: a sleeper is one), the swept disc's box meets its AABB — then sensor, filter and exclusion as the step applies them,
// then the exact cast; a candidate counts only if the step approaches it by more than the skin (dot(normal, d) < -skin).  The wave takes
// the smallest (t, index); lane 0 stops the body a skin short of that touch, t' = max(t - skin / approach, 0), and writes
// pos = start + d*t', the AABB (geom_aabb) and the body's slot of the hit list, whose t is t'.  totals[0] += the clamps.
template <int SHAPES>
static __global__ void __launch_bounds__(256) k_sweep_bodies(WorldBodies w, int n, const int* __restrict__ list, int count, const float4* __restrict__ cells,
                                                             SweepTables tb, phx_sweep_hit* __restrict__ slots, unsigned long long* __restrict__ totals)
{
    constexpr int CAPS = SHAPES == SWEEP_POLYGONS ? 2 : (SHAPES == SWEEP_CAPSULES ? 1 : 0);
    const int lane = threadIdx.x & 63;
    const int waves = (int)((gridDim.x * blockDim.x) >> 6);
    for (int k = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6); k < count; k += waves) {
        const int i = list[k];
        const float4 cell = cells[i], mi = w.s.mpos[i];
        const float rc = cell.x, dx = mi.z - cell.y, dy = mi.w - cell.z;
        bool live = rc > 0.f && !(mi.x == 0.f && mi.y == 0.f) && (dx != 0.f || dy != 0.f);
        if (live && tb.flags) live = (tb.flags[i] & PHX_BODY_SENSOR) == 0u;
        unsigned long long best = ~0ull;
        float bnx = 0.f, bny = 0.f;
        if (live) {
            const QDiscCast c = {{cell.y, cell.z, rc}, dx, dy, 1.0f};
            const uint4 fa = tb.filters ? tb.filters[i] : make_uint4(0u, 0u, 0u, 0u);
            const unsigned xa = tb.xmember ? tb.xmember[i] : 0u;
            for (int j = lane; j < n; j += 64) {
                const float4 m = w.s.mpos[j];
                if (!(m.x == 0.f && m.y == 0.f)) continue;
                const float4 a = w.aabb[j];
                if (!q_cast_aabb(c, a)) continue;
                if (tb.flags && (tb.flags[j] & PHX_BODY_SENSOR)) continue;
                if (tb.filters && !collision_filter_pass(fa, tb.filters[j])) continue;
                if (xa && ps_contains(tb.xtable, tb.xmask, ps_unordered_key((unsigned)i, (unsigned)j))) continue;
                const unsigned kind = SHAPES == SWEEP_BOXES ? (unsigned)PHX_SHAPE_BOX : q_kind<CAPS>(w.kinds, j);
                float t, nx, ny;
                if (!sweep_cast<SHAPES>(c, kind, a, m, w.frame[j], w.size[j], q_poly<CAPS>(w, j), t, nx, ny)) continue;
                if (!(nx * dx + ny * dy < -sweep_skin(rc))) continue;
                const unsigned long long key = q_ray_key(t, j);
                if (key < best) { best = key; bnx = nx; bny = ny; }      // (j ascends in a lane: the lowest index stays on a tie)
            }
        }
        const unsigned long long won = q_wave_min64(best);
        phx_sweep_hit hit;
        hit.body = -1; hit.target = -1; hit.t = 0.f; hit.normal.x = 0.f; hit.normal.y = 0.f;
        if (won != ~0ull) {
            const int src = __builtin_ctzll(__ballot(best == won));
            const float nx = __shfl(bnx, src), ny = __shfl(bny, src);
            if (lane == 0) {
                const float approach = -(nx * dx + ny * dy);               // (> skin: the candidate's own test)
                const float back = __uint_as_float((unsigned)(won >> 32)) - sweep_skin(rc) / approach;
                const float t = back > 0.f ? back : 0.f;
                const float4 f = w.frame[i];
                const float2 sz = w.size[i];
                const float px = cell.y + dx * t, py = cell.z + dy * t;
                float4 box;
                geom_aabb(v2(px, py), v2(f.x, f.y), v2(f.z, f.w), v2(sz.x, sz.y), box.x, box.y, box.z, box.w);
                w.s.mpos[i] = make_float4(mi.x, mi.y, px, py);
                w.aabb[i] = box;
                hit.body = i; hit.target = (int)(unsigned)(won & 0xFFFFFFFFull); hit.t = t; hit.normal.x = nx; hit.normal.y = ny;
                atomicAdd(totals, 1ull);
            }
        }
        if (lane == 0) slots[k] = hit;
    }
}

} // namespace phx
