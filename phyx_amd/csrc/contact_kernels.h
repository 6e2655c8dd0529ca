// contact_kernels.h — the device side of the World's contact reports (include/phyx_amd.h, CONTACTS): the contacts of listed bodies,
// the touch events and the markers, over the resident contact cache (manifolds, contact points, joints in the reference's layouts) and
// the resident body arrays (body_view.h).  A record is a copy or an fp32 sum of stored floats, each sum rounded on its own (the library
// is compiled with -ffp-contract=off); tests/contact_spec.py states every field again in numpy.
//
// Contacts, two paths with byte-identical results:
//   scan   manifolds in lanes, a chunk of listed bodies in LDS: count per listing (LDS counters, one global atomic per workgroup and
//          listing), offsets by device_scan.h, a fill through per-listing cursors (unordered), then one workgroup per segment ranks its
//          records by (other, manifold, slot) — the keys are unique, so the rank is the position;
//   index  a body -> (other, manifold) incidence in CSR form: 2 entries per manifold, per-body counts and an exclusive scan give the
//          offsets, two stable radix passes (by other, then by body) over entries made in manifold order put each body's segment in
//          (other, manifold) order; a listing's records are its segment's live slots, one lane per listing, already in order.
// Events: the touching manifolds' (body1, body2) keys — the others as a sentinel that sorts last — in two stable radix passes, adjacent
// duplicates dropped (T), then T \ B and B \ T by binary search, one lane per key; all three compacted by flag / scan / compact.
#pragma once

#include "body_view.h"
#include "sleep.h"

namespace phx {

constexpr int C_SKIP_STATIC = 1;                // PHX_QUERY_SKIP_STATIC
constexpr int C_CHUNK_MAX = 1024;               // listed bodies per scan-path chunk (LDS: 4 KiB of bodies, 4 KiB of counters)
constexpr int C_SORT_TILE = 1024;               // keys per LDS tile of the segment ranking

// (`sleep`: the sleep column, null while sleeping is off: a sleeper is not static to a report, as to a query)
__device__ __forceinline__ bool c_static(const float4* __restrict__ mpos, const SleepCell* __restrict__ sleep, int b)
{
    const float4 m = mpos[b];
    return m.x == 0.f && m.y == 0.f && !(sleep && sleep[b].asleep);
}

// live slots of a manifold: point_count clamped to the two slots it owns (set_state and the step keep it in [0, 2])
__device__ __forceinline__ int c_live(const phx_manifold& m) { return m.point_count < 0 ? 0 : (m.point_count > 2 ? 2 : m.point_count); }

// the record of slot k of manifold mi seen from its body `side` (0: body1, 1: body2)
__device__ __forceinline__ phx_contact c_record(const phx_manifold& m, int mi, int k, int side, const float4* __restrict__ mpos,
                                                const phx_contact_point* __restrict__ cps, const phx_contact_joint* __restrict__ joints, int nj)
{
    const phx_contact_point cp = cps[m.point_index + k];
    const int b = side ? m.body2 : m.body1;
    const float4 mp = mpos[b];
    phx_contact r;
    r.other = side ? m.body1 : m.body2;
    r.manifold = mi;
    r.slot = k;
    const phx_vec2 d = side ? cp.delta2 : cp.delta1;
    r.point.x = mp.z + d.x;
    r.point.y = mp.w + d.y;
    r.normal.x = side ? -cp.normal.x : cp.normal.x;
    r.normal.y = side ? -cp.normal.y : cp.normal.y;
    int flags = cp.is_newly_created ? PHX_CONTACT_NEW : 0;
    if (cp.solver_index >= 0 && cp.solver_index < nj) {
        const phx_contact_joint j = joints[cp.solver_index];
        r.normal_impulse = j.normal_accumulated_impulse;
        r.friction_impulse = j.friction_accumulated_impulse;
    } else {
        r.normal_impulse = 0.f;
        r.friction_impulse = 0.f;
        flags |= PHX_CONTACT_NO_JOINT;
    }
    r.flags = flags;
    return r;
}

__device__ __forceinline__ unsigned long long c_key(const phx_contact& r)
{
    return ((unsigned long long)(unsigned)r.other << 32) | ((unsigned)r.manifold << 1) | (unsigned)r.slot;
}

// ---- scan path ------------------------------------------------------------------------------------------------------------------
// FILL = false: counts[q0 + q] += the records of listing q0 + q;  FILL = true: each record goes to out[cursor[q0 + q]++] (unordered)
template <bool FILL>
static __global__ void __launch_bounds__(256) k_cscan(const phx_manifold* __restrict__ manifolds, int nm, const float4* __restrict__ mpos, const SleepCell* __restrict__ sleep,
                                                      const phx_contact_point* __restrict__ cps, const phx_contact_joint* __restrict__ joints, int nj,
                                                      const int* __restrict__ bodies, int q0, int nq, int flags, unsigned* __restrict__ counts,
                                                      unsigned* __restrict__ cursor, phx_contact* __restrict__ out)
{
    __shared__ int s_body[C_CHUNK_MAX];
    __shared__ unsigned s_count[C_CHUNK_MAX];
    for (int q = threadIdx.x; q < nq; q += blockDim.x) { s_body[q] = bodies[q0 + q]; s_count[q] = 0u; }
    __syncthreads();
    const bool skip = flags & C_SKIP_STATIC;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        const int live = c_live(m);
        if (!live) continue;
        const bool keep1 = !skip || !c_static(mpos, sleep, m.body2);      // records of body1 (other = body2)
        const bool keep2 = !skip || !c_static(mpos, sleep, m.body1);
        for (int q = 0; q < nq; ++q) {
            const int b = s_body[q];
            for (int side = 0; side < 2; ++side) {
                if (b != (side ? m.body2 : m.body1) || !(side ? keep2 : keep1)) continue;
                if constexpr (!FILL) atomicAdd(&s_count[q], (unsigned)live);
                else {
                    const unsigned at = atomicAdd(&cursor[q0 + q], (unsigned)live);
                    for (int k = 0; k < live; ++k) out[at + k] = c_record(m, i, k, side, mpos, cps, joints, nj);
                }
            }
        }
    }
    if constexpr (!FILL) {
        __syncthreads();
        for (int q = threadIdx.x; q < nq; q += blockDim.x)
            if (s_count[q]) atomicAdd(&counts[q0 + q], s_count[q]);
    }
}

// one workgroup per segment [seg[q], ends[q]) (grid-strided): out[seg[q] + rank] = in[seg[q] + i], rank = how many keys of the segment
// are smaller
static __global__ void __launch_bounds__(256) k_csort_segments(const phx_contact* __restrict__ in, const unsigned* __restrict__ seg,
                                                               const unsigned* __restrict__ ends, int count, phx_contact* __restrict__ out)
{
    __shared__ unsigned long long s_key[C_SORT_TILE];
    for (int q = blockIdx.x; q < count; q += gridDim.x) {
        const unsigned base = seg[q], n = ends[q] - base;
        if (n == 1 && threadIdx.x == 0) out[base] = in[base];
        if (n <= 1) continue;                                       // (uniform across the workgroup)
        for (unsigned i0 = 0; i0 < n; i0 += blockDim.x) {
            const unsigned i = i0 + threadIdx.x;
            const bool mine = i < n;
            const unsigned long long key = mine ? c_key(in[base + i]) : 0ull;
            unsigned rank = 0;
            for (unsigned t0 = 0; t0 < n; t0 += C_SORT_TILE) {
                const unsigned tn = n - t0 < (unsigned)C_SORT_TILE ? n - t0 : (unsigned)C_SORT_TILE;
                __syncthreads();
                for (unsigned t = threadIdx.x; t < tn; t += blockDim.x) s_key[t] = c_key(in[base + t0 + t]);
                __syncthreads();
                if (mine)
                    for (unsigned t = 0; t < tn; ++t) rank += s_key[t] < key ? 1u : 0u;
            }
            if (mine) out[base + rank] = in[base + i];
        }
        __syncthreads();
    }
}

// ---- index path -----------------------------------------------------------------------------------------------------------------
// entries e = 2 * manifold + side, made in manifold order: key = the entry's body, value = e; the first pass sorts by the other body
static __global__ void __launch_bounds__(256) k_cidx_entries(const phx_manifold* __restrict__ manifolds, int nm, unsigned* __restrict__ other,
                                                             unsigned* __restrict__ entry, unsigned* __restrict__ body_count)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        other[2 * i] = (unsigned)m.body2;     entry[2 * i] = 2u * (unsigned)i;
        other[2 * i + 1] = (unsigned)m.body1; entry[2 * i + 1] = 2u * (unsigned)i + 1u;
        atomicAdd(&body_count[m.body1], 1u);
        atomicAdd(&body_count[m.body2], 1u);
    }
}

// the second pass's keys: the body of each entry, in the first pass's order
static __global__ void __launch_bounds__(256) k_cidx_body_keys(const phx_manifold* __restrict__ manifolds, const unsigned* __restrict__ entry, int ne,
                                                               unsigned* __restrict__ body)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < ne; i += gridDim.x * blockDim.x) {
        const unsigned e = entry[i];
        const phx_manifold m = manifolds[e >> 1];
        body[i] = (unsigned)((e & 1u) ? m.body2 : m.body1);
    }
}

// COUNT: counts[q] = the records of listing q;  FILL: its records at out[seg[q] ..], in segment order
template <bool FILL>
static __global__ void __launch_bounds__(256) k_cidx_query(const phx_manifold* __restrict__ manifolds, const float4* __restrict__ mpos, const SleepCell* __restrict__ sleep,
                                                           const phx_contact_point* __restrict__ cps, const phx_contact_joint* __restrict__ joints, int nj,
                                                           const unsigned* __restrict__ offsets, const unsigned* __restrict__ entries,
                                                           const int* __restrict__ bodies, int count, int flags, unsigned* __restrict__ counts,
                                                           const unsigned* __restrict__ seg, phx_contact* __restrict__ out)
{
    const bool skip = flags & C_SKIP_STATIC;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < count; q += gridDim.x * blockDim.x) {
        const int b = bodies[q];
        const unsigned lo = offsets[b], hi = offsets[b + 1];
        unsigned at = FILL ? seg[q] : 0u;
        for (unsigned j = lo; j < hi; ++j) {
            const unsigned e = entries[j];
            const int mi = (int)(e >> 1), side = (int)(e & 1u);
            const phx_manifold m = manifolds[mi];
            const int live = c_live(m);
            if (!live || (skip && c_static(mpos, sleep, side ? m.body1 : m.body2))) continue;
            if constexpr (FILL) { for (int k = 0; k < live; ++k) out[at + k] = c_record(m, mi, k, side, mpos, cps, joints, nj); }
            at += (unsigned)live;
        }
        if constexpr (!FILL) counts[q] = at;
    }
}

// ---- events ---------------------------------------------------------------------------------------------------------------------
// keys of the first pass: body2 (value body1) of the touching manifolds, the sentinel n for the others (it sorts behind every body)
static __global__ void __launch_bounds__(256) k_cev_keys(const phx_manifold* __restrict__ manifolds, int nm, unsigned n, unsigned* __restrict__ b2,
                                                         unsigned* __restrict__ b1)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i];
        const bool touching = m.point_count > 0;
        b2[i] = touching ? (unsigned)m.body2 : n;
        b1[i] = touching ? (unsigned)m.body1 : n;
    }
}

__device__ __forceinline__ unsigned long long c_pair(unsigned b1, unsigned b2) { return ((unsigned long long)b1 << 32) | b2; }

// T: sorted (body1, body2) with the sentinels behind; an element is kept if it is no sentinel and differs from its predecessor
struct CevUniqueLoad {
    const unsigned* b1; const unsigned* b2; unsigned n;
    __device__ unsigned operator()(int i) const { return b1[i] < n && (i == 0 || b1[i] != b1[i - 1] || b2[i] != b2[i - 1]) ? 1u : 0u; }
    static constexpr bool in_place = false;
};

static __global__ void __launch_bounds__(256) k_cev_unique(const unsigned* __restrict__ b1, const unsigned* __restrict__ b2, int nm, unsigned n,
                                                           const unsigned* __restrict__ pos, unsigned long long* __restrict__ t)
{
    const CevUniqueLoad keep{b1, b2, n};
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nm; i += gridDim.x * blockDim.x)
        if (keep(i)) t[pos[i]] = c_pair(b1[i], b2[i]);
}

__device__ __forceinline__ bool c_contains(const unsigned long long* __restrict__ set, unsigned n, unsigned long long key)
{
    unsigned lo = 0, hi = n;
    while (lo < hi) {
        const unsigned mid = lo + ((hi - lo) >> 1);
        if (set[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo < n && set[lo] == key;
}

// element i of `from` (its size: *from_n if from_n is set, else from_count) that is not in `in` (size: *in_n if set, else in_count)
struct CevMissingLoad {
    const unsigned long long* from; const unsigned* from_n; unsigned from_count;
    const unsigned long long* in; const unsigned* in_n; unsigned in_count;
    static constexpr bool in_place = false;
    __device__ unsigned operator()(int i) const
    {
        const unsigned nf = from_n ? *from_n : from_count, ni = in_n ? *in_n : in_count;
        return (unsigned)i < nf && !c_contains(in, ni, from[i]) ? 1u : 0u;
    }
};

static __global__ void __launch_bounds__(256) k_cev_missing(CevMissingLoad miss, int count, const unsigned* __restrict__ pos, int2* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
        if (miss(i)) { const unsigned long long k = miss.from[i]; out[pos[i]] = make_int2((int)(k >> 32), (int)(k & 0xFFFFFFFFull)); }
}

// the removal's remap of B: kept iff both bodies are kept; new[] is monotonic, so the kept keys stay sorted
struct CevRemapLoad {
    const unsigned long long* b; const int* remap;
    static constexpr bool in_place = false;
    __device__ unsigned operator()(int i) const { const unsigned long long k = b[i]; return remap[k >> 32] >= 0 && remap[k & 0xFFFFFFFFull] >= 0 ? 1u : 0u; }
};

static __global__ void __launch_bounds__(256) k_cev_remap(CevRemapLoad keep, int count, const unsigned* __restrict__ pos, unsigned long long* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < count; i += gridDim.x * blockDim.x)
        if (keep(i)) {
            const unsigned long long k = keep.b[i];
            out[pos[i]] = c_pair((unsigned)keep.remap[k >> 32], (unsigned)keep.remap[k & 0xFFFFFFFFull]);
        }
}

// ---- markers --------------------------------------------------------------------------------------------------------------------
static __global__ void __launch_bounds__(256) k_cmarkers(const phx_manifold* __restrict__ manifolds, int nm, const float4* __restrict__ mpos,
                                                         const phx_contact_point* __restrict__ cps, phx_contact_marker* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < 2 * nm; i += gridDim.x * blockDim.x) {
        const phx_manifold m = manifolds[i >> 1];
        const int k = i - m.point_index;
        phx_contact_marker r;
        if (k >= 0 && k < c_live(m)) {
            const phx_contact_point cp = cps[i];
            const float4 p1 = mpos[m.body1], p2 = mpos[m.body2];
            r.point1.x = p1.z + cp.delta1.x; r.point1.y = p1.w + cp.delta1.y;
            r.point2.x = p2.z + cp.delta2.x; r.point2.y = p2.w + cp.delta2.y;
            r.live = 1;
            r.newly_created = cp.is_newly_created;
        } else {
            r.point1.x = r.point1.y = r.point2.x = r.point2.y = 0.f;
            r.live = 0; r.newly_created = 0;
        }
        out[i] = r;
    }
}

} // namespace phx
