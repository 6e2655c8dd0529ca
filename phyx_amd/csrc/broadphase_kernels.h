// broadphase_kernels.h — the device side of the single-axis sweep-and-prune broadphase on gfx950: its kernels, the sweep's views and
// the layout of what they share with the host (broadphase.hip, the only file that includes this: a second one would emit every
// non-template kernel here a second time).
//
// Replaces (ref = the reference's src): Collider::UpdateBroadphase (Collider.cpp:251-284) = key build with
// radixFloat (base/RadixSort.h:19-26) + radixSort3 (base/RadixSort.h:28-95) + gather of sorted
// BroadphaseEntry records; Collider::UpdatePairs* (Collider.cpp:286-366) = forward sweep with the y-overlap
// test and the persistent pair set `manifoldMap` (Collider.h:58, base/DenseHash.h).
//
// Device layout:
//   keys/idx      u32 key = radixFloat(aabb.min.x), u32 idx — two ping-pong pairs of SoA arrays
//   entries       float4 {minx, maxx, centery, extenty} per sorted position + u32 body index (SoA)
//   pair set      open-addressing table of u64 (index_i << 32 | index_j), linear probing, in HBM
//   new pairs     uint2 list in the reference's serial emission order (row i ascending, then j)
//
// The sort is a stable LSD radix sort on the full 32-bit key.  The reference splits the key 11/11/10; a
// stable sort's output permutation does not depend on the digit split, so 4 passes of 8 bits (256-bin
// LDS histograms, one wave-private counter row per wave) give the identical sequence.
#pragma once

#include "device_scan.h"
#include "exclusions.h"
#include "splitter_sort.h"
#include "pair_set.h"

#include <algorithm>

namespace phx {

static inline int grid_for(int n, int per_block = 256, int cap = 4096) { return std::max(1, std::min(div_up(n, per_block), cap)); }

// the C-ABI edge: the AABBs of 128-byte records (ref: Collider.cpp:259-265)
__global__ void __launch_bounds__(256) k_extract_aabb(const phx_rigid_body* __restrict__ bodies, int n, float4* __restrict__ aabb)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        aabb[i] = make_float4(bodies[i].aabb_min.x, bodies[i].aabb_min.y, bodies[i].aabb_max.x, bodies[i].aabb_max.y);
}

// the LSD sort's keys (ref: Collider.cpp:259-265); the first kernel of such an update (splitter_sort.h update_head).
// INTEGRATE: IntegrateVelocity rides along (body_view.h integrate_velocity) — a body's key is its AABB's min x, which that does not touch
template <bool INTEGRATE>
__global__ void __launch_bounds__(256) k_build_keys(const float4* __restrict__ aabb, int n, unsigned* __restrict__ keys, unsigned* __restrict__ idx, UpdateHead head)
{
    update_head<INTEGRATE>(head);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        keys[i] = radix_float(aabb[i].x);
        idx[i] = (unsigned)i;
        if (INTEGRATE) head.vel[i] = integrate_velocity(head.vel[i], head.accel ? head.accel[i] : make_float4(0.f, 0.f, 0.f, 0.f), head.mpos[i].x, head.gravity, head.dt);
    }
}

// ref: Collider.cpp:269-283
// (`splitters`: the records at positions SS_STRIDE, 2 SS_STRIDE, ... of the sorted sequence — what the next update deals its bodies
//  into buckets by, splitter_sort.h)
__global__ void __launch_bounds__(256) k_gather_entries(const float4* __restrict__ aabb, const unsigned* __restrict__ keys, const unsigned* __restrict__ idx, int n,
                                                        float4* __restrict__ entries, unsigned long long* __restrict__ splitters, int stride)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 b = aabb[idx[i]];
        const float minx = b.x, miny = b.y, maxx = b.z, maxy = b.w;
        entries[i] = make_float4(minx, maxx, (miny + maxy) * 0.5f, (maxy - miny) * 0.5f);
        if (i && i % stride == 0) splitters[i / stride - 1] = ((unsigned long long)keys[i] << 32) | idx[i];
    }
}

// ---- persistent pair set (the table as the device reads it — PS_EMPTY, ps_hash, ps_contains: pair_set.h) ----------------------

// keys are distinct and known to be absent
__global__ void __launch_bounds__(256) k_ps_insert(unsigned long long* table, unsigned mask, const uint2* __restrict__ pairs, int n, unsigned long long* __restrict__ end_stamp)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long k = ps_ordered_key(pairs[i].x, pairs[i].y);
        unsigned p = ps_hash(k) & mask;
        for (;;) {
            const unsigned long long s = table[p];
            if (s == PS_EMPTY || s == PS_TOMB) {
                if (atomicCAS(&table[p], s, k) == s) break;
                continue;      // lost the slot to another inserter: look at it again
            }
            p = (p + 1) & mask;
        }
    }
    if (end_stamp && threadIdx.x == 0) atomicMax(end_stamp, (unsigned long long)wall_clock64());      // (the update's last kernel)
}

__global__ void __launch_bounds__(256) k_ps_erase(unsigned long long* table, unsigned mask, const uint2* __restrict__ pairs, int n, int* erased)
{
    int mine = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned long long k = ps_ordered_key(pairs[i].x, pairs[i].y);
        unsigned p = ps_hash(k) & mask;
        for (;;) {
            const unsigned long long s = table[p];
            if (s == k) { table[p] = PS_TOMB; ++mine; break; }
            if (s == PS_EMPTY) break;
            p = (p + 1) & mask;
        }
    }
    for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);      // one atomic per wave
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(erased, mine);
}

__global__ void __launch_bounds__(256) k_ps_rehash(const unsigned long long* __restrict__ old_table, unsigned old_cap,
                                                   unsigned long long* table, unsigned mask)
{
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < old_cap; i += gridDim.x * blockDim.x) {
        const unsigned long long k = old_table[i];
        if (k == PS_EMPTY || k == PS_TOMB) continue;
        unsigned p = ps_hash(k) & mask;
        for (;;) {
            if (table[p] == PS_EMPTY && atomicCAS(&table[p], PS_EMPTY, k) == PS_EMPTY) break;
            p = (p + 1) & mask;
        }
    }
}

// ---- sweep (ref: Collider.cpp:296-318 serial order, :347-366 per-row body) ----------------------------
// Rows with a short scan range are swept one row per lane: lane l of a wave owns sorted row i0+l and reads
// entries[i0+l+1+t] in step t, so a wave's loads are contiguous.  Rows whose range exceeds HUB_LEN (the
// ground box spans every column) are deferred to a workgroup-per-row kernel.
constexpr int STAT_SLOTS = 64;     // same-address atomics serialise (~10 ns each): 31k of them cost 0.3 ms of a 0.4 ms kernel
constexpr int ROW_CACHE = 4;        // new pairs remembered per row by the count pass (rows with more are rescanned by the emit pass)
constexpr int HUB_LEN = 2048;      // rows scanning more candidates than this are cut into chunks
constexpr int HUB_CHUNK = 512;     // candidates per chunk = one 256-lane workgroup x 2 tiles (2048: the ground row of the 200k-box scene was 98 workgroups
                                   // walking eight dependent tiles each, 10 us per pass; 391 workgroups of two are done in a third of that)

// The update's small words (DeviceBroadphase::small_, 64 bits each): cleared by the update's first kernel (UpdateHead), written by the
// count pass and the scan, read back by the host in one piece.
constexpr int SMALL_CHUNKS_NEEDED = 2;      // low half: hub chunks the count pass asked for (more than the list holds: the host grows it and counts again)
constexpr int SMALL_NEW_PAIRS = 3;          // low half: the total of the rows' new pairs (the scan's)
constexpr int SMALL_CACHE_OVERFLOW = 4;     // low half: some row found more than ROW_CACHE new pairs
constexpr int SMALL_STATS = 16;             // 2 * STAT_SLOTS statistics words from here (SweepView::counters)
constexpr int SMALL_WORDS = SMALL_STATS + 2 * STAT_SLOTS;

struct SweepView {
    const float4* entries;
    const unsigned* idx;
    int n;
    const unsigned long long* table;
    unsigned mask;
    unsigned* row_count;       // new pairs per row
    unsigned* row_cache;       // count pass: the first ROW_CACHE new partners of every row (index_j)
    int* cache_overflow;       // set by the count pass if some row found more than ROW_CACHE new pairs
    int4* chunks;              // hub chunks {row, j_begin, j_end, index of the row's first chunk}
    unsigned* chunk_count;     // new pairs per chunk, later: the chunk's base inside its row
    int* n_chunks;
    int chunk_cap;
    unsigned long long* counters;   // statistics, spread over STAT_SLOTS slots to keep the atomics apart: [2 * slot] candidate tests, [2 * slot + 1] overlapping pairs
};

// A World with collision filters (common.h collision_filter_pass) sweeps with this view: the same kernels instantiated on it test the
// rule where a y-overlapping candidate's body index is looked up, before the pair-set lookup — a rejected pair costs one 16-byte gather
// and no hash probe, and is neither counted as new, nor cached, nor emitted (its overlap is still counted: phx_broadphase_stats).
// Instantiated on the plain SweepView the kernels are the unfiltered code, instruction for instruction.
struct FilteredSweepView : SweepView {
    const uint4* filters;      // per body {category, mask, group, 0}
};
template <class V> struct SweepFilter { static constexpr bool on = false; };
template <> struct SweepFilter<FilteredSweepView> { static constexpr bool on = true; };
template <class V> __device__ __forceinline__ uint4 sweep_filter_of(const V& v, unsigned body)
{
    if constexpr (SweepFilter<V>::on) return v.filters[body];
    else return make_uint4(0u, 0u, 0u, 0u);
}

// A World with collision exclusions (exclusions.h) sweeps with one of these two views: the second trait of the same kernels.  The test
// stands behind the collision filter and in front of the pair-set lookup.  A row reads its body's word once, where it reads its filter:
// a body in no excluded pair makes no probe at all.  Any other row probes the exclusions' table once per y-overlapping candidate that
// passed the filter — the key is of the UNORDERED pair (ps_unordered_key: ia, ib come in sorted-row order, not index order) — and the
// probe's first load is issued with the pair-set lookups', so that the row's SWEEP_LOOK loads stay in flight together.  A rejected
// candidate is what a filtered one is: not new, not cached, not emitted, its overlap counted.  The count pass, the rescan and the
// chunk kernels apply the same test, or the offsets would lie.
struct ExcludedSweepView : SweepView {
    ExclusionView excl;
};
struct FilteredExcludedSweepView : FilteredSweepView {
    ExclusionView excl;
};
template <> struct SweepFilter<FilteredExcludedSweepView> { static constexpr bool on = true; };
template <class V> struct SweepExclude { static constexpr bool on = false; };
template <> struct SweepExclude<ExcludedSweepView> { static constexpr bool on = true; };
template <> struct SweepExclude<FilteredExcludedSweepView> { static constexpr bool on = true; };
template <class V> __device__ __forceinline__ unsigned sweep_member_of(const V& v, unsigned body)       // the row's word: in some excluded pair?
{
    if constexpr (SweepExclude<V>::on) return v.excl.member[body];
    else return 0u;
}
template <class V> __device__ __forceinline__ bool sweep_excluded(const V& v, unsigned ia, unsigned ib)
{
    if constexpr (SweepExclude<V>::on) return ps_contains(v.excl.table, v.excl.mask, ps_unordered_key(ia, ib));
    else return false;
}
// Is the y-overlapping candidate `ib` of the row of body `ia` (filter fa, exclusion word xa) a NEW pair?  The chain in its one order —
// collision filter, exclusion (only a row with xa probes), pair set — for the chunk kernels' two arms; k_sweep_rows makes the same three
// tests in batches, SWEEP_LOOK lookups in flight (its `flush`).
template <class V> __device__ __forceinline__ bool sweep_is_new(const V& v, unsigned ia, const uint4& fa, unsigned xa, unsigned ib)
{
    if (SweepFilter<V>::on && !collision_filter_pass(fa, sweep_filter_of(v, ib))) return false;
    if (SweepExclude<V>::on && xa && sweep_excluded(v, ia, ib)) return false;
    return !ps_contains(v.table, v.mask, ps_ordered_key(ia, ib));
}

constexpr int SWEEP_CAND = 16;      // y-overlapping candidates a row can hold before it must look them up in the pair set
constexpr int SWEEP_LOOK = 8;        // lookups a row keeps in flight
constexpr int SWEEP_GROUP = 8;       // candidates the wave reads from its staged block per step of its walk

// first position j > i with minx[j] > maxx (entries sorted by minx)
__device__ __forceinline__ int scan_end(const float4* __restrict__ entries, int n, int i, float maxx)
{
    int lo = i + 1, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (entries[mid].x > maxx) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// One sorted row per lane, and the wave walks the CANDIDATES together: lane l owns row i0 + l, the wave steps through positions
// c = i0 + 1, i0 + 2, ... and every lane whose row has begun (c > its row) and not ended (minx[c] <= its maxx) tests the SAME
// candidate — whose record is therefore one scalar load for the wave (eight per fetch) instead of a 16-byte gather per lane.
// (Round 3 let every lane fetch its own window, eight loads in flight per lane: 20 M tests were 320 MB through the L1s and a
// row's scan a chain of dependent gathers — 44 us at cfg 2, 95 us at cfg 4.)  A lane sees its candidates in the same increasing
// order as before, so counts, caches and the emission order are unchanged.
// (Round 6 built the transposed walk — the lanes hold a block of 64 CANDIDATES in registers, the wave tests them against one row after
//  the other, row data by v_readlane, ballots give tests / overlaps / the row's end, the lane that holds an overlapping candidate looks
//  the pair up — byte-equal lists and counts, and SLOWER: 50.1 against 38.7 us at cfg 2, 103.9 against 80.6 at cfg 4.  Both walks do
//  one 64-wide step per (row block, candidate) resp. (row, candidate block) and the triangle of a tie column half fills either; the
//  transposed step is ~27 mostly scalar instructions, this one ~15 vector ones.  tools/probe/sweep_tiles.hip.txt keeps it.)
#define PHX_SWEEP_WAVE_SYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)

template <bool EMIT, class V>
__global__ void __launch_bounds__(256) k_sweep_rows(V v, const unsigned* __restrict__ row_offset, uint2* __restrict__ out, unsigned total)
{
    // EMIT = false: the count pass (also remembers each row's first ROW_CACHE new partners).
    // EMIT = true : rescans ONLY the rows that found more than ROW_CACHE new pairs; all other rows are emitted from the
    //               cache by k_emit_cached without touching the entries or the pair set again.
    __shared__ unsigned cand[SWEEP_CAND][256];          // per lane: positions of the candidates that overlap in y, not looked up yet
    __shared__ float4 stage[4][2][64];                  // per wave: the block of 64 candidates under test, and the next one
    unsigned long long tests = 0, overlaps = 0;
    const int lane = threadIdx.x & 63;
    for (int base = blockIdx.x * blockDim.x + (threadIdx.x & ~63); base < v.n; base += gridDim.x * blockDim.x) {      // (wave-uniform)
        const int i = base + lane;
        const bool in_range = i < v.n;
        const float4 a = in_range ? v.entries[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        // a hub row (more than HUB_LEN candidates) is recognised by one probe: entries are sorted by minx, so the row is a
        // hub iff the candidate HUB_LEN places ahead still starts at or before this row's maxx.  Only hub rows pay the
        // binary search for their end; every other row finds it by scanning (ref: Collider.cpp:300-303 breaks the same way).
        const bool hub = in_range && i + 1 + HUB_LEN < v.n && !(v.entries[i + 1 + HUB_LEN].x > a.y);
        if (!EMIT) {
            // hand a hub row to the chunk kernels: its chunks sit contiguously and in j order in the list.  The row's lane finds the
            // end and takes the list positions; the WAVE writes the descriptors (the ground row of the 1M-box scene is 1954 of them).
            int end = 0, nc = 0, first = 0;
            if (hub) {
                end = scan_end(v.entries, v.n, i, a.y);
                const int len = end - i - 1;
                nc = (len + HUB_CHUNK - 1) / HUB_CHUNK;
                first = atomicAdd(v.n_chunks, nc);
                v.row_count[i] = 0;
                tests += (unsigned long long)len;
            }
            for (unsigned long long hubs = __ballot(hub); hubs; hubs &= hubs - 1ull) {
                const int l = __builtin_ctzll(hubs);
                const int hi = __shfl(i, l), hend = __shfl(end, l), hnc = __shfl(nc, l), hfirst = __shfl(first, l);
                for (int k = lane; k < hnc && hfirst + k < v.chunk_cap; k += 64)
                    v.chunks[hfirst + k] = make_int4(hi, hi + 1 + k * HUB_CHUNK, min(hend, hi + 1 + (k + 1) * HUB_CHUNK), hfirst);
            }
        }
        bool scanning = in_range && !hub;
        const unsigned dst = EMIT && scanning ? row_offset[i] : 0u;
        if (EMIT && scanning) {
            const unsigned next = i + 1 < v.n ? row_offset[i + 1] : total;
            if (next - dst <= (unsigned)ROW_CACHE) scanning = false;      // emitted from the cache
        }
        const unsigned ia = scanning ? v.idx[i] : 0u;
        const uint4 fa = scanning ? sweep_filter_of(v, ia) : make_uint4(0u, 0u, 0u, 0u);      // (the row's filter: once per row)
        const unsigned xa = scanning ? sweep_member_of(v, ia) : 0u;                           // (the row's exclusion word: once per row)
        unsigned found = 0;
        // The candidates that overlap in y are only COLLECTED by the scan (their positions, in j order, in LDS); the pair-set
        // lookups — two dependent memory round trips each — are made afterwards, all in flight together.  Done inside the scan
        // they were its whole cost: some lane of the wave hits an overlap in almost every step, and the wave waits for it.
        int ncand = 0;
        auto flush = [&]() {
            for (int h = 0; h < ncand; h += SWEEP_LOOK) {          // SWEEP_LOOK lookups in flight at a time
                unsigned ib[SWEEP_LOOK];
                unsigned long long first[SWEEP_LOOK];
#pragma unroll
                for (int k = 0; k < SWEEP_LOOK; ++k) ib[k] = h + k < ncand ? v.idx[cand[h + k][threadIdx.x]] : 0u;
                unsigned pass = ~0u;                               // bit k: candidate h + k passes the collision filter (always, unfiltered)
                if constexpr (SweepFilter<V>::on) {
                    pass = 0u;
#pragma unroll
                    for (int k = 0; k < SWEEP_LOOK; ++k)
                        if (h + k < ncand && collision_filter_pass(fa, sweep_filter_of(v, ib[k]))) pass |= 1u << k;
                }
                // (the exclusion probes' home slots are loaded here, in front of the pair-set lookups' and in flight with them, and looked
                //  at behind them; a row of a body in no excluded pair — xa == 0 — loads none)
                unsigned long long xfirst[SWEEP_LOOK];
                if constexpr (SweepExclude<V>::on) {
#pragma unroll
                    for (int k = 0; k < SWEEP_LOOK; ++k)
                        xfirst[k] = xa && h + k < ncand && ((pass >> k) & 1u) ? v.excl.table[ps_hash(ps_unordered_key(ia, ib[k])) & v.excl.mask] : PS_EMPTY;
                }
#pragma unroll
                for (int k = 0; k < SWEEP_LOOK; ++k) first[k] = h + k < ncand && ((pass >> k) & 1u) ? v.table[ps_hash(ps_ordered_key(ia, ib[k])) & v.mask] : 0ull;
                if constexpr (SweepExclude<V>::on) {
#pragma unroll
                    for (int k = 0; k < SWEEP_LOOK; ++k) {
                        if (xfirst[k] == PS_EMPTY) continue;       // nothing at the home slot, or no probe: not excluded
                        const unsigned long long xkey = ps_unordered_key(ia, ib[k]);
                        if (xfirst[k] == xkey || ps_contains(v.excl.table, v.excl.mask, xkey)) pass &= ~(1u << k);      // excluded: what a filtered candidate is
                    }
                }
#pragma unroll
                for (int k = 0; k < SWEEP_LOOK; ++k) {
                    if (h + k >= ncand) break;
                    if (!((pass >> k) & 1u)) continue;             // rejected by the filter (or excluded): no lookup, not new
                    const unsigned long long key = ps_ordered_key(ia, ib[k]);
                    bool present = first[k] == key;
                    if (!present && first[k] != PS_EMPTY) present = ps_contains(v.table, v.mask, key);       // a collision at the home slot: walk on
                    if (!present) {
                        if (EMIT) out[dst + found] = make_uint2(ia, ib[k]);
                        else if (found < (unsigned)ROW_CACHE) v.row_cache[(size_t)i * ROW_CACHE + found] = ib[k];
                        ++found;
                    }
                }
            }
            ncand = 0;
        };
        // the wave's walk, 64 candidates per fetch: lane l fetches record c + l (one coalesced load for the wave), the block waits in
        // LDS, and the wave reads it record by record at a uniform address (a broadcast) — the NEXT block's fetch is already in
        // flight while this one is tested, so the walk never waits for memory: a fetch per 8 candidates (scalar loads, or eight
        // gathers per lane before that) was a ~1 us round trip each, 30 of them in a row per wave.
        int len = 0;
        bool ended = !scanning;
        int ended_w = scanning ? 0 : -1;
        const int c0 = __builtin_amdgcn_readfirstlane(base) + 1;
        float4* my_stage = &stage[threadIdx.x >> 6][0][0];
        float4 nxt = v.entries[min(c0 + lane, v.n - 1)];
        int buf = 0;
        for (int c = c0; c < v.n && __ballot(!ended); c += 64) {
            my_stage[buf * 64 + lane] = nxt;
            if (c + 64 < v.n) nxt = v.entries[min(c + 64 + lane, v.n - 1)];
            PHX_SWEEP_WAVE_SYNC();
            const float4* blockp = my_stage + buf * 64;
            const int rel = i - c;                                   // candidate g of this block lies behind my row iff g > rel
            for (int g = 0; g < 64 && c + g < v.n && __ballot(!ended); g += SWEEP_GROUP) {
                // (the list holds SWEEP_CAND = 2 x SWEEP_GROUP positions and is emptied HERE, once per group, when the next eight might
                //  not fit: emptied where it fills up — inside the unrolled tests — the lookups' code stood eight times in the hot loop)
                if (ncand > SWEEP_CAND - SWEEP_GROUP) flush();
                float4 b[SWEEP_GROUP];
#pragma unroll
                for (int k = 0; k < SWEEP_GROUP; ++k) b[k] = blockp[g + k];
                // The tests are PREDICATED, not branched: a CU's waves share one scalar unit, and a branch is three or four scalar
                // instructions (compare-to-mask, s_and_saveexec, s_cbranch, the exec restore) — twelve waves walking 260 candidates
                // with three nested branches each were bound by it (~20 us of the kernel's 45).  Lane state lives in VGPRs as
                // all-ones / zero words; the only branch left is 'some lane of the wave overlaps this candidate in y'.
#pragma unroll
                for (int k = 0; k < SWEEP_GROUP; ++k) {
                    const int j = c + g + k;
                    const int started = (rel - (g + k)) >> 31;                          // -1 iff this candidate lies behind my row (j > i)
                    const int in_list = (j - v.n) >> 31;                                // -1 iff j < n
                    const int beyond = b[k].x > a.y ? -1 : 0;                           // ref: Collider.cpp:300-303: the row ends here
                    const int live = started & in_list & ~ended_w;
                    ended_w |= live & beyond;
                    const int tested = live & ~beyond;
                    len -= tested;
                    const int ov = (fabsf(b[k].z - a.z) <= a.w + b[k].w ? -1 : 0) & tested;
                    if (__any(ov)) {
                        if (ov) {
                            if (!EMIT) ++overlaps;
                            cand[ncand++][threadIdx.x] = (unsigned)j;
                        }
                    }
                }
                ended = ended_w != 0;
            }
            buf ^= 1;
        }
        if (scanning) {
            flush();
            if (!EMIT) { v.row_count[i] = found; tests += (unsigned long long)len; if (found > (unsigned)ROW_CACHE) *v.cache_overflow = 1; }
        }
    }
    if (!EMIT) {
        for (int off = 32; off > 0; off >>= 1) { tests += __shfl_down(tests, off); overlaps += __shfl_down(overlaps, off); }
        __shared__ unsigned long long part[2][4];
        if ((threadIdx.x & 63) == 0) { part[0][threadIdx.x >> 6] = tests; part[1][threadIdx.x >> 6] = overlaps; }
        __syncthreads();
        if (threadIdx.x < 2) {                             // one atomic per workgroup per counter, 64 slots
            const unsigned long long t = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
            if (t) atomicAdd(&v.counters[2 * (blockIdx.x % STAT_SLOTS) + threadIdx.x], t);
        }
    }
}
// emit pass for every row with at most ROW_CACHE new pairs: straight from what the count pass remembered
__device__ __forceinline__ void emit_cached_rows(const SweepView& v, const unsigned* __restrict__ row_offset, uint2* __restrict__ out, unsigned total, int block, int blocks)
{
    for (int i = block * (int)blockDim.x + (int)threadIdx.x; i < v.n; i += blocks * (int)blockDim.x) {
        const unsigned dst = row_offset[i];
        const unsigned count = (i + 1 < v.n ? row_offset[i + 1] : total) - dst;
        if (count == 0 || count > (unsigned)ROW_CACHE) continue;     // nothing new, or a rescanned row
        // a hub row's pairs are emitted by its chunks and its row_cache entries were never written: skip it explicitly (the
        // same one-probe test as the count pass) instead of relying on k_sweep_chunks<true> overwriting the slots afterwards
        if (i + 1 + HUB_LEN < v.n && !(v.entries[i + 1 + HUB_LEN].x > v.entries[i].y)) continue;
        const unsigned ia = v.idx[i];
        for (unsigned k = 0; k < count; ++k) out[dst + k] = make_uint2(ia, v.row_cache[(size_t)i * ROW_CACHE + k]);
    }
}

// one workgroup per hub chunk; tiles of 256 candidates in j order, a running base keeps the emission order
template <bool EMIT, class V>
__device__ __forceinline__ void sweep_chunks(const V& v, const unsigned* __restrict__ row_offset, uint2* __restrict__ out, int block, int blocks)
{
    __shared__ unsigned wave_cnt[4];
    __shared__ unsigned running;
    const int total = min(*v.n_chunks, v.chunk_cap);
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long overlaps_all = 0;
    for (int c = block; c < total; c += blocks) {
        const int4 ch = v.chunks[c];
        const float4 a = v.entries[ch.x];
        const unsigned ia = v.idx[ch.x];
        const uint4 fa = sweep_filter_of(v, ia);
        const unsigned xa = sweep_member_of(v, ia);
        unsigned long long overlaps = 0;
        if constexpr (!EMIT) {
            // the count pass only wants the chunk's number of new pairs: every lane counts its own candidates over all tiles (their
            // loads and lookups in flight together) and the workgroup adds up once — no per-tile ordering, one barrier pair per chunk
            unsigned mine = 0;
            for (int j = ch.y + (int)threadIdx.x; j < ch.z; j += 256) {
                const float4 b = v.entries[j];
                if (fabsf(b.z - a.z) <= a.w + b.w) {
                    ++overlaps;
                    if (sweep_is_new(v, ia, fa, xa, v.idx[j])) ++mine;
                }
            }
            for (int off = 32; off > 0; off >>= 1) mine += __shfl_down(mine, off);
            if (lane == 0) wave_cnt[wave] = mine;
            __syncthreads();
            if (threadIdx.x == 0) v.chunk_count[c] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            overlaps_all += overlaps;
            __syncthreads();
            continue;
        }
        if (threadIdx.x == 0) running = row_offset[ch.x] + v.chunk_count[c];
        __syncthreads();
        for (int j0 = ch.y; j0 < ch.z; j0 += 256) {
            const int j = j0 + threadIdx.x;
            bool hit = false;
            unsigned ib = 0;
            if (j < ch.z) {
                const float4 b = v.entries[j];
                if (fabsf(b.z - a.z) <= a.w + b.w) {
                    ib = v.idx[j];
                    ++overlaps;
                    hit = sweep_is_new(v, ia, fa, xa, ib);
                }
            }
            const unsigned long long bal = __ballot(hit);
            if (lane == 0) wave_cnt[wave] = (unsigned)__popcll(bal);
            __syncthreads();
            unsigned before = 0;
            for (int w = 0; w < wave; ++w) before += wave_cnt[w];
            const unsigned base = running;
            if (EMIT && hit) out[base + before + (unsigned)__popcll(bal & ((1ull << lane) - 1ull))] = make_uint2(ia, ib);
            __syncthreads();
            if (threadIdx.x == 0) running = base + wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
            __syncthreads();
        }
        __syncthreads();
    }
    if (!EMIT) {                                           // one statistics atomic per wave for the whole launch, not per chunk
        for (int off = 32; off > 0; off >>= 1) overlaps_all += __shfl_down(overlaps_all, off);
        if (lane == 0 && overlaps_all) atomicAdd(&v.counters[2 * ((block * 4 + wave) % STAT_SLOTS) + 1], overlaps_all);
    }
}

// the count pass over the hub rows' chunks
template <class V>
__global__ void __launch_bounds__(256) k_sweep_chunks_count(V v) { sweep_chunks<false>(v, nullptr, nullptr, (int)blockIdx.x, (int)gridDim.x); }

// The emit pass, ONE launch: the first `row_blocks` workgroups emit the ordinary rows' new pairs from what the count pass remembered,
// the others the hub rows' chunks — different rows, different places in the list (two launches of ~5 us each at the dispatch floor).
template <class V>
__global__ void __launch_bounds__(256) k_emit_pairs(V v, const unsigned* __restrict__ row_offset, uint2* __restrict__ out, unsigned total, int row_blocks)
{
    if ((int)blockIdx.x < row_blocks) emit_cached_rows(v, row_offset, out, total, (int)blockIdx.x, row_blocks);
    else sweep_chunks<true>(v, row_offset, out, (int)blockIdx.x - row_blocks, (int)gridDim.x - row_blocks);
}

// per hub row: chunk counts -> chunk bases inside the row, row_count[row] = sum.  A row's chunks are contiguous in the
// list, so differences of the exclusive scan of the counts give both.  The list is short (the ground row of the 200k-box
// scene is 391 chunks, of the 1M-box scene 1954), so ONE workgroup scans it tile by tile with a running carry and then takes the differences — one
// dispatch where a copy, a second copy, a scan and a difference kernel used to be four.
__global__ void __launch_bounds__(1024) k_chunk_bases(SweepView v, unsigned* __restrict__ scanned)
{
    __shared__ unsigned lds[16];
    __shared__ unsigned tot;
    const int total = min(*v.n_chunks, v.chunk_cap);
    unsigned carry = 0;
    for (int tile = 0; tile < total; tile += 1024) {
        const int c = tile + (int)threadIdx.x;
        const unsigned mine = c < total ? v.chunk_count[c] : 0u;
        const unsigned ex = block_exclusive_scan_1024(mine, lds, threadIdx.x == 0 ? &tot : nullptr);
        if (c < total) scanned[c] = carry + ex;
        __syncthreads();
        carry += tot;
        __syncthreads();
    }
    __threadfence_block();
    __syncthreads();
    for (int c = threadIdx.x; c < total; c += 1024) {
        const int4 ch = v.chunks[c];
        const unsigned count = v.chunk_count[c];
        const bool last = (c + 1 == total) || v.chunks[c + 1].x != ch.x;
        if (last) v.row_count[ch.x] = scanned[c] + count - scanned[ch.w];
    }
    __syncthreads();                                                        // every count has been read: now overwrite them with the bases
    for (int c = threadIdx.x; c < total; c += 1024) v.chunk_count[c] = scanned[c] - scanned[v.chunks[c].w];
}

__global__ void __launch_bounds__(256) k_entries_to_aos(const float4* __restrict__ entries, const unsigned* __restrict__ keys,
                                                        const unsigned* __restrict__ idx, int n,
                                                        phx_broadphase_entry* __restrict__ out_entries, phx_sort_entry* __restrict__ out_sorted)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 e = entries[i];
        out_entries[i].minx = e.x; out_entries[i].maxx = e.y; out_entries[i].centery = e.z; out_entries[i].extenty = e.w;
        out_entries[i].index = idx[i];
        out_sorted[i].value = keys[i]; out_sorted[i].index = idx[i];
    }
}

} // namespace phx
