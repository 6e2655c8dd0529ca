// query.hip — the World's queries (include/phyx_amd.h, QUERIES; kernels in query_kernels.h).  Everything is queued on the world's
// stream; the AABB query reads its per-query counts back once (the caller's offsets, and the size of the fill) and its hits at the end.
#include "query.h"
#include "query_kernels.h"
#include "device_radix.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

static_assert(sizeof(phx_ray_hit) == 24, "phx_ray_hit is 24 bytes (include/phyx_amd.h)");
static_assert(sizeof(phx_shape_hit) == 16, "phx_shape_hit is 16 bytes (include/phyx_amd.h)");

namespace phx {

static inline int qgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }
// tiles of one scan launch (gridDim.y): with up to 2048 body workgroups of 256 lanes a launch stays under 2^31 work-items
constexpr int Q_MAX_TILES = 4096;
// workgroups of the grid-strided per-query launches (4 queries per workgroup in k_qtree, 1 in k_qsort_segments)
static inline int qtree_grid(int count) { return std::max(1, std::min(div_up(count, 4), 1 << 20)); }
static inline int qsort_grid(int count) { return std::max(1, std::min(count, 1 << 16)); }

int DeviceQuery::configure_from_env()
{
    const char* v = getenv("PHX_QUERY_PATH");
    if (!v || !*v) forced_ = AUTO;
    else if (!std::strcmp(v, "scan")) forced_ = SCAN;
    else if (!std::strcmp(v, "index")) forced_ = INDEX;
    else { set_error("PHX_QUERY_PATH=%s: expected scan or index (or unset)", v); return PHX_ERR_INVALID; }
    const char* c = getenv("PHX_QUERY_SCAN_CHUNK");
    if (c && *c) {
        char* end = nullptr;
        const long q = std::strtol(c, &end, 10);
        if (*end || q < Q_TILE || q % Q_TILE) { set_error("PHX_QUERY_SCAN_CHUNK=%s: expected a positive multiple of %d", c, Q_TILE); return PHX_ERR_INVALID; }
        scan_chunk_ = (int)std::min<long>(q, (long)Q_MAX_TILES * Q_TILE);
    }
    return PHX_OK;
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
int DeviceQuery::ensure_index(const WorldBodies& w, int n, unsigned long long epoch, hipStream_t s)
{
    if (built_ && built_epoch_ == epoch && built_n_ == n) return PHX_OK;
    built_ = false;
    levels_ = 0;
    if (n > 0) {
        PHX_TRY(keys0_.reserve((size_t)n)); PHX_TRY(vals0_.reserve((size_t)n)); PHX_TRY(keys1_.reserve((size_t)n)); PHX_TRY(vals1_.reserve((size_t)n));
        PHX_TRY(hist_.reserve(radix_hist_words(n))); PHX_TRY(bounds_.reserve(4));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bounds_.p), 0xFFFFFFFFu, 2, s));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bounds_.p + 2), 0u, 2, s));
        hipLaunchKernelGGL(k_qcentre_bounds, dim3(qgrid(n)), dim3(256), 0, s, (const float4*)w.aabb, n, bounds_.p);
        hipLaunchKernelGGL(k_qmorton, dim3(qgrid(n)), dim3(256), 0, s, (const float4*)w.aabb, n, (const unsigned*)bounds_.p, keys0_.p, vals0_.p);
        PHX_HIP(hipGetLastError());
        int which = 0;
        PHX_TRY(device_radix_sort_pairs(keys0_.p, vals0_.p, keys1_.p, vals1_.p, n, 32, hist_.p, scan_, s, &which));      // (stable: body order breaks ties)
        perm_ = which ? vals1_.p : vals0_.p;
        int total = 0;
        level_cnt_[0] = n;
        while (levels_ == 0 || level_cnt_[levels_] > 1) {
            if (levels_ == Q_MAX_LEVELS) { set_error("query index: too many levels"); return PHX_ERR_STATE; }
            level_cnt_[levels_ + 1] = div_up(level_cnt_[levels_], Q_FANOUT);
            level_off_[levels_ + 1] = total;
            total += level_cnt_[levels_ + 1];
            ++levels_;
        }
        PHX_TRY(nodes_.reserve((size_t)total));
        for (int l = 1; l <= levels_; ++l) {
            const float4* src = l == 1 ? (const float4*)w.aabb : (const float4*)nodes_.p + level_off_[l - 1];
            hipLaunchKernelGGL(k_qnodes, dim3(div_up(level_cnt_[l], 4)), dim3(256), 0, s, src, l == 1 ? perm_ : (const unsigned*)nullptr,
                               level_cnt_[l - 1], nodes_.p + level_off_[l], level_cnt_[l]);
        }
        PHX_HIP(hipGetLastError());
    }
    built_ = true; built_epoch_ = epoch; built_n_ = n;
    ++builds_;
    return PHX_OK;
}

static QTree make_tree(const float4* nodes, const unsigned* perm, int n, int levels, const int* off, const int* cnt)
{
    QTree t;
    t.nodes = nodes; t.perm = perm; t.n = n; t.levels = levels;
    for (int l = 0; l <= Q_MAX_LEVELS; ++l) { t.off[l] = l <= levels ? off[l] : 0; t.cnt[l] = l <= levels ? cnt[l] : 0; }
    return t;
}

// ---- points and rays --------------------------------------------------------------------------------------------------------------
int DeviceQuery::points(const WorldBodies& w, int n, unsigned long long epoch, const float* d_pts, int count, int flags, int* d_body, hipStream_t s)
{
    if (count <= 0) return PHX_OK;
    unsigned* out = reinterpret_cast<unsigned*>(d_body);
    if (n == 0 || choose(QUERY_POINTS, count) == SCAN) {
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), 0xFFFFFFFFu, (size_t)count, s));      // (-1: no body)
        if (n)
            for (int q0 = 0; q0 < count; q0 += Q_MAX_TILES * Q_TILE)
                hipLaunchKernelGGL(k_qscan_points, dim3(qgrid(n), std::min(div_up(count - q0, Q_TILE), Q_MAX_TILES)), dim3(256), 0, s, w, n, d_pts, count, q0, flags, out);
    } else {
        PHX_TRY(ensure_index(w, n, epoch, s));
        const QTree t = make_tree(nodes_.p, perm_, n, levels_, level_off_, level_cnt_);
        hipLaunchKernelGGL((k_qtree<QK_POINT>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_pts, count, flags, out, (unsigned long long*)nullptr,
                           (const unsigned*)nullptr, (int*)nullptr);
    }
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

template <bool CAST, class Hit>
int DeviceQuery::closest(const WorldBodies& w, int n, unsigned long long epoch, const float* d_queries, int count, int flags, Hit* d_out, hipStream_t s)
{
    if (count <= 0) return PHX_OK;
    PHX_TRY(ray_keys_.reserve((size_t)count));
    if (n == 0 || choose(CAST ? QUERY_CASTS : QUERY_RAYS, count) == SCAN) {
        hipLaunchKernelGGL(k_qfill_u64, dim3(qgrid(count)), dim3(256), 0, s, ray_keys_.p, count, ~0ull);
        if (n)
            for (int q0 = 0; q0 < count; q0 += Q_MAX_TILES * Q_TILE)
                hipLaunchKernelGGL((k_qscan_rays<CAST>), dim3(qgrid(n), std::min(div_up(count - q0, Q_TILE), Q_MAX_TILES)), dim3(256), 0, s, w, n, d_queries, count, q0, flags, ray_keys_.p);
    } else {
        PHX_TRY(ensure_index(w, n, epoch, s));
        const QTree t = make_tree(nodes_.p, perm_, n, levels_, level_off_, level_cnt_);
        hipLaunchKernelGGL((k_qtree<CAST ? QK_CAST : QK_RAY>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_queries, count, flags, (unsigned*)nullptr, ray_keys_.p,
                           (const unsigned*)nullptr, (int*)nullptr);
    }
    if constexpr (CAST) hipLaunchKernelGGL(k_qcast_finish, dim3(qgrid(count)), dim3(256), 0, s, w, d_queries, count, (const unsigned long long*)ray_keys_.p, d_out);
    else hipLaunchKernelGGL(k_qray_finish, dim3(qgrid(count)), dim3(256), 0, s, w, d_queries, count, (const unsigned long long*)ray_keys_.p, d_out);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceQuery::rays(const WorldBodies& w, int n, unsigned long long epoch, const float* d_rays, int count, int flags, phx_ray_hit* d_out, hipStream_t s)
{
    return closest<false>(w, n, epoch, d_rays, count, flags, d_out, s);
}

int DeviceQuery::casts(const WorldBodies& w, int n, unsigned long long epoch, const float* d_casts, int count, int flags, phx_shape_hit* d_out, hipStream_t s)
{
    return closest<true>(w, n, epoch, d_casts, count, flags, d_out, s);
}

// ---- AABB and oriented-box queries ----------------------------------------------------------------------------------------------------
// offsets[] and *total from the per-query counts read back into counts_; *fits: the total fits hit_cap (and so int32)
int DeviceQuery::offsets_from_counts(const char* what, int count, int32_t* offsets, int hit_cap, int64_t* total, bool* fits)
{
    long long run = 0;
    offsets[0] = 0;
    for (int q = 0; q < count; ++q) {
        run += counts_[(size_t)q];
        offsets[q + 1] = run <= (long long)INT32_MAX ? (int32_t)run : INT32_MAX;
    }
    *total = run;
    *fits = run <= (long long)hit_cap;
    if (!*fits) set_error("%s: %lld hits, room for %d", what, run, hit_cap);
    return PHX_OK;
}

template <bool OBB>
int DeviceQuery::overlaps(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                          int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    if (count <= 0 || n == 0) {
        for (int q = 0; q <= std::max(count, 0); ++q) offsets[q] = 0;
        *total = 0;
        return PHX_OK;
    }
    if (choose(OBB ? QUERY_SHAPES : QUERY_BOXES, count) == SCAN) return scan_aabb<OBB>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    PHX_TRY(ensure_index(w, n, epoch, s));
    return index_aabb<OBB>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

int DeviceQuery::aabb(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                      int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    return overlaps<false>(w, n, epoch, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

int DeviceQuery::shapes(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                        int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    return overlaps<true>(w, n, epoch, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

template <bool OBB>
int DeviceQuery::scan_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                           int64_t* total, Readback& rb, hipStream_t s)
{
    const int bblocks = div_up(n, 256);
    // queries per chunk: the chunk's (query, body block) table stays within 2^26 words and one launch's tiles (PHX_QUERY_SCAN_CHUNK
    // lowers it: tests reach the chunked form on small worlds)
    const int chunk = std::max(Q_TILE, std::min(std::min((1 << 26) / bblocks, Q_MAX_TILES * Q_TILE), scan_chunk_) / Q_TILE * Q_TILE);
    PHX_TRY(qcount_.reserve((size_t)count));
    PHX_TRY(table_.reserve((size_t)std::min(count, chunk) * (size_t)bblocks));
    PHX_HIP(hipMemsetAsync(qcount_.p, 0, (size_t)count * sizeof(unsigned), s));
    for (int q0 = 0; q0 < count; q0 += chunk) {
        const int nq = std::min(chunk, count - q0);
        hipLaunchKernelGGL((k_qscan_aabb<QS_COUNT, OBB>), dim3(bblocks, div_up(nq, Q_TILE)), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, qcount_.p, 0u, (int*)nullptr);
    }
    PHX_HIP(hipGetLastError());
    counts_.resize((size_t)count);
    PHX_TRY(rb.add(counts_.data(), qcount_.p, (size_t)count * sizeof(unsigned), s));
    PHX_TRY(rb.wait(s));
    bool fits = false;
    PHX_TRY(offsets_from_counts(OBB ? "phx_world_query_boxes" : "phx_world_query_aabb", count, offsets, hit_cap, total, &fits));
    if (!fits) return PHX_ERR_CAPACITY;
    if (*total == 0) return PHX_OK;
    PHX_TRY(hits_.reserve((size_t)*total));
    for (int q0 = 0; q0 < count; q0 += chunk) {
        const int nq = std::min(chunk, count - q0), tiles = div_up(nq, Q_TILE);
        if (count > chunk)                                                  // (the table holds the last chunk's counts: count this one again)
            hipLaunchKernelGGL((k_qscan_aabb<QS_RECOUNT, OBB>), dim3(bblocks, tiles), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, (unsigned*)nullptr, 0u, (int*)nullptr);
        PHX_TRY(device_exclusive_scan(table_.p, nq * bblocks, nullptr, scan_, s));
        hipLaunchKernelGGL((k_qscan_aabb<QS_FILL, OBB>), dim3(bblocks, tiles), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, (unsigned*)nullptr,
                           (unsigned)offsets[q0], hits_.p);
    }
    PHX_HIP(hipGetLastError());
    PHX_TRY(rb.add(hits, hits_.p, (size_t)*total * sizeof(int), s));
    return rb.wait(s);
}

template <bool OBB>
int DeviceQuery::index_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                            int64_t* total, Readback& rb, hipStream_t s)
{
    const QTree t = make_tree(nodes_.p, perm_, n, levels_, level_off_, level_cnt_);
    PHX_TRY(qcount_.reserve((size_t)count)); PHX_TRY(qseg_.reserve((size_t)count));
    hipLaunchKernelGGL((k_qtree<OBB ? QK_BOX_COUNT : QK_AABB_COUNT>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_boxes, count, flags, qcount_.p, (unsigned long long*)nullptr,
                       (const unsigned*)nullptr, (int*)nullptr);
    PHX_HIP(hipGetLastError());
    counts_.resize((size_t)count);
    PHX_TRY(rb.add(counts_.data(), qcount_.p, (size_t)count * sizeof(unsigned), s));
    PHX_TRY(rb.wait(s));
    bool fits = false;
    PHX_TRY(offsets_from_counts(OBB ? "phx_world_query_boxes" : "phx_world_query_aabb", count, offsets, hit_cap, total, &fits));
    if (!fits) return PHX_ERR_CAPACITY;
    if (*total == 0) return PHX_OK;
    PHX_TRY(hits_.reserve((size_t)*total));
    PHX_HIP(hipMemcpyAsync(qseg_.p, qcount_.p, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    PHX_TRY(device_exclusive_scan(qseg_.p, count, nullptr, scan_, s));
    hipLaunchKernelGGL((k_qtree<OBB ? QK_BOX_FILL : QK_AABB_FILL>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_boxes, count, flags, (unsigned*)nullptr, (unsigned long long*)nullptr,
                       (const unsigned*)qseg_.p, hits_.p);
    // ascending order: short segments in LDS, long ones by the radix sort (31-bit keys: the body indices)
    hipLaunchKernelGGL(k_qsort_segments, dim3(qsort_grid(count)), dim3(256), 0, s, (const unsigned*)qseg_.p, (const unsigned*)qcount_.p, count, hits_.p);
    PHX_HIP(hipGetLastError());
    for (int q = 0; q < count; ++q) {
        const unsigned len = counts_[(size_t)q];
        if (len <= (unsigned)Q_SORT_MAX) continue;
        PHX_TRY(sort_k1_.reserve(len)); PHX_TRY(sort_v0_.reserve(len)); PHX_TRY(sort_v1_.reserve(len)); PHX_TRY(hist_.reserve(radix_hist_words((int)len)));
        unsigned* seg = reinterpret_cast<unsigned*>(hits_.p) + offsets[q];
        int which = 0;
        PHX_TRY(device_radix_sort_pairs(seg, sort_v0_.p, sort_k1_.p, sort_v1_.p, (int)len, 31, hist_.p, scan_, s, &which));
        if (which) PHX_HIP(hipMemcpyAsync(seg, sort_k1_.p, (size_t)len * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    }
    PHX_TRY(rb.add(hits, hits_.p, (size_t)*total * sizeof(int), s));
    return rb.wait(s);
}

} // namespace phx
