// query.hip — the World's queries (include/phyx_amd.h, QUERIES; kernels in query_kernels.h).  Everything is queued on the world's
// stream; the AABB query reads its per-query counts back once (the caller's offsets, and the size of the fill) and its hits at the end.
#include "query.h"
#include "query_kernels.h"
#include "device_radix.h"

#include <algorithm>
#include <type_traits>

static_assert(sizeof(phx_ray_hit) == 24, "phx_ray_hit is 24 bytes (include/phyx_amd.h)");
static_assert(sizeof(phx_shape_hit) == 16, "phx_shape_hit is 16 bytes (include/phyx_amd.h)");
static_assert(sizeof(phx_near_hit) == 24, "phx_near_hit is 24 bytes (include/phyx_amd.h)");

namespace phx {

// tiles of one scan launch (gridDim.y): with up to 2048 body workgroups of 256 lanes a launch stays under 2^31 work-items
constexpr int Q_MAX_TILES = 4096;
// workgroups of the grid-strided per-query launches (4 queries per workgroup in k_qtree, 1 in k_qsort_segments)
static inline int qtree_grid(int count) { return std::max(1, std::min(div_up(count, 4), 1 << 20)); }
// the scan's per-query launches over n bodies: launch(q0, grid) for each run of at most Q_MAX_TILES tiles of queries
template <class Launch>
static void scan_in_chunks(int n, int count, Launch launch)
{
    for (int q0 = 0; q0 < count; q0 += Q_MAX_TILES * Q_TILE) launch(q0, dim3(stream_grid(n), std::min(div_up(count - q0, Q_TILE), Q_MAX_TILES)));
}

// f(std::integral_constant<int, CAPS>): the kernels' polygon instantiations (2) for a world in which a polygon was named, the capsule
// instantiations (1) for one in which a capsule was, the plain ones (0) otherwise
// (query_kernels.h q_kind).  A kernel that never reads the kinds (AABBs, oriented boxes, box casts) has the plain one alone.
template <class F>
static void q_caps(const WorldBodies& w, F f)
{
    if (w.polys) f(std::integral_constant<int, 2>{});                       // (the polygon instantiations hold the capsule predicates too)
    else if (w.capsules) f(std::integral_constant<int, 1>{});
    else f(std::integral_constant<int, 0>{});
}

int DeviceQuery::configure_from_env()
{
    PHX_TRY(path_from_env("PHX_QUERY_PATH", &forced_));
    long q = 0;
    const char* c = nullptr;
    const EnvInt got = int_from_env("PHX_QUERY_SCAN_CHUNK", &q, &c);
    if (got == ENV_UNSET) return PHX_OK;
    if (got == ENV_MALFORMED || q < Q_TILE || q % Q_TILE) { set_error("PHX_QUERY_SCAN_CHUNK=%s: expected a positive multiple of %d", c, Q_TILE); return PHX_ERR_INVALID; }
    scan_chunk_ = (int)std::min<long>(q, (long)Q_MAX_TILES * Q_TILE);
    return PHX_OK;
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
int DeviceQuery::ensure_index(const WorldBodies& w, int n, unsigned long long epoch, hipStream_t s)
{
    if (index_.current(epoch, n)) return PHX_OK;
    index_.stale();
    levels_ = 0;
    if (n > 0) {
        PHX_TRY(sort_.reserve(n)); PHX_TRY(hist_.reserve(radix_hist_words(n))); PHX_TRY(bounds_.reserve(4));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bounds_.p), 0xFFFFFFFFu, 2, s));
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(bounds_.p + 2), 0u, 2, s));
        hipLaunchKernelGGL(k_qcentre_bounds, dim3(stream_grid(n)), dim3(256), 0, s, (const float4*)w.aabb, n, bounds_.p);
        hipLaunchKernelGGL(k_qmorton, dim3(stream_grid(n)), dim3(256), 0, s, (const float4*)w.aabb, n, (const unsigned*)bounds_.p, sort_.keys(), sort_.vals());
        PHX_HIP(hipGetLastError());
        PHX_TRY(sort_.sort(n, 32, hist_.p, scan_, s));      // (stable: body order breaks ties)
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
            hipLaunchKernelGGL(k_qnodes, dim3(div_up(level_cnt_[l], 4)), dim3(256), 0, s, src, l == 1 ? sort_.vals() : (const unsigned*)nullptr,
                               level_cnt_[l - 1], nodes_.p + level_off_[l], level_cnt_[l]);
        }
        PHX_HIP(hipGetLastError());
    }
    index_.built(epoch, n);
    return PHX_OK;
}

QTree DeviceQuery::tree(int n) const
{
    QTree t;
    t.nodes = nodes_.p; t.perm = sort_.vals(); t.n = n; t.levels = levels_;
    for (int l = 0; l <= Q_MAX_LEVELS; ++l) { t.off[l] = l <= levels_ ? level_off_[l] : 0; t.cnt[l] = l <= levels_ ? level_cnt_[l] : 0; }
    return t;
}

// ---- points and rays --------------------------------------------------------------------------------------------------------------
int DeviceQuery::points(const WorldBodies& w, int n, unsigned long long epoch, const float* d_pts, int count, int flags, int* d_body, hipStream_t s)
{
    if (count <= 0) return PHX_OK;
    unsigned* out = reinterpret_cast<unsigned*>(d_body);
    if (n == 0 || choose(QUERY_POINTS, count) == PATH_SCAN) {
        PHX_HIP(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(out), 0xFFFFFFFFu, (size_t)count, s));      // (-1: no body)
        if (n) q_caps(w, [&](auto caps) {
            constexpr int C = decltype(caps)::value;
            scan_in_chunks(n, count, [&](int q0, dim3 grid) { hipLaunchKernelGGL((k_qscan_points<C>), grid, dim3(256), 0, s, w, n, d_pts, count, q0, flags, out); });
        });
    } else {
        PHX_TRY(ensure_index(w, n, epoch, s));
        const QTree t = tree(n);
        q_caps(w, [&](auto caps) {
            hipLaunchKernelGGL((k_qtree<QK_POINT, decltype(caps)::value>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_pts, count, flags, out, (unsigned long long*)nullptr,
                               (const unsigned*)nullptr, (int*)nullptr);
        });
    }
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// the overlap lists' entry point, by query shape (the capacity complaint names it)
static constexpr const char* OVERLAP_NAME[3] = {"phx_world_query_aabb", "phx_world_query_boxes", "phx_world_query_circles"};

template <int SHAPE, class Hit>
int DeviceQuery::closest(const WorldBodies& w, int n, unsigned long long epoch, const float* d_queries, int count, int flags, Hit* d_out, hipStream_t s)
{
    if (count <= 0) return PHX_OK;
    PHX_TRY(ray_keys_.reserve((size_t)count));
    constexpr Kind kind = SHAPE == QSHAPE_BOX ? QUERY_CASTS : SHAPE == QSHAPE_DISC ? QUERY_DISC_CASTS : QUERY_RAYS;
    constexpr int tree_kind = SHAPE == QSHAPE_BOX ? QK_CAST : SHAPE == QSHAPE_DISC ? QK_DISC_CAST : QK_RAY;
    const bool scan = n == 0 || choose(kind, count) == PATH_SCAN;
    if (!scan) PHX_TRY(ensure_index(w, n, epoch, s));
    q_caps(w, [&](auto caps) {
        constexpr int C = SHAPE != QSHAPE_BOX ? decltype(caps)::value : 0;      // (a box cast sees every body as its frame box)
        if (scan) {
            hipLaunchKernelGGL(k_qfill_u64, dim3(stream_grid(count)), dim3(256), 0, s, ray_keys_.p, count, ~0ull);
            if (n) scan_in_chunks(n, count, [&](int q0, dim3 grid) { hipLaunchKernelGGL((k_qscan_rays<SHAPE, C>), grid, dim3(256), 0, s, w, n, d_queries, count, q0, flags, ray_keys_.p); });
        } else {
            const QTree t = tree(n);
            hipLaunchKernelGGL((k_qtree<tree_kind, C>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_queries, count, flags, (unsigned*)nullptr, ray_keys_.p,
                               (const unsigned*)nullptr, (int*)nullptr);
        }
        if constexpr (SHAPE != QSHAPE_NONE) hipLaunchKernelGGL((k_qcast_finish<SHAPE, C>), dim3(stream_grid(count)), dim3(256), 0, s, w, d_queries, count, (const unsigned long long*)ray_keys_.p, d_out);
        else hipLaunchKernelGGL((k_qray_finish<C>), dim3(stream_grid(count)), dim3(256), 0, s, w, d_queries, count, (const unsigned long long*)ray_keys_.p, d_out);
    });
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceQuery::rays(const WorldBodies& w, int n, unsigned long long epoch, const float* d_rays, int count, int flags, phx_ray_hit* d_out, hipStream_t s)
{
    return closest<QSHAPE_NONE>(w, n, epoch, d_rays, count, flags, d_out, s);
}

int DeviceQuery::casts(const WorldBodies& w, int n, unsigned long long epoch, const float* d_casts, int count, int flags, phx_shape_hit* d_out, hipStream_t s)
{
    return closest<QSHAPE_BOX>(w, n, epoch, d_casts, count, flags, d_out, s);
}

int DeviceQuery::disc_casts(const WorldBodies& w, int n, unsigned long long epoch, const float* d_casts, int count, int flags, phx_shape_hit* d_out, hipStream_t s)
{
    return closest<QSHAPE_DISC>(w, n, epoch, d_casts, count, flags, d_out, s);
}

// nearest bodies: closest<>'s shape (keys filled or walked, then a finish kernel) with kernels of its own; the scan goes chunk by chunk of
// PHX_QUERY_SCAN_CHUNK queries, as the overlap lists' scan does
int DeviceQuery::near(const WorldBodies& w, int n, unsigned long long epoch, const float* d_queries, int count, int flags, phx_near_hit* d_out, hipStream_t s)
{
    if (count <= 0) return PHX_OK;
    PHX_TRY(ray_keys_.reserve((size_t)count));
    const bool scan = n == 0 || choose(QUERY_NEAR, count) == PATH_SCAN;
    if (!scan) PHX_TRY(ensure_index(w, n, epoch, s));
    q_caps(w, [&](auto caps) {
        constexpr int C = decltype(caps)::value;
        if (scan) {
            hipLaunchKernelGGL(k_qfill_u64, dim3(stream_grid(count)), dim3(256), 0, s, ray_keys_.p, count, ~0ull);
            const int chunk = std::max(Q_TILE, std::min(scan_chunk_, Q_MAX_TILES * Q_TILE) / Q_TILE * Q_TILE);
            for (int q0 = 0; n && q0 < count; q0 += chunk)
                hipLaunchKernelGGL((k_qscan_near<C>), dim3(stream_grid(n), div_up(std::min(chunk, count - q0), Q_TILE)), dim3(256), 0, s, w, n, d_queries, count, q0, flags, ray_keys_.p);
        } else {
            const QTree t = tree(n);
            hipLaunchKernelGGL((k_qtree<QK_NEAR, C>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_queries, count, flags, (unsigned*)nullptr, ray_keys_.p,
                               (const unsigned*)nullptr, (int*)nullptr);
        }
        hipLaunchKernelGGL((k_qnear_finish<C>), dim3(stream_grid(count)), dim3(256), 0, s, w, d_queries, count, (const unsigned long long*)ray_keys_.p, d_out);
    });
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// ---- AABB, oriented-box and circle queries ----------------------------------------------------------------------------------------------------
template <int SHAPE>
int DeviceQuery::overlaps(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                          int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    if (count <= 0 || n == 0) { Listing::none(count, offsets, total); return PHX_OK; }
    constexpr Kind kind = SHAPE == QSHAPE_BOX ? QUERY_SHAPES : SHAPE == QSHAPE_DISC ? QUERY_DISCS : QUERY_BOXES;
    if (choose(kind, count) == PATH_SCAN) return scan_aabb<SHAPE>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    PHX_TRY(ensure_index(w, n, epoch, s));
    return index_aabb<SHAPE>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

int DeviceQuery::aabb(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                      int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    return overlaps<QSHAPE_NONE>(w, n, epoch, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

int DeviceQuery::shapes(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                        int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    return overlaps<QSHAPE_BOX>(w, n, epoch, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

int DeviceQuery::discs(const WorldBodies& w, int n, unsigned long long epoch, const float* d_circles, int count, int flags, int32_t* offsets, int32_t* hits,
                       int hit_cap, int64_t* total, Readback& rb, hipStream_t s)
{
    return overlaps<QSHAPE_DISC>(w, n, epoch, d_circles, count, flags, offsets, hits, hit_cap, total, rb, s);
}

template <int SHAPE>
int DeviceQuery::scan_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                           int64_t* total, Readback& rb, hipStream_t s)
{
    if (SHAPE == QSHAPE_DISC && w.polys) return scan_aabb_as<SHAPE, SHAPE == QSHAPE_DISC ? 2 : 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    if (SHAPE == QSHAPE_DISC && w.capsules) return scan_aabb_as<SHAPE, SHAPE == QSHAPE_DISC ? 1 : 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    return scan_aabb_as<SHAPE, 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

template <int SHAPE, int C>
int DeviceQuery::scan_aabb_as(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                              int64_t* total, Readback& rb, hipStream_t s)
{
    const int bblocks = div_up(n, 256);
    // queries per chunk: the chunk's (query, body block) table stays within 2^26 words and one launch's tiles (PHX_QUERY_SCAN_CHUNK
    // lowers it: tests reach the chunked form on small worlds)
    const int chunk = std::max(Q_TILE, std::min(std::min((1 << 26) / bblocks, Q_MAX_TILES * Q_TILE), scan_chunk_) / Q_TILE * Q_TILE);
    PHX_TRY(list_.room(count));
    PHX_TRY(table_.reserve((size_t)std::min(count, chunk) * (size_t)bblocks));
    PHX_HIP(hipMemsetAsync(list_.counts(), 0, (size_t)count * sizeof(unsigned), s));
    for (int q0 = 0; q0 < count; q0 += chunk) {
        const int nq = std::min(chunk, count - q0);
        hipLaunchKernelGGL((k_qscan_aabb<QS_COUNT, SHAPE, C>), dim3(bblocks, div_up(nq, Q_TILE)), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, list_.counts(), 0u, (int*)nullptr);
    }
    PHX_HIP(hipGetLastError());
    PHX_TRY(list_.settle(OVERLAP_NAME[SHAPE], "hits", count, offsets, hit_cap, total, rb, s));
    if (*total == 0) return PHX_OK;
    PHX_TRY(hits_.reserve((size_t)*total));
    for (int q0 = 0; q0 < count; q0 += chunk) {
        const int nq = std::min(chunk, count - q0), tiles = div_up(nq, Q_TILE);
        if (count > chunk)                                                  // (the table holds the last chunk's counts: count this one again)
            hipLaunchKernelGGL((k_qscan_aabb<QS_RECOUNT, SHAPE, C>), dim3(bblocks, tiles), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, (unsigned*)nullptr, 0u, (int*)nullptr);
        PHX_TRY(device_exclusive_scan(table_.p, nq * bblocks, nullptr, scan_, s));
        hipLaunchKernelGGL((k_qscan_aabb<QS_FILL, SHAPE, C>), dim3(bblocks, tiles), dim3(256), 0, s, w, n, d_boxes, count, q0, flags, bblocks, table_.p, (unsigned*)nullptr,
                           (unsigned)offsets[q0], hits_.p);
    }
    PHX_HIP(hipGetLastError());
    return Listing::deliver(hits, hits_.p, *total, rb, s);
}

template <int SHAPE>
int DeviceQuery::index_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                            int64_t* total, Readback& rb, hipStream_t s)
{
    if (SHAPE == QSHAPE_DISC && w.polys) return index_aabb_as<SHAPE, SHAPE == QSHAPE_DISC ? 2 : 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    if (SHAPE == QSHAPE_DISC && w.capsules) return index_aabb_as<SHAPE, SHAPE == QSHAPE_DISC ? 1 : 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
    return index_aabb_as<SHAPE, 0>(w, n, d_boxes, count, flags, offsets, hits, hit_cap, total, rb, s);
}

template <int SHAPE, int C>
int DeviceQuery::index_aabb_as(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                               int64_t* total, Readback& rb, hipStream_t s)
{
    const QTree t = tree(n);
    PHX_TRY(list_.room_with_segments(count));
    hipLaunchKernelGGL((k_qtree<SHAPE == QSHAPE_BOX ? QK_BOX_COUNT : SHAPE == QSHAPE_DISC ? QK_DISC_COUNT : QK_AABB_COUNT, C>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_boxes, count, flags, list_.counts(), (unsigned long long*)nullptr,
                       (const unsigned*)nullptr, (int*)nullptr);
    PHX_HIP(hipGetLastError());
    PHX_TRY(list_.settle(OVERLAP_NAME[SHAPE], "hits", count, offsets, hit_cap, total, rb, s));
    if (*total == 0) return PHX_OK;
    PHX_TRY(hits_.reserve((size_t)*total));
    PHX_TRY(list_.segments_from_counts(count, scan_, s));
    hipLaunchKernelGGL((k_qtree<SHAPE == QSHAPE_BOX ? QK_BOX_FILL : SHAPE == QSHAPE_DISC ? QK_DISC_FILL : QK_AABB_FILL, C>), dim3(qtree_grid(count)), dim3(256), 0, s, w, t, d_boxes, count, flags, (unsigned*)nullptr, (unsigned long long*)nullptr,
                       list_.segments(), hits_.p);
    // ascending order: short segments in LDS, long ones by the radix sort (31-bit keys: the body indices)
    hipLaunchKernelGGL(k_qsort_segments, dim3(segment_grid(count)), dim3(256), 0, s, list_.segments(), (const unsigned*)list_.counts(), count, hits_.p);
    PHX_HIP(hipGetLastError());
    for (int q = 0; q < count; ++q) {
        const unsigned len = list_.host_count(q);
        if (len <= (unsigned)Q_SORT_MAX) continue;
        PHX_TRY(sort_k1_.reserve(len)); PHX_TRY(sort_v0_.reserve(len)); PHX_TRY(sort_v1_.reserve(len)); PHX_TRY(hist_.reserve(radix_hist_words((int)len)));
        unsigned* seg = reinterpret_cast<unsigned*>(hits_.p) + offsets[q];
        int which = 0;
        PHX_TRY(device_radix_sort_pairs(seg, sort_v0_.p, sort_k1_.p, sort_v1_.p, (int)len, 31, hist_.p, scan_, s, &which));
        if (which) PHX_HIP(hipMemcpyAsync(seg, sort_k1_.p, (size_t)len * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    }
    return Listing::deliver(hits, hits_.p, *total, rb, s);
}

} // namespace phx
