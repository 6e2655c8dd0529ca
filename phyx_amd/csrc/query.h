// query.h — the World's queries (include/phyx_amd.h, QUERIES): the host side of query_kernels.h.  The World hands over its resident
// arrays, its body count, its geometry epoch and its stream; everything is queued on that stream.  The query index (a 64-wide tree over
// the bodies in Morton order) is built by the first index-path query after the geometry changed and kept while the epoch stays.
// What is left here is the queries' own: the thresholds, the index and its tree, the scan's (query, body block) table and which
// kernels count and fill.  The path choice, the index stamp and the two-pass protocol of the overlap lists are listing.h's.
#pragma once

#include "body_view.h"
#include "listing.h"

#include <cstdint>

namespace phx {

struct QTree;

class DeviceQuery {
public:
    // (BOXES: AABBs; SHAPES: oriented boxes; DISCS: circles)
    enum Kind { QUERY_POINTS = 0, QUERY_RAYS = 1, QUERY_BOXES = 2, QUERY_SHAPES = 3, QUERY_CASTS = 4, QUERY_DISCS = 5, QUERY_DISC_CASTS = 6, QUERY_NEAR = 7 };
    // the scan path answers batches up to this many queries of each kind, the index larger ones: the largest batch size at which
    // tools/query_cost.py measured the scan faster at cfg 2, each call after a step so that the index pays its build (INTEGRATION.md
    // §4b: points 2048 scan / 4096 index, rays 512 / 1024, boxes 1024 / 2048; sizes between two measured ones are not measured)
    // Oriented boxes and box casts take the thresholds of the AABB queries and the rays: they share their data path, and their own
    // crossover was not measured when they were made.  Circles and circle casts take 512, by the rule above:
    // tools/round_query_cost.py measured both with the scan faster at 512 and the index faster at 1024 (Queries: circles).
    // Nearest queries: 1.  tools/near_cost.py measured the scan faster up to 2 048 queries at max_dist 2 and 50 but at a batch of 1 only at
    // FLT_MAX, where every pair is a candidate and the scan has nothing to skip (0.78 ms against the index's 0.38 at 64 queries, 43.6
    // against 1.5 at 65 536): 1 is the largest measured size at which the scan was faster at every max_dist (Queries: nearest).
    static constexpr int SCAN_MAX[8] = {2048, 512, 1024, 1024, 512, 512, 512, 1};

    // PHX_QUERY_PATH=scan|index forces a path; PHX_QUERY_SCAN_CHUNK=q (a multiple of 64) lowers the queries per chunk of the scan path's
    // AABB table and per launch of the nearest scan.  Read when the world is created; any other value is refused (PHX_ERR_INVALID).
    int configure_from_env();
    ReportPath choose(Kind kind, int count) const { return choose_path(forced_, count, SCAN_MAX[kind]); }

    // device inputs and outputs; d_body gets -1 where no body contains the point
    int points(const WorldBodies& w, int n, unsigned long long epoch, const float* d_pts, int count, int flags, int* d_body, hipStream_t s);
    int rays(const WorldBodies& w, int n, unsigned long long epoch, const float* d_rays, int count, int flags, phx_ray_hit* d_out, hipStream_t s);
    // host outputs (offsets: count + 1); waits through `rb`.  PHX_ERR_CAPACITY as phx_world_query_aabb.
    int aabb(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
             int hit_cap, int64_t* total, Readback& rb, hipStream_t s);
    // oriented boxes (8 floats per query) and box casts (11): as aabb and rays
    int shapes(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
               int hit_cap, int64_t* total, Readback& rb, hipStream_t s);
    int casts(const WorldBodies& w, int n, unsigned long long epoch, const float* d_casts, int count, int flags, phx_shape_hit* d_out, hipStream_t s);
    // circles (3 floats per query) and circle casts (6): as shapes and casts
    int discs(const WorldBodies& w, int n, unsigned long long epoch, const float* d_circles, int count, int flags, int32_t* offsets, int32_t* hits,
              int hit_cap, int64_t* total, Readback& rb, hipStream_t s);
    int disc_casts(const WorldBodies& w, int n, unsigned long long epoch, const float* d_casts, int count, int flags, phx_shape_hit* d_out, hipStream_t s);
    // nearest bodies (3 floats per query {p, max_dist}): as rays; the scan's launches hold at most PHX_QUERY_SCAN_CHUNK queries each
    int near(const WorldBodies& w, int n, unsigned long long epoch, const float* d_queries, int count, int flags, phx_near_hit* d_out, hipStream_t s);
    // the index alone (tools/query_cost.py times it): built unless it is current
    int ensure_index(const WorldBodies& w, int n, unsigned long long epoch, hipStream_t s);
    int index_builds() const { return index_.builds(); }

private:
    // SHAPE (query_kernels.h QSHAPE_*): AABBs or rays, oriented boxes, circles
    template <int SHAPE>
    int overlaps(const WorldBodies& w, int n, unsigned long long epoch, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits,
                 int hit_cap, int64_t* total, Readback& rb, hipStream_t s);
    template <int SHAPE>
    int scan_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                  int64_t* total, Readback& rb, hipStream_t s);
    template <int SHAPE>
    int index_aabb(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                   int64_t* total, Readback& rb, hipStream_t s);
    // (C: the kernels' capsule instantiations, for circle queries of a world in which a capsule was named)
    template <int SHAPE, int C>
    int scan_aabb_as(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                     int64_t* total, Readback& rb, hipStream_t s);
    template <int SHAPE, int C>
    int index_aabb_as(const WorldBodies& w, int n, const float* d_boxes, int count, int flags, int32_t* offsets, int32_t* hits, int hit_cap,
                      int64_t* total, Readback& rb, hipStream_t s);
    template <int SHAPE, class Hit>
    int closest(const WorldBodies& w, int n, unsigned long long epoch, const float* d_queries, int count, int flags, Hit* d_out, hipStream_t s);
    // the current index over n bodies, as the kernels take it
    QTree tree(int n) const;

    ReportPath forced_ = PATH_AUTO;
    int scan_chunk_ = INT32_MAX;
    // the index: the bodies in Morton order are sort_.vals()
    IndexStamp index_;
    int levels_ = 0, level_off_[8] = {0}, level_cnt_[8] = {0};
    RadixPairs sort_;
    DevBuf<unsigned> hist_, bounds_;
    DevBuf<float4> nodes_;
    ScanScratch scan_;
    // per-call scratch
    DevBuf<unsigned long long> ray_keys_;
    Listing list_;
    DevBuf<unsigned> table_;
    DevBuf<int> hits_;
    DevBuf<unsigned> sort_k1_, sort_v0_, sort_v1_;
};

} // namespace phx
