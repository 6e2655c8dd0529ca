// debug_primitives.hip — test entry points of the two device primitives (device_scan.h, device_radix.h): the tests call the
// dispatchers directly, at the sizes where they switch paths, instead of through whatever sizes the features above them reach.
// Host arrays go in and come out; every call allocates, copies and synchronises.  Nothing in the product calls these.
// Beside them, host only: the narrowphase's update_manifold (narrowphase.h) on one pair, so that the CPU suite can hold the C++ the
// device kernel calls to tests/circle_spec.py without a GPU.
#include "common.h"
#include "device_radix.h"
#include "narrowphase.h"

namespace phx {
namespace {

// computed loaders of the scan (device_scan.h): word i comes from a source array of its own
struct DebugLoadWords {
    const unsigned* src;
    static constexpr bool in_place = false;
    __device__ unsigned operator()(int i) const { return src[i]; }
};
// ... with load4, which declines every other 4-word base: both arms of scan_load4 run inside one tile
struct DebugLoadQuads {
    const unsigned* src;
    static constexpr bool in_place = false;
    __device__ unsigned operator()(int i) const { return src[i]; }
    __device__ bool load4(int base, uint4& out) const
    {
        if ((base >> 2) & 1) return false;
        out = make_uint4(src[base], src[base + 1], src[base + 2], src[base + 3]);      // (scalar loads: src may be misaligned)
        return true;
    }
};

struct DebugStream {
    hipStream_t s = nullptr;
    ~DebugStream() { if (s) (void)hipStreamDestroy(s); }
};

constexpr unsigned DEBUG_GUARD = 0xA5A5A5A5u;      // fills every word a scan must not write: the gaps between the scans' ranges
constexpr int DEBUG_GAP = 8;                       // guard words behind each range (before rounding up to 16 bytes)
constexpr long long DEBUG_MAX_WORDS = 1ll << 27;

} // namespace
} // namespace phx

extern "C" {

int phx_debug_scan(int device, const uint32_t* words, const int32_t* counts, int32_t nscans, int32_t loader, int32_t misalign_words,
                   uint32_t initial_epoch, uint32_t* out, uint32_t* totals)
{
    using namespace phx;
    PHX_REQUIRE(nscans >= 0 && (nscans == 0 || (counts && totals)), "phx_debug_scan: null counts / totals");
    PHX_REQUIRE(loader >= 0 && loader <= 2, "phx_debug_scan: loader is 0, 1 or 2");
    PHX_REQUIRE(misalign_words >= 0 && misalign_words <= 3, "phx_debug_scan: misalign_words is 0 .. 3");
    PHX_REQUIRE(initial_epoch < (1u << 30), "phx_debug_scan: the epoch has 30 bits");
    // device layout: scan k's range starts misalign_words behind a 16-byte boundary; guard words fill the rest
    std::vector<size_t> at((size_t)nscans, 0);
    size_t dev_words = 4, host_words = 0;
    int max_count = 0;
    for (int k = 0; k < nscans; ++k) {
        PHX_REQUIRE(counts[k] >= 0, "phx_debug_scan: negative count");
        at[(size_t)k] = dev_words + (size_t)misalign_words;
        dev_words = (at[(size_t)k] + (size_t)counts[k] + DEBUG_GAP + 3) & ~size_t(3);
        host_words += (size_t)counts[k];
        max_count = std::max(max_count, counts[k]);
        PHX_REQUIRE((long long)dev_words <= DEBUG_MAX_WORDS, "phx_debug_scan: too many words");
    }
    PHX_REQUIRE(host_words == 0 || (words && out), "phx_debug_scan: null words / out");
    PHX_TRY(use_device(device));
    DebugStream st;
    PHX_HIP(hipStreamCreate(&st.s));
    DevBuf<unsigned> data, src, tot;
    PHX_TRY(data.reserve(dev_words)); PHX_TRY(tot.reserve((size_t)std::max(nscans, 1)));
    std::vector<unsigned> image(dev_words, DEBUG_GUARD), garbage(dev_words, DEBUG_GUARD);
    for (int k = 0, h = 0; k < nscans; h += counts[k], ++k)
        if (counts[k]) std::memcpy(image.data() + at[(size_t)k], words + h, (size_t)counts[k] * sizeof(unsigned));
    if (loader) {      // the words sit in `src`; `data` starts as guard words all over
        PHX_TRY(src.reserve(dev_words));
        PHX_HIP(hipMemcpyAsync(src.p, image.data(), dev_words * sizeof(unsigned), hipMemcpyHostToDevice, st.s));
        PHX_HIP(hipMemcpyAsync(data.p, garbage.data(), dev_words * sizeof(unsigned), hipMemcpyHostToDevice, st.s));
    } else PHX_HIP(hipMemcpyAsync(data.p, image.data(), dev_words * sizeof(unsigned), hipMemcpyHostToDevice, st.s));
    PHX_HIP(hipMemsetAsync(tot.p, 0xA5, (size_t)std::max(nscans, 1) * sizeof(unsigned), st.s));
    ScanScratch scratch;
    if (initial_epoch) {
        // (an empty scratch starts over at epoch 1 whatever it holds: allocate and clear it as prepare() would, then set the counter)
        PHX_TRY(scratch.state.reserve((size_t)div_up(std::max(max_count, 1), SCAN_TILE) + 1));
        PHX_HIP(hipMemsetAsync(scratch.state.p, 0, scratch.state.cap * sizeof(unsigned long long), st.s));
        scratch.epoch = initial_epoch;
    }
    for (int k = 0; k < nscans; ++k) {
        unsigned* d = data.p + at[(size_t)k];
        if (loader == 0) PHX_TRY(device_exclusive_scan(d, counts[k], tot.p + k, scratch, st.s));
        else if (loader == 1) PHX_TRY(device_exclusive_scan_of(DebugLoadWords{src.p + at[(size_t)k]}, d, counts[k], tot.p + k, scratch, st.s));
        else PHX_TRY(device_exclusive_scan_of(DebugLoadQuads{src.p + at[(size_t)k]}, d, counts[k], tot.p + k, scratch, st.s));
    }
    PHX_HIP(hipMemcpyAsync(image.data(), data.p, dev_words * sizeof(unsigned), hipMemcpyDeviceToHost, st.s));
    if (nscans) PHX_HIP(hipMemcpyAsync(totals, tot.p, (size_t)nscans * sizeof(unsigned), hipMemcpyDeviceToHost, st.s));
    PHX_HIP(hipStreamSynchronize(st.s));
    // nothing outside the ranges was written
    size_t w = 0;
    for (int k = 0, h = 0; k <= nscans; ++k) {
        const size_t stop = k < nscans ? at[(size_t)k] : dev_words;
        for (; w < stop; ++w)
            if (image[w] != DEBUG_GUARD) { set_error("phx_debug_scan: device word %zu outside every scanned range was written (scan %d starts at %zu)", w, k, stop); return PHX_ERR_STATE; }
        if (k == nscans) break;
        if (counts[k]) std::memcpy(out + h, image.data() + w, (size_t)counts[k] * sizeof(unsigned));
        w += (size_t)counts[k];
        h += counts[k];
    }
    return PHX_OK;
}

int phx_debug_radix_sort(int device, const uint32_t* keys, const uint32_t* vals, int32_t n, int32_t bits, uint32_t* keys_out, uint32_t* vals_out,
                         int32_t* which)
{
    using namespace phx;
    PHX_REQUIRE(n >= 0 && (long long)n <= DEBUG_MAX_WORDS, "phx_debug_radix_sort: n out of range");
    PHX_REQUIRE(bits >= 0 && bits <= 32, "phx_debug_radix_sort: bits is 0 .. 32");
    PHX_REQUIRE(which && (n == 0 || (keys && vals && keys_out && vals_out)), "phx_debug_radix_sort: null argument");
    PHX_TRY(use_device(device));
    DebugStream st;
    PHX_HIP(hipStreamCreate(&st.s));
    const size_t room = (size_t)std::max(n, 1), bytes = (size_t)n * sizeof(unsigned);
    DevBuf<unsigned> k0, v0, k1, v1, hist;
    PHX_TRY(k0.reserve(room)); PHX_TRY(v0.reserve(room)); PHX_TRY(k1.reserve(room)); PHX_TRY(v1.reserve(room));
    PHX_TRY(hist.reserve(radix_hist_words(n)));
    if (n) {
        PHX_HIP(hipMemcpyAsync(k0.p, keys, bytes, hipMemcpyHostToDevice, st.s));
        PHX_HIP(hipMemcpyAsync(v0.p, vals, bytes, hipMemcpyHostToDevice, st.s));
    }
    ScanScratch scratch;
    int where = 0;
    PHX_TRY(device_radix_sort_pairs(k0.p, v0.p, k1.p, v1.p, n, bits, hist.p, scratch, st.s, &where));
    if (n) {
        PHX_HIP(hipMemcpyAsync(keys_out, where ? k1.p : k0.p, bytes, hipMemcpyDeviceToHost, st.s));
        PHX_HIP(hipMemcpyAsync(vals_out, where ? v1.p : v0.p, bytes, hipMemcpyDeviceToHost, st.s));
    }
    PHX_HIP(hipStreamSynchronize(st.s));
    *which = where;
    return PHX_OK;
}

int phx_debug_update_manifold(const phx_rigid_body* b1, int32_t kind1, const phx_rigid_body* b2, int32_t kind2, phx_manifold* manifold,
                              phx_contact_point pts[2])
{
    using namespace phx;
    PHX_REQUIRE(b1 && b2 && manifold && pts, "phx_debug_update_manifold: null argument");
    PHX_REQUIRE(kind1 >= PHX_SHAPE_BOX && kind1 <= PHX_SHAPE_CAPSULE && kind2 >= PHX_SHAPE_BOX && kind2 <= PHX_SHAPE_CAPSULE, "phx_debug_update_manifold: a kind is 0, 1 or 2");
    PHX_REQUIRE(manifold->point_count >= 0 && manifold->point_count <= 2, "phx_debug_update_manifold: point_count is 0 .. 2");
    auto body = [](const phx_rigid_body& b, int32_t kind) {
        NpBody n;
        n.pos = v2(b.pos); n.xv = v2(b.xvector); n.yv = v2(b.yvector); n.size = v2(b.geom_size); n.kind = (unsigned)kind; n.poly = nullptr;
        return n;
    };
    // (the instantiation the world would launch: the capsule one only for a pair that holds a capsule)
    if (kind1 == PHX_SHAPE_CAPSULE || kind2 == PHX_SHAPE_CAPSULE) (void)update_manifold<true>(*manifold, body(*b1, kind1), body(*b2, kind2), pts);
    else (void)update_manifold<false>(*manifold, body(*b1, kind1), body(*b2, kind2), pts);
    return PHX_OK;
}

int phx_debug_update_manifold_polygons(const phx_rigid_body* b1, int32_t kind1, const phx_polygon* poly1, const phx_rigid_body* b2, int32_t kind2,
                                       const phx_polygon* poly2, phx_manifold* manifold, phx_contact_point pts[2])
{
    using namespace phx;
    PHX_REQUIRE(b1 && b2 && manifold && pts, "phx_debug_update_manifold_polygons: null argument");
    PHX_REQUIRE(kind1 >= PHX_SHAPE_BOX && kind1 <= PHX_SHAPE_POLYGON && kind2 >= PHX_SHAPE_BOX && kind2 <= PHX_SHAPE_POLYGON, "phx_debug_update_manifold_polygons: a kind is 0 .. 3");
    PHX_REQUIRE((kind1 != PHX_SHAPE_POLYGON || poly1) && (kind2 != PHX_SHAPE_POLYGON || poly2), "phx_debug_update_manifold_polygons: a polygon body needs its polygon");
    PHX_REQUIRE((kind1 != PHX_SHAPE_POLYGON || (poly1->count >= 3 && poly1->count <= PHX_POLYGON_MAX_VERTICES)) &&
                (kind2 != PHX_SHAPE_POLYGON || (poly2->count >= 3 && poly2->count <= PHX_POLYGON_MAX_VERTICES)), "phx_debug_update_manifold_polygons: a vertex count is 3 .. 8");
    PHX_REQUIRE(manifold->point_count >= 0 && manifold->point_count <= 2, "phx_debug_update_manifold_polygons: point_count is 0 .. 2");
    PolyRec r1 = {}, r2 = {};                                               // (the records the set call would store)
    if (kind1 == PHX_SHAPE_POLYGON) r1 = poly_record(*poly1);
    if (kind2 == PHX_SHAPE_POLYGON) r2 = poly_record(*poly2);
    auto body = [](const phx_rigid_body& b, int32_t kind, const PolyRec* rec) {
        NpBody n;
        n.pos = v2(b.pos); n.xv = v2(b.xvector); n.yv = v2(b.yvector); n.size = v2(b.geom_size); n.kind = (unsigned)kind; n.poly = rec;
        return n;
    };
    // (the fourth instantiation: what a world in which a polygon was named launches for every pair)
    (void)update_manifold<true, true>(*manifold, body(*b1, kind1, &r1), body(*b2, kind2, &r2), pts);
    return PHX_OK;
}

int phx_debug_primitive_plan(int32_t bits, int32_t scan_count, int32_t* digit_bits, int32_t* passes, int32_t* scan_single, int32_t* scan_tiles)
{
    using namespace phx;
    PHX_REQUIRE(bits >= 0 && bits <= 32 && scan_count >= 0, "phx_debug_primitive_plan: bits is 0 .. 32, scan_count >= 0");
    const int width = radix_digit_bits(bits);
    if (digit_bits) *digit_bits = width;
    if (passes) *passes = std::max(1, div_up(bits, width));
    if (scan_single) *scan_single = scan_count > 0 && scan_count <= SCAN_SINGLE_MAX;      // (an empty scan launches nothing)
    if (scan_tiles) *scan_tiles = div_up(scan_count, SCAN_TILE);
    return PHX_OK;
}

} // extern "C"
