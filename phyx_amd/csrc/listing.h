// listing.h — what the World's two report modules (query.h, contact.h) decide alike on the host; no kernel lives here.
//   the path: AUTO / SCAN / INDEX, read from a module's PHX_*_PATH, chosen from the batch size otherwise; the integer knobs;
//   IndexStamp: which (epoch, n) a module's index was built for, and how often it has been built;
//   RadixPairs: the two-plus-two buffers of a radix sort and who holds the sorted pairs (the sort itself: device_radix.h);
//   Listing: the two-pass protocol of phx_world_query_aabb / _boxes / _contacts (include/phyx_amd.h) — one round trip for the per-row
//            counts, from which the caller gets offsets[] and *total even when the records do not fit, and one for the records;
//   the launch grids of the streaming and the per-segment kernels.
#pragma once

#include "common.h"
#include "device_scan.h"

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

namespace phx {

// workgroups of a streaming pass, 256 lanes each (grid-stride beyond 2048 workgroups)
inline int stream_grid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }
// workgroups of a per-segment sort, one segment each (grid-stride beyond 2^16 segments)
inline int segment_grid(int count) { return std::max(1, std::min(count, 1 << 16)); }

// ---- the path ---------------------------------------------------------------------------------------------------------------------
enum ReportPath { PATH_AUTO = 0, PATH_SCAN = 1, PATH_INDEX = 2 };

// `var` = scan | index forces a path, unset or empty leaves the choice to the batch size; any other value is refused
inline int path_from_env(const char* var, ReportPath* forced)
{
    const char* v = getenv(var);
    if (!v || !*v) *forced = PATH_AUTO;
    else if (!std::strcmp(v, "scan")) *forced = PATH_SCAN;
    else if (!std::strcmp(v, "index")) *forced = PATH_INDEX;
    else { set_error("%s=%s: expected scan or index (or unset)", var, v); return PHX_ERR_INVALID; }
    return PHX_OK;
}

// the scan answers batches of up to scan_max rows, the index larger ones
inline ReportPath choose_path(ReportPath forced, int count, int scan_max) { return forced != PATH_AUTO ? forced : (count <= scan_max ? PATH_SCAN : PATH_INDEX); }

// an integer knob: *text is the variable's value (for the caller's message: each knob has its own range and says it its own way)
enum EnvInt { ENV_UNSET, ENV_MALFORMED, ENV_PARSED };      // (UNSET: unset or empty)
inline EnvInt int_from_env(const char* var, long* value, const char** text)
{
    const char* c = *text = getenv(var);
    if (!c || !*c) return ENV_UNSET;
    char* end = nullptr;
    *value = std::strtol(c, &end, 10);
    return *end ? ENV_MALFORMED : ENV_PARSED;
}

// ---- the index stamp --------------------------------------------------------------------------------------------------------------
// A module's index is kept while the World's epoch for it and the body count stay.  A build goes: current()? -> stale() -> queue the
// build -> built(); one that fails in between leaves the index stale.
class IndexStamp {
public:
    bool current(unsigned long long epoch, int n) const { return built_ && epoch_ == epoch && n_ == n; }
    void stale() { built_ = false; }
    void built(unsigned long long epoch, int n) { built_ = true; epoch_ = epoch; n_ = n; ++builds_; }
    int builds() const { return builds_; }

private:
    bool built_ = false;
    unsigned long long epoch_ = 0;
    int n_ = -1, builds_ = 0;
};

// ---- the buffers of a radix sort --------------------------------------------------------------------------------------------------
// The two key buffers and the two value buffers of device_radix_sort_pairs, and who holds what: a producer writes keys() / vals(),
// sort() sorts them, and keys() / vals() are the sorted pairs; the other two buffers are the spares.  A chained sort by a second key
// (stable, so the first order breaks the ties) changes the roles before it sorts again: the new key goes into spare_keys() and
// rekey_from_spare() makes it keys() (the sorted keys are spent), or rekey_by_vals() sorts the pairs the other way round.
// `hist` (radix_hist_words(n) words) stays the caller's: each report module shares one between two sorts.
// sort() is defined in device_radix.h, beside the sort and its kernels: a file that sorts includes it.
struct RadixPairs {
    int reserve(int n)
    {
        for (DevBuf<unsigned>& b : buf_) PHX_TRY(b.reserve((size_t)n));
        return PHX_OK;
    }
    unsigned* keys() const { return buf_[k_].p; }
    unsigned* vals() const { return buf_[v_].p; }
    unsigned* spare_keys() const { return buf_[sk_].p; }
    unsigned* spare_vals() const { return buf_[sv_].p; }
    void rekey_from_spare() { std::swap(k_, sk_); }
    void rekey_by_vals() { std::swap(k_, v_); }
    int sort(int n, int bits, unsigned* hist, ScanScratch& scan_scratch, hipStream_t stream);

private:
    DevBuf<unsigned> buf_[4];
    int k_ = 0, v_ = 1, sk_ = 2, sv_ = 3;
};

// ---- the listing ------------------------------------------------------------------------------------------------------------------
// `count` rows (query boxes, listed bodies), each with a segment of records (hits, contacts) in one output array.  A call goes
//     room -> its own count kernels into counts() -> settle -> [segments_from_counts ->] its own fill kernels -> deliver
// and makes two round trips through the caller's Readback, or one when settle ends the call: with PHX_ERR_CAPACITY (the records do not
// fit; offsets[] and *total are written all the same, include/phyx_amd.h) or with *total == 0 (nothing to fill).
class Listing {
public:
    // the answer without a launch: nothing to ask (count <= 0) or nothing to list
    static void none(int count, int32_t* offsets, int64_t* total)
    {
        for (int q = 0; q <= std::max(count, 0); ++q) offsets[q] = 0;
        *total = 0;
    }

    // ahead of the count kernels: the per-row counts alone / with the segments' starts
    int room(int count) { return qcount_.reserve((size_t)count); }
    int room_with_segments(int count) { PHX_TRY(room(count)); return qseg_.reserve((size_t)count); }
    unsigned* counts() const { return qcount_.p; }
    const unsigned* segments() const { return qseg_.p; }
    // the counts on the host (after settle)
    unsigned host_count(int q) const { return counts_[(size_t)q]; }

    // the one readback of the counts: offsets[] (saturated at INT32_MAX) and *total, then PHX_ERR_CAPACITY unless the total fits `cap`
    // (and so int32).  The caller returns that status, and PHX_OK when *total is 0.
    int settle(const char* what, const char* noun, int count, int32_t* offsets, int cap, int64_t* total, Readback& rb, hipStream_t s)
    {
        counts_.resize((size_t)count);
        PHX_TRY(rb.add(counts_.data(), qcount_.p, (size_t)count * sizeof(unsigned), s));
        PHX_TRY(rb.wait(s));
        long long run = 0;
        offsets[0] = 0;
        for (int q = 0; q < count; ++q) {
            run += counts_[(size_t)q];
            offsets[q + 1] = run <= (long long)INT32_MAX ? (int32_t)run : INT32_MAX;
        }
        *total = run;
        if (run > (long long)cap) { set_error("%s: %lld %s, room for %d", what, run, noun, cap); return PHX_ERR_CAPACITY; }
        return PHX_OK;
    }

    // segments() := the exclusive scan of counts(), on the device
    int segments_from_counts(int count, ScanScratch& scan, hipStream_t s)
    {
        PHX_HIP(hipMemcpyAsync(qseg_.p, qcount_.p, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
        return device_exclusive_scan(qseg_.p, count, nullptr, scan, s);
    }

    // the one readback of the records
    template <class Rec>
    static int deliver(Rec* out, const Rec* d_src, int64_t total, Readback& rb, hipStream_t s)
    {
        PHX_TRY(rb.add(out, d_src, (size_t)total * sizeof(Rec), s));
        return rb.wait(s);
    }

private:
    DevBuf<unsigned> qcount_, qseg_;
    std::vector<unsigned> counts_;
};

} // namespace phx
