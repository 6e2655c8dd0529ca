// contact.hip — the World's contact reports (include/phyx_amd.h, CONTACTS; kernels in contact_kernels.h).  Everything is queued on the
// world's stream; the contacts read their per-listing counts back once (the caller's offsets, and the size of the fill) and the records at
// the end; the events read back their three totals once, then the two lists.
#include "contact.h"
#include "contact_kernels.h"
#include "device_radix.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <utility>

static_assert(sizeof(phx_contact) == 40, "phx_contact is 40 bytes (include/phyx_amd.h)");
static_assert(sizeof(phx_contact_marker) == 24, "phx_contact_marker is 24 bytes (include/phyx_amd.h)");

namespace phx {

static inline int cgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }
static inline int csort_grid(int count) { return std::max(1, std::min(count, 1 << 16)); }
static inline int key_bits(unsigned max_key) { return max_key ? 32 - __builtin_clz(max_key) : 1; }

int DeviceContacts::configure_from_env()
{
    const char* v = getenv("PHX_CONTACT_PATH");
    if (!v || !*v) forced_ = AUTO;
    else if (!std::strcmp(v, "scan")) forced_ = SCAN;
    else if (!std::strcmp(v, "index")) forced_ = INDEX;
    else { set_error("PHX_CONTACT_PATH=%s: expected scan or index (or unset)", v); return PHX_ERR_INVALID; }
    const char* c = getenv("PHX_CONTACT_SCAN_CHUNK");
    if (c && *c) {
        char* end = nullptr;
        const long q = std::strtol(c, &end, 10);
        if (*end || q < 1 || q > C_CHUNK_MAX) { set_error("PHX_CONTACT_SCAN_CHUNK=%s: expected 1 .. %d", c, C_CHUNK_MAX); return PHX_ERR_INVALID; }
        scan_chunk_ = (int)q;
    }
    return PHX_OK;
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
int DeviceContacts::ensure_index(const ContactCache& c, unsigned long long epoch, hipStream_t s)
{
    if (built_ && built_epoch_ == epoch && built_n_ == c.n) return PHX_OK;
    built_ = false;
    PHX_TRY(offsets_.reserve((size_t)c.n + 1));
    PHX_HIP(hipMemsetAsync(offsets_.p, 0, ((size_t)c.n + 1) * sizeof(unsigned), s));
    const int ne = 2 * c.nm;
    entries_ = nullptr;
    if (ne) {
        PHX_TRY(keys0_.reserve((size_t)ne)); PHX_TRY(vals0_.reserve((size_t)ne)); PHX_TRY(keys1_.reserve((size_t)ne)); PHX_TRY(vals1_.reserve((size_t)ne));
        PHX_TRY(hist_.reserve(radix_hist_words(ne)));
        hipLaunchKernelGGL(k_cidx_entries, dim3(cgrid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, keys0_.p, vals0_.p, offsets_.p);
        PHX_HIP(hipGetLastError());
        const int bits = key_bits((unsigned)c.n - 1u);
        // (stable passes over entries made in manifold order: by the other body, then by the entry's body)
        int which = 0;
        PHX_TRY(device_radix_sort_pairs(keys0_.p, vals0_.p, keys1_.p, vals1_.p, ne, bits, hist_.p, scan_, s, &which));
        unsigned* sorted = which ? vals1_.p : vals0_.p;
        unsigned* spare_v = which ? vals0_.p : vals1_.p;
        unsigned* k_in = which ? keys0_.p : keys1_.p;               // (the first pass's keys are spent: both key buffers are free)
        unsigned* k_out = which ? keys1_.p : keys0_.p;
        hipLaunchKernelGGL(k_cidx_body_keys, dim3(cgrid(ne)), dim3(256), 0, s, (const phx_manifold*)c.manifolds, (const unsigned*)sorted, ne, k_in);
        PHX_HIP(hipGetLastError());
        PHX_TRY(device_radix_sort_pairs(k_in, sorted, k_out, spare_v, ne, bits, hist_.p, scan_, s, &which));
        entries_ = which ? spare_v : sorted;
    }
    PHX_TRY(device_exclusive_scan(offsets_.p, c.n + 1, nullptr, scan_, s));      // (per-body counts -> CSR offsets; [n] = 2 nm)
    built_ = true; built_epoch_ = epoch; built_n_ = c.n;
    ++builds_;
    return PHX_OK;
}

// ---- contacts -------------------------------------------------------------------------------------------------------------------
int DeviceContacts::offsets_from_counts(int count, int32_t* offsets, int cap, int64_t* total, bool* fits)
{
    long long run = 0;
    offsets[0] = 0;
    for (int q = 0; q < count; ++q) {
        run += counts_[(size_t)q];
        offsets[q + 1] = run <= (long long)INT32_MAX ? (int32_t)run : INT32_MAX;
    }
    *total = run;
    *fits = run <= (long long)cap;
    if (!*fits) set_error("phx_world_query_contacts: %lld records, room for %d", run, cap);
    return PHX_OK;
}

int DeviceContacts::contacts(const ContactCache& c, unsigned long long epoch, const int* d_bodies, int count, int flags, int32_t* offsets,
                             phx_contact* out, int cap, int64_t* total, Readback& rb, hipStream_t s)
{
    if (count <= 0 || c.nm == 0) {
        for (int q = 0; q <= std::max(count, 0); ++q) offsets[q] = 0;
        *total = 0;
        return PHX_OK;
    }
    if (choose(count) == SCAN) return scan_contacts(c, d_bodies, count, flags, offsets, out, cap, total, rb, s);
    PHX_TRY(ensure_index(c, epoch, s));
    return index_contacts(c, d_bodies, count, flags, offsets, out, cap, total, rb, s);
}

int DeviceContacts::scan_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap,
                                  int64_t* total, Readback& rb, hipStream_t s)
{
    PHX_TRY(qcount_.reserve((size_t)count)); PHX_TRY(qseg_.reserve((size_t)count));
    PHX_HIP(hipMemsetAsync(qcount_.p, 0, (size_t)count * sizeof(unsigned), s));
    for (int q0 = 0; q0 < count; q0 += scan_chunk_)
        hipLaunchKernelGGL((k_cscan<false>), dim3(cgrid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.sleep, c.cps, c.joints, c.nj, d_bodies, q0,
                           std::min(scan_chunk_, count - q0), flags, qcount_.p, (unsigned*)nullptr, (phx_contact*)nullptr);
    PHX_HIP(hipGetLastError());
    counts_.resize((size_t)count);
    PHX_TRY(rb.add(counts_.data(), qcount_.p, (size_t)count * sizeof(unsigned), s));
    PHX_TRY(rb.wait(s));
    bool fits = false;
    PHX_TRY(offsets_from_counts(count, offsets, cap, total, &fits));
    if (!fits) return PHX_ERR_CAPACITY;
    if (*total == 0) return PHX_OK;
    PHX_TRY(recs_.reserve((size_t)*total)); PHX_TRY(sorted_.reserve((size_t)*total));
    PHX_HIP(hipMemcpyAsync(qseg_.p, qcount_.p, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    PHX_TRY(device_exclusive_scan(qseg_.p, count, nullptr, scan_, s));
    // (the cursors start at the segments' offsets: qcount_ becomes them, the counts are on the host)
    PHX_HIP(hipMemcpyAsync(qcount_.p, qseg_.p, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    for (int q0 = 0; q0 < count; q0 += scan_chunk_)
        hipLaunchKernelGGL((k_cscan<true>), dim3(cgrid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.sleep, c.cps, c.joints, c.nj, d_bodies, q0,
                           std::min(scan_chunk_, count - q0), flags, (unsigned*)nullptr, qcount_.p, recs_.p);
    // (the cursors have moved to the segments' ends)
    hipLaunchKernelGGL(k_csort_segments, dim3(csort_grid(count)), dim3(256), 0, s, (const phx_contact*)recs_.p, (const unsigned*)qseg_.p,
                       (const unsigned*)qcount_.p, count, sorted_.p);
    PHX_HIP(hipGetLastError());
    PHX_TRY(rb.add(out, sorted_.p, (size_t)*total * sizeof(phx_contact), s));
    return rb.wait(s);
}

int DeviceContacts::index_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap,
                                   int64_t* total, Readback& rb, hipStream_t s)
{
    PHX_TRY(qcount_.reserve((size_t)count)); PHX_TRY(qseg_.reserve((size_t)count));
    hipLaunchKernelGGL((k_cidx_query<false>), dim3(cgrid(count)), dim3(256), 0, s, c.manifolds, c.mpos, c.sleep, c.cps, c.joints, c.nj, (const unsigned*)offsets_.p,
                       entries_, d_bodies, count, flags, qcount_.p, (const unsigned*)nullptr, (phx_contact*)nullptr);
    PHX_HIP(hipGetLastError());
    counts_.resize((size_t)count);
    PHX_TRY(rb.add(counts_.data(), qcount_.p, (size_t)count * sizeof(unsigned), s));
    PHX_TRY(rb.wait(s));
    bool fits = false;
    PHX_TRY(offsets_from_counts(count, offsets, cap, total, &fits));
    if (!fits) return PHX_ERR_CAPACITY;
    if (*total == 0) return PHX_OK;
    PHX_TRY(recs_.reserve((size_t)*total));
    PHX_HIP(hipMemcpyAsync(qseg_.p, qcount_.p, (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    PHX_TRY(device_exclusive_scan(qseg_.p, count, nullptr, scan_, s));
    hipLaunchKernelGGL((k_cidx_query<true>), dim3(cgrid(count)), dim3(256), 0, s, c.manifolds, c.mpos, c.sleep, c.cps, c.joints, c.nj, (const unsigned*)offsets_.p,
                       entries_, d_bodies, count, flags, (unsigned*)nullptr, (const unsigned*)qseg_.p, recs_.p);
    PHX_HIP(hipGetLastError());
    PHX_TRY(rb.add(out, recs_.p, (size_t)*total * sizeof(phx_contact), s));
    return rb.wait(s);
}

// ---- events ---------------------------------------------------------------------------------------------------------------------
int DeviceContacts::set_baseline(const std::vector<unsigned long long>& keys, hipStream_t s)
{
    base_n_ = 0;
    if (!keys.empty()) {
        PHX_TRY(base_.reserve(keys.size()));
        PHX_HIP(hipMemcpyAsync(base_.p, keys.data(), keys.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        PHX_HIP(hipStreamSynchronize(s));                           // (`keys` belongs to the caller)
    }
    base_n_ = (int)keys.size();
    return PHX_OK;
}

int DeviceContacts::remap_baseline(const int* d_remap, unsigned* d_count, hipStream_t s)
{
    PHX_TRY(base_spare_.reserve(std::max<size_t>((size_t)base_n_, 1)));
    PHX_TRY(ev_pos_.reserve((size_t)base_n_ + 1));
    const CevRemapLoad keep{base_.p, d_remap};
    PHX_TRY(device_exclusive_scan_of(keep, ev_pos_.p, base_n_, d_count, scan_, s));
    if (base_n_) hipLaunchKernelGGL(k_cev_remap, dim3(cgrid(base_n_)), dim3(256), 0, s, keep, base_n_, (const unsigned*)ev_pos_.p, base_spare_.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceContacts::events(const ContactCache& c, int32_t* begin, int begin_cap, int64_t* begin_total, int32_t* end, int end_cap, int64_t* end_total,
                           Readback& rb, hipStream_t s)
{
    const int nm = c.nm;
    const size_t room = (size_t)std::max(nm, 1);
    PHX_TRY(ev_tot_.reserve(4)); PHX_TRY(t_.reserve(room));
    PHX_TRY(ev_pos_.reserve((size_t)std::max(nm, base_n_) + 1));
    PHX_TRY(ev_begin_.reserve(room)); PHX_TRY(ev_end_.reserve(std::max<size_t>((size_t)base_n_, 1)));
    // 1-2. T: the touching manifolds' keys sorted by (body1, body2) (the others carry the sentinel n and sort last), duplicates dropped
    if (nm) {
        PHX_TRY(ev_k0_.reserve(room)); PHX_TRY(ev_v0_.reserve(room)); PHX_TRY(ev_k1_.reserve(room)); PHX_TRY(ev_v1_.reserve(room));
        PHX_TRY(hist_.reserve(radix_hist_words(nm)));
        hipLaunchKernelGGL(k_cev_keys, dim3(cgrid(nm)), dim3(256), 0, s, c.manifolds, nm, (unsigned)c.n, ev_k0_.p, ev_v0_.p);
        PHX_HIP(hipGetLastError());
        const int bits = key_bits((unsigned)c.n);
        int w = 0;
        PHX_TRY(device_radix_sort_pairs(ev_k0_.p, ev_v0_.p, ev_k1_.p, ev_v1_.p, nm, bits, hist_.p, scan_, s, &w));      // by body2
        unsigned* kb[2] = {ev_k0_.p, ev_k1_.p};
        unsigned* vb[2] = {ev_v0_.p, ev_v1_.p};
        unsigned* b1 = vb[w]; unsigned* b2 = kb[w];
        unsigned* b1_spare = kb[w ^ 1]; unsigned* b2_spare = vb[w ^ 1];
        int w2 = 0;
        PHX_TRY(device_radix_sort_pairs(b1, b2, b1_spare, b2_spare, nm, bits, hist_.p, scan_, s, &w2));              // by body1 (stable)
        const unsigned* s1 = w2 ? b1_spare : b1;
        const unsigned* s2 = w2 ? b2_spare : b2;
        const CevUniqueLoad uniq{s1, s2, (unsigned)c.n};
        PHX_TRY(device_exclusive_scan_of(uniq, ev_pos_.p, nm, ev_tot_.p, scan_, s));
        hipLaunchKernelGGL(k_cev_unique, dim3(cgrid(nm)), dim3(256), 0, s, s1, s2, nm, (unsigned)c.n, (const unsigned*)ev_pos_.p, t_.p);
        PHX_HIP(hipGetLastError());
    } else PHX_HIP(hipMemsetAsync(ev_tot_.p, 0, sizeof(unsigned), s));
    // 3. begin = T \ B (one lane per element of T: its size is on the device), end = B \ T
    const CevMissingLoad begins{t_.p, ev_tot_.p, 0u, base_.p, nullptr, (unsigned)base_n_};
    PHX_TRY(device_exclusive_scan_of(begins, ev_pos_.p, nm, ev_tot_.p + 1, scan_, s));
    if (nm) hipLaunchKernelGGL(k_cev_missing, dim3(cgrid(nm)), dim3(256), 0, s, begins, nm, (const unsigned*)ev_pos_.p, ev_begin_.p);
    PHX_HIP(hipGetLastError());
    const CevMissingLoad ends{base_.p, nullptr, (unsigned)base_n_, t_.p, ev_tot_.p, 0u};      // (ev_pos_ again: stream order)
    PHX_TRY(device_exclusive_scan_of(ends, ev_pos_.p, base_n_, ev_tot_.p + 2, scan_, s));
    if (base_n_) hipLaunchKernelGGL(k_cev_missing, dim3(cgrid(base_n_)), dim3(256), 0, s, ends, base_n_, (const unsigned*)ev_pos_.p, ev_end_.p);
    PHX_HIP(hipGetLastError());
    // 4. the one round trip for the totals, then the lists
    unsigned got[3] = {0, 0, 0};
    PHX_TRY(rb.add(got, ev_tot_.p, sizeof got, s));
    PHX_TRY(rb.wait(s));
    *begin_total = got[1];
    *end_total = got[2];
    if ((long long)got[1] > (long long)begin_cap || (long long)got[2] > (long long)end_cap) {
        set_error("phx_world_contact_events: %u begins (room for %d), %u ends (room for %d)", got[1], begin_cap, got[2], end_cap);
        return PHX_ERR_CAPACITY;
    }
    if (got[1]) PHX_TRY(rb.add(begin, ev_begin_.p, (size_t)got[1] * sizeof(int2), s));
    if (got[2]) PHX_TRY(rb.add(end, ev_end_.p, (size_t)got[2] * sizeof(int2), s));
    if (got[1] || got[2]) PHX_TRY(rb.wait(s));
    // 5. B := T
    std::swap(base_, t_);
    base_n_ = (int)got[0];
    return PHX_OK;
}

// ---- markers --------------------------------------------------------------------------------------------------------------------
int DeviceContacts::markers(const ContactCache& c, phx_contact_marker* d_out, hipStream_t s)
{
    if (!c.nm) return PHX_OK;
    hipLaunchKernelGGL(k_cmarkers, dim3(cgrid(2 * c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.cps, d_out);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

} // namespace phx
