// contact.hip — the World's contact reports (include/phyx_amd.h, CONTACTS; kernels in contact_kernels.h).  Everything is queued on the
// world's stream; the contacts read their per-listing counts back once (the caller's offsets, and the size of the fill) and the records at
// the end; the events read back their three totals once, then the two lists.
#include "contact.h"
#include "contact_kernels.h"
#include "device_radix.h"

#include <algorithm>
#include <utility>

static_assert(sizeof(phx_contact) == 40, "phx_contact is 40 bytes (include/phyx_amd.h)");
static_assert(sizeof(phx_contact_marker) == 24, "phx_contact_marker is 24 bytes (include/phyx_amd.h)");

namespace phx {

static inline int key_bits(unsigned max_key) { return max_key ? 32 - __builtin_clz(max_key) : 1; }

int DeviceContacts::configure_from_env()
{
    PHX_TRY(path_from_env("PHX_CONTACT_PATH", &forced_));
    long q = 0;
    const char* c = nullptr;
    const EnvInt got = int_from_env("PHX_CONTACT_SCAN_CHUNK", &q, &c);
    if (got == ENV_UNSET) return PHX_OK;
    if (got == ENV_MALFORMED || q < 1 || q > C_CHUNK_MAX) { set_error("PHX_CONTACT_SCAN_CHUNK=%s: expected 1 .. %d", c, C_CHUNK_MAX); return PHX_ERR_INVALID; }
    scan_chunk_ = (int)q;
    return PHX_OK;
}

// ---- the index ------------------------------------------------------------------------------------------------------------------
int DeviceContacts::ensure_index(const ContactCache& c, unsigned long long epoch, hipStream_t s)
{
    if (index_.current(epoch, c.n)) return PHX_OK;
    index_.stale();
    PHX_TRY(offsets_.reserve((size_t)c.n + 1));
    PHX_HIP(hipMemsetAsync(offsets_.p, 0, ((size_t)c.n + 1) * sizeof(unsigned), s));
    const int ne = 2 * c.nm;
    entries_ = nullptr;
    if (ne) {
        PHX_TRY(idx_sort_.reserve(ne)); PHX_TRY(hist_.reserve(radix_hist_words(ne)));
        hipLaunchKernelGGL(k_cidx_entries, dim3(stream_grid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, idx_sort_.keys(), idx_sort_.vals(), offsets_.p);
        PHX_HIP(hipGetLastError());
        const int bits = key_bits((unsigned)c.n - 1u);
        // (stable passes over entries made in manifold order: by the other body, then by the entry's body)
        PHX_TRY(idx_sort_.sort(ne, bits, hist_.p, scan_, s));
        hipLaunchKernelGGL(k_cidx_body_keys, dim3(stream_grid(ne)), dim3(256), 0, s, (const phx_manifold*)c.manifolds, (const unsigned*)idx_sort_.vals(), ne, idx_sort_.spare_keys());
        PHX_HIP(hipGetLastError());
        idx_sort_.rekey_from_spare();                               // (the first pass's keys are spent: both key buffers are free)
        PHX_TRY(idx_sort_.sort(ne, bits, hist_.p, scan_, s));
        entries_ = idx_sort_.vals();
    }
    PHX_TRY(device_exclusive_scan(offsets_.p, c.n + 1, nullptr, scan_, s));      // (per-body counts -> CSR offsets; [n] = 2 nm)
    index_.built(epoch, c.n);
    return PHX_OK;
}

// ---- contacts -------------------------------------------------------------------------------------------------------------------
int DeviceContacts::contacts(const ContactCache& c, unsigned long long epoch, const int* d_bodies, int count, int flags, int32_t* offsets,
                             phx_contact* out, int cap, int64_t* total, Readback& rb, hipStream_t s)
{
    if (count <= 0 || c.nm == 0) { Listing::none(count, offsets, total); return PHX_OK; }
    if (choose(count) == PATH_SCAN) return scan_contacts(c, d_bodies, count, flags, offsets, out, cap, total, rb, s);
    PHX_TRY(ensure_index(c, epoch, s));
    return index_contacts(c, d_bodies, count, flags, offsets, out, cap, total, rb, s);
}

int DeviceContacts::scan_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap,
                                  int64_t* total, Readback& rb, hipStream_t s)
{
    PHX_TRY(list_.room_with_segments(count));
    PHX_HIP(hipMemsetAsync(list_.counts(), 0, (size_t)count * sizeof(unsigned), s));
    for (int q0 = 0; q0 < count; q0 += scan_chunk_)
        hipLaunchKernelGGL((k_cscan<false>), dim3(stream_grid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.sleep, c.cps, c.joints, c.nj, d_bodies, q0,
                           std::min(scan_chunk_, count - q0), flags, list_.counts(), (unsigned*)nullptr, (phx_contact*)nullptr);
    PHX_HIP(hipGetLastError());
    PHX_TRY(list_.settle("phx_world_query_contacts", "records", count, offsets, cap, total, rb, s));
    if (*total == 0) return PHX_OK;
    PHX_TRY(recs_.reserve((size_t)*total)); PHX_TRY(sorted_.reserve((size_t)*total));
    PHX_TRY(list_.segments_from_counts(count, scan_, s));
    // (the cursors start at the segments' offsets: counts() becomes them, the counts are on the host)
    unsigned* cursors = list_.counts();
    PHX_HIP(hipMemcpyAsync(cursors, list_.segments(), (size_t)count * sizeof(unsigned), hipMemcpyDeviceToDevice, s));
    for (int q0 = 0; q0 < count; q0 += scan_chunk_)
        hipLaunchKernelGGL((k_cscan<true>), dim3(stream_grid(c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.sleep, c.cps, c.joints, c.nj, d_bodies, q0,
                           std::min(scan_chunk_, count - q0), flags, (unsigned*)nullptr, cursors, recs_.p);
    // (the cursors have moved to the segments' ends)
    hipLaunchKernelGGL(k_csort_segments, dim3(segment_grid(count)), dim3(256), 0, s, (const phx_contact*)recs_.p, list_.segments(),
                       (const unsigned*)cursors, count, sorted_.p);
    PHX_HIP(hipGetLastError());
    return Listing::deliver(out, sorted_.p, *total, rb, s);
}

int DeviceContacts::index_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap,
                                   int64_t* total, Readback& rb, hipStream_t s)
{
    PHX_TRY(list_.room_with_segments(count));
    hipLaunchKernelGGL((k_cidx_query<false>), dim3(stream_grid(count)), dim3(256), 0, s, c.manifolds, c.mpos, c.sleep, c.cps, c.joints, c.nj, (const unsigned*)offsets_.p,
                       entries_, d_bodies, count, flags, list_.counts(), (const unsigned*)nullptr, (phx_contact*)nullptr);
    PHX_HIP(hipGetLastError());
    PHX_TRY(list_.settle("phx_world_query_contacts", "records", count, offsets, cap, total, rb, s));
    if (*total == 0) return PHX_OK;
    PHX_TRY(recs_.reserve((size_t)*total));
    PHX_TRY(list_.segments_from_counts(count, scan_, s));
    hipLaunchKernelGGL((k_cidx_query<true>), dim3(stream_grid(count)), dim3(256), 0, s, c.manifolds, c.mpos, c.sleep, c.cps, c.joints, c.nj, (const unsigned*)offsets_.p,
                       entries_, d_bodies, count, flags, (unsigned*)nullptr, list_.segments(), recs_.p);
    PHX_HIP(hipGetLastError());
    return Listing::deliver(out, recs_.p, *total, rb, s);
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
    if (base_n_) hipLaunchKernelGGL(k_cev_remap, dim3(stream_grid(base_n_)), dim3(256), 0, s, keep, base_n_, (const unsigned*)ev_pos_.p, base_spare_.p);
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
        PHX_TRY(ev_sort_.reserve(nm)); PHX_TRY(hist_.reserve(radix_hist_words(nm)));
        hipLaunchKernelGGL(k_cev_keys, dim3(stream_grid(nm)), dim3(256), 0, s, c.manifolds, nm, (unsigned)c.n, ev_sort_.keys(), ev_sort_.vals());
        PHX_HIP(hipGetLastError());
        const int bits = key_bits((unsigned)c.n);
        PHX_TRY(ev_sort_.sort(nm, bits, hist_.p, scan_, s));      // by body2 (the keys), body1 riding as the values
        ev_sort_.rekey_by_vals();
        PHX_TRY(ev_sort_.sort(nm, bits, hist_.p, scan_, s));      // by body1 (stable)
        const unsigned* s1 = ev_sort_.keys();
        const unsigned* s2 = ev_sort_.vals();
        const CevUniqueLoad uniq{s1, s2, (unsigned)c.n};
        PHX_TRY(device_exclusive_scan_of(uniq, ev_pos_.p, nm, ev_tot_.p, scan_, s));
        hipLaunchKernelGGL(k_cev_unique, dim3(stream_grid(nm)), dim3(256), 0, s, s1, s2, nm, (unsigned)c.n, (const unsigned*)ev_pos_.p, t_.p);
        PHX_HIP(hipGetLastError());
    } else PHX_HIP(hipMemsetAsync(ev_tot_.p, 0, sizeof(unsigned), s));
    // 3. begin = T \ B (one lane per element of T: its size is on the device), end = B \ T
    const CevMissingLoad begins{t_.p, ev_tot_.p, 0u, base_.p, nullptr, (unsigned)base_n_};
    PHX_TRY(device_exclusive_scan_of(begins, ev_pos_.p, nm, ev_tot_.p + 1, scan_, s));
    if (nm) hipLaunchKernelGGL(k_cev_missing, dim3(stream_grid(nm)), dim3(256), 0, s, begins, nm, (const unsigned*)ev_pos_.p, ev_begin_.p);
    PHX_HIP(hipGetLastError());
    const CevMissingLoad ends{base_.p, nullptr, (unsigned)base_n_, t_.p, ev_tot_.p, 0u};      // (ev_pos_ again: stream order)
    PHX_TRY(device_exclusive_scan_of(ends, ev_pos_.p, base_n_, ev_tot_.p + 2, scan_, s));
    if (base_n_) hipLaunchKernelGGL(k_cev_missing, dim3(stream_grid(base_n_)), dim3(256), 0, s, ends, base_n_, (const unsigned*)ev_pos_.p, ev_end_.p);
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
    hipLaunchKernelGGL(k_cmarkers, dim3(stream_grid(2 * c.nm)), dim3(256), 0, s, c.manifolds, c.nm, c.mpos, c.cps, d_out);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

} // namespace phx
