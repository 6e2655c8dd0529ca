// contact.h — the World's contact reports (include/phyx_amd.h, CONTACTS): the host side of contact_kernels.h.  The World hands over its
// resident contact cache, its body count, its contact epoch and its stream; everything is queued on that stream.  The contact index (a
// body -> (other, manifold) incidence in CSR form) is built by the first index-path call after the contact cache changed and kept while
// the epoch stays.  The events' baseline B (sorted (body1, body2) keys) lives here too.
// What is left here is the reports' own: the threshold, the index, which kernels count and fill, the events and the markers.  The
// path choice, the index stamp and the two-pass protocol of the contact lists are listing.h's.
#pragma once

#include "body_view.h"
#include "sleep.h"
#include "listing.h"

#include <cstdint>
#include <utility>
#include <vector>

namespace phx {

// what the contact reports read: the World's resident arrays and their counts
struct ContactCache {
    const phx_manifold* manifolds; int nm;
    const phx_contact_point* cps;
    const phx_contact_joint* joints; int nj;
    const float4* mpos; int n;
    const SleepCell* sleep;      // the sleep column (sleep.h), null while sleeping is off: PHX_QUERY_SKIP_STATIC keeps a sleeper
};

class DeviceContacts {
public:
    // the scan path answers up to this many listed bodies, the index larger batches: the largest batch at which tools/contact_cost.py
    // measured the scan faster at cfg 2, each call after a step so that the index pays its build (512 scan 0.40 ms /
    // index 0.44 ms, 768 scan 0.54 / index 0.49; sizes between two measured ones are not measured)
    static constexpr int SCAN_MAX = 512;

    // PHX_CONTACT_PATH=scan|index forces a path; PHX_CONTACT_SCAN_CHUNK=q (1 .. 1024) lowers the listed bodies per chunk of the scan
    // path.  Read when the world is created; any other value is refused (PHX_ERR_INVALID).
    int configure_from_env();
    ReportPath choose(int count) const { return choose_path(forced_, count, SCAN_MAX); }

    // d_bodies: the listed bodies on the device (checked by the caller).  Host outputs; waits through `rb`.
    int contacts(const ContactCache& c, unsigned long long epoch, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out,
                 int cap, int64_t* total, Readback& rb, hipStream_t s);
    int ensure_index(const ContactCache& c, unsigned long long epoch, hipStream_t s);
    int index_builds() const { return index_.builds(); }

    // T(s) \ B and B \ T(s) into host memory; B := T(s) only when both fit
    int events(const ContactCache& c, int32_t* begin, int begin_cap, int64_t* begin_total, int32_t* end, int end_cap, int64_t* end_total,
               Readback& rb, hipStream_t s);
    int markers(const ContactCache& c, phx_contact_marker* d_out, hipStream_t s);

    // B := the given sorted, distinct keys ((body1 << 32) | body2)
    int set_baseline(const std::vector<unsigned long long>& keys, hipStream_t s);
    // the removal: queue the remap of B through the device's new[] into the spare baseline, its size into *d_count; then, once the
    // caller has read that count back, baseline_remapped(count) makes it B (a removal that changes nothing does not call it)
    int remap_baseline(const int* d_remap, unsigned* d_count, hipStream_t s);
    void baseline_remapped(unsigned count) { std::swap(base_, base_spare_); base_n_ = (int)count; }
    // snapshots (world_state.hip save / load): B as it is — its keys in HBM and their number; a load makes room (the old B goes), queues the
    // copy itself and then says how many keys B has
    unsigned long long* baseline() const { return base_.p; }
    int baseline_count() const { return base_n_; }
    int reserve_baseline(size_t count) { return base_.reserve(std::max<size_t>(count, 1)); }
    void baseline_replaced(int count) { base_n_ = count; }

private:
    int scan_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap, int64_t* total,
                      Readback& rb, hipStream_t s);
    int index_contacts(const ContactCache& c, const int* d_bodies, int count, int flags, int32_t* offsets, phx_contact* out, int cap, int64_t* total,
                       Readback& rb, hipStream_t s);

    ReportPath forced_ = PATH_AUTO;
    int scan_chunk_ = 256;
    // the index
    IndexStamp index_;
    const unsigned* entries_ = nullptr;
    RadixPairs idx_sort_;
    DevBuf<unsigned> offsets_, hist_;
    ScanScratch scan_;
    // per-call scratch
    Listing list_;
    DevBuf<phx_contact> recs_, sorted_;
    // events
    DevBuf<unsigned long long> base_, base_spare_, t_;
    int base_n_ = 0;
    RadixPairs ev_sort_;
    DevBuf<unsigned> ev_pos_, ev_tot_;
    DevBuf<int2> ev_begin_, ev_end_;
};

} // namespace phx
