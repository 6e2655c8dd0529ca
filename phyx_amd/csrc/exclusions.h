// exclusions.h — the collision exclusions of a World (include/phyx_amd.h COLLISION EXCLUSIONS): a set of unordered body pairs that
// UpdatePairs never emits.  The host's sorted list of keys is the truth, as it is for the units' anchors; the device holds what the
// sweep reads — a table of the keys in the pair set's own form (pair_set.h: open addressing, at most half full, no tombstones: it is
// rebuilt, never edited) and one word per body that says whether the body is in any excluded pair, so that a row of any other body
// makes no probe — and the list itself as {lo, hi} records, which a snapshot copies and a removal of bodies remaps.  The device side
// follows lazily: an edit only marks it stale, and sync() rebuilds it before the next reader (a step, the add's compaction, a save).
// O(pairs) bytes cross PCIe per rebuild, nothing per step.
#pragma once

#include <vector>

#include "common.h"

namespace phx {

// what the sweep (broadphase_kernels.h ExcludedSweepView) and the compaction (world_kernels.h ExclusionKept) read
struct ExclusionView {
    const unsigned long long* table;     // keys ps_unordered_key(a, b)
    unsigned mask;
    const unsigned* member;              // per body: non-zero iff the body is in some excluded pair
};

class ExclusionSet {
public:
    int count() const { return (int)keys_.size(); }
    bool empty() const { return keys_.empty(); }
    const std::vector<unsigned long long>& keys() const { return keys_; }      // ascending: by (lo, hi)
    // the set's arithmetic on the host, on keys that are normalised and distinct (the World has checked the call)
    void add(const std::vector<unsigned long long>& keys);                     // union
    void remove(const std::vector<unsigned long long>& keys);                  // difference
    void clear();
    // the device side for `nb` bodies, rebuilt unless current (bodies appended since: the words are zero-extended, nothing else moves)
    int sync(int nb, hipStream_t stream);
    const ExclusionView* view() const { return keys_.empty() ? nullptr : &view_; }      // (after sync; null: the plain sweep)
    const uint2* device_pairs() const { return d_pairs_.p; }                            // (after sync) {lo, hi}, ascending
    // a removal of bodies: pairs with a removed body go, the rest are renumbered through new[] (increasing on kept bodies: the order stays)
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream);
    // load: the set := a device list as device_pairs() gave it (queued; the host list follows at once)
    int adopt_device(const uint2* d_src, int count, hipStream_t stream);

private:
    int upload_pairs(hipStream_t stream);
    std::vector<unsigned long long> keys_;
    std::vector<uint2> staged_;
    DevBuf<uint2> d_pairs_;
    DevBuf<int2> d_moved_;
    DevBuf<unsigned long long> table_;
    DevBuf<unsigned> member_;
    int member_n_ = 0;                   // bodies the words cover
    bool stale_ = false;                 // the host list changed since the device side was built
    ExclusionView view_ = {nullptr, 0u, nullptr};
};

} // namespace phx
