// pins.h — the World's pins (include/phyx_amd.h PINS): the list, its schedule and the pass that solves it (pins.hip, pin_kernels.h).
//
// Where the truth is: the host list always has the pins' bodies and anchors; the impulses are the device's once the list has been
// uploaded (`dirty_` clear) and come down only when a call needs them (get, add, remove: O(pins) bytes at such a change).  The
// schedule is built on the host from the pins' bodies and their static bits — gathered on the device, O(pins) bytes — lazily at the
// next step after the pin set or the static set changed.
//
// Links (include/phyx_amd.h LINKS) are the pass's second kind of unit: the units are the pins followed by the links, one schedule and
// one pass for both.  UnitList is the one copy of the list machinery (host and device copy, upload, fetch, remap) for either record.
#pragma once

#include "body_view.h"
#include "schedule.h"

namespace phx {

constexpr int PIN_LANES = 256;          // pins per LDS group = lanes of its workgroup (the island kernel's ISL_T)
constexpr int PIN_BODIES = 768;         // bodies per LDS group (the island kernel's ISL_B): 12 KB of LDS, so 13 groups share a CU's 160 KB
constexpr int PIN_MAX_ITERATIONS = 64;

// the schedule of `count` pins (body2 = -1: the world, one virtual static body `nb`) as build_island_schedule makes it with one pin per unit
void build_pin_schedule(const int32_t* body1, const int32_t* body2, int count, const unsigned char* is_static, int nb, int group_pins, Schedule& out);

// a list of records `P` (phx_pin, phx_link: body1, body2, anchor1, anchor2 first; `impulse` the device's once uploaded)
template <class P> class UnitList {
public:
    int count() const { return (int)host_.size(); }
    bool on_device() const { return !dirty_ && !host_.empty(); }
    const std::vector<P>& host() const { return host_; }                      // (impulses: only after fetch)
    P* device() const { return d_.p; }
    int fetch(hipStream_t stream);       // the impulses come down: the host list is complete
    int upload(hipStream_t stream);
    int add(const P* recs, int count, hipStream_t stream);
    int remove(const int32_t* which, int count, hipStream_t stream);
    int get(P* out, hipStream_t stream);
    void clear() { host_.clear(); dirty_ = true; }
    // an edit of fields that are the host's truth: `edit(record, k)` on the host list; the caller scatters on the device when on_device()
    template <class F> void edit(const int32_t* which, int count, F f) { for (int k = 0; k < count; ++k) f(host_[(size_t)which[k]], k); }
    int set_anchors(const int32_t* which, const float* anchors, int count, const int* d_which, const float* d_anchors, hipStream_t stream);
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream, bool* changed);
    int adopt_device(const P* d_src, int count, hipStream_t stream);
    int statics(const float4* mpos, unsigned* d_bits, hipStream_t stream) const;      // queues the static bits of every record's bodies
private:
    std::vector<P> host_;
    bool dirty_ = true;                  // the host list is the truth, impulses included; the device copy is stale
    DevBuf<P> d_;
    DevBuf<int2> d_moved_;
};

class PinSet {
public:
    int configure_from_env();            // PHX_PIN_GROUP_PINS
    int count() const { return pins_.count(); }
    int link_count() const { return links_.count(); }
    int units() const { return count() + link_count(); }                    // the pass's units: the pins, then the links
    int group_pins() const { return group_pins_; }
    long long builds() const { return builds_; }
    int iterations = 8;

    // the calls (arguments already checked by the World); `stream` is the world's
    int add(const phx_pin* pins, int count, hipStream_t stream) { sched_dirty_ = true; return pins_.add(pins, count, stream); }
    int remove(const int32_t* which, int count, hipStream_t stream) { sched_dirty_ = true; return pins_.remove(which, count, stream); }
    int set_anchors(const int32_t* which, const float* anchors, int count, const int* d_which, const float* d_anchors, hipStream_t stream)
    { return pins_.set_anchors(which, anchors, count, d_which, d_anchors, stream); }
    bool on_device() const { return pins_.on_device(); }              // set_anchors needs its batch staged only then
    int get(phx_pin* out, hipStream_t stream) { return pins_.get(out, stream); }
    int add_links(const phx_link* links, int count, hipStream_t stream) { sched_dirty_ = true; return links_.add(links, count, stream); }
    int remove_links(const int32_t* which, int count, hipStream_t stream) { sched_dirty_ = true; return links_.remove(which, count, stream); }
    int set_link_anchors(const int32_t* which, const float* anchors, int count, const int* d_which, const float* d_anchors, hipStream_t stream)
    { return links_.set_anchors(which, anchors, count, d_which, d_anchors, stream); }
    int set_link_lengths(const int32_t* which, const float* lengths, int count, const int* d_which, const float* d_lengths, hipStream_t stream);
    bool links_on_device() const { return links_.on_device(); }
    int get_links(phx_link* out, hipStream_t stream) { return links_.get(out, stream); }
    const std::vector<phx_link>& host_links() const { return links_.host(); }      // (bodies, anchors, lengths, hertz: always current)
    void clear() { pins_.clear(); links_.clear(); sched_dirty_ = true; }
    void statics_changed() { if (units()) sched_dirty_ = true; }
    // a removal of bodies compacted them through `d_remap` (old index -> new or -1): the units of removed bodies go, the rest are renumbered
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream);
    // snapshots: the device copies, current
    int upload(hipStream_t stream) { PHX_TRY(pins_.upload(stream)); return links_.upload(stream); }
    const phx_pin* device_pins() const { return pins_.device(); }
    const phx_link* device_links() const { return links_.device(); }
    // load: the lists := device arrays (queued; the host lists follow at once)
    int adopt_device(const phx_pin* d_pins, int pin_count, const phx_link* d_links, int link_count, hipStream_t stream);

    // the schedule, built unless current
    int prepare(const float4* mpos, int nb, Readback& rb, hipStream_t stream);
    const Schedule& schedule() const { return sched_; }
    // the pass: everything queued on `stream`
    int solve(const WorldBodies& bodies, int nb, float dt, Readback& rb, hipStream_t stream);

private:
    UnitList<phx_pin> pins_;
    UnitList<phx_link> links_;
    bool sched_dirty_ = true;
    int group_pins_ = 0;
    long long builds_ = 0;
    DevBuf<unsigned> d_bits_;
    DevBuf<char> d_tables_;              // slots | groups | group bodies, one upload per build
    DevBuf<char> d_work_;                // the trailing group's prestep results
    size_t off_groups_ = 0, off_bodies_ = 0;
    Schedule sched_;
    std::vector<int> hbm_classes_;       // the trailing group's class offsets (absolute slots)
};

} // namespace phx
