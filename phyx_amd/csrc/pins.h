// pins.h — the World's pins (include/phyx_amd.h PINS): the list, its schedule and the pass that solves it (pins.hip, pin_kernels.h).
//
// Where the truth is: the host list always has the pins' bodies and anchors; the impulses are the device's once the list has been
// uploaded (`dirty_` clear) and come down only when a call needs them (get, add, remove: O(pins) bytes at such a change).  The
// schedule is built on the host from the pins' bodies and their static bits — gathered on the device, O(pins) bytes — lazily at the
// next step after the pin set or the static set changed.
#pragma once

#include "body_view.h"
#include "schedule.h"

namespace phx {

constexpr int PIN_LANES = 256;          // pins per LDS group = lanes of its workgroup (the island kernel's ISL_T)
constexpr int PIN_BODIES = 768;         // bodies per LDS group (the island kernel's ISL_B): 12 KB of LDS, so 13 groups share a CU's 160 KB
constexpr int PIN_MAX_ITERATIONS = 64;

// the schedule of `count` pins (body2 = -1: the world, one virtual static body `nb`) as build_island_schedule makes it with one pin per unit
void build_pin_schedule(const int32_t* body1, const int32_t* body2, int count, const unsigned char* is_static, int nb, int group_pins, Schedule& out);

class PinSet {
public:
    int configure_from_env();            // PHX_PIN_GROUP_PINS
    int count() const { return (int)host_.size(); }
    int group_pins() const { return group_pins_; }
    long long builds() const { return builds_; }
    int iterations = 8;

    // the calls (arguments already checked by the World); `stream` is the world's
    int add(const phx_pin* pins, int count, hipStream_t stream);
    int remove(const int32_t* which, int count, hipStream_t stream);
    int set_anchors(const int32_t* which, const float* anchors, int count, const int* d_which, const float* d_anchors, hipStream_t stream);
    bool on_device() const { return !dirty_ && !host_.empty(); }      // set_anchors needs its batch staged only then
    int get(phx_pin* out, hipStream_t stream);
    void clear() { host_.clear(); dirty_ = true; sched_dirty_ = true; }
    void statics_changed() { if (!host_.empty()) sched_dirty_ = true; }
    // a removal of bodies compacted them through `d_remap` (old index -> new or -1): the pins of removed bodies go, the rest are renumbered
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream);
    // snapshots: the device copy, current
    int upload(hipStream_t stream);
    const phx_pin* device_pins() const { return d_pins_.p; }
    int adopt_device(const phx_pin* d_src, int count, hipStream_t stream);      // load: the list := a device array (queued; the host list follows at once)

    // the schedule, built unless current
    int prepare(const float4* mpos, int nb, Readback& rb, hipStream_t stream);
    const Schedule& schedule() const { return sched_; }
    // the pass: everything queued on `stream`
    int solve(const WorldBodies& bodies, int nb, float dt, Readback& rb, hipStream_t stream);

private:
    int fetch(hipStream_t stream);       // the impulses come down: the host list is complete
    std::vector<phx_pin> host_;
    bool dirty_ = true;                  // the host list is the truth, impulses included; the device copy is stale
    bool sched_dirty_ = true;
    int group_pins_ = 0;
    long long builds_ = 0;
    DevBuf<phx_pin> d_pins_;
    DevBuf<unsigned> d_bits_;
    DevBuf<int2> d_moved_;
    DevBuf<char> d_tables_;              // slots | groups | group bodies, one upload per build
    DevBuf<char> d_work_;                // the trailing group's prestep results
    size_t off_groups_ = 0, off_bodies_ = 0;
    Schedule sched_;
    std::vector<int> hbm_classes_;       // the trailing group's class offsets (absolute slots)
};

} // namespace phx
