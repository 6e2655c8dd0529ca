// pins.h — the World's pins (include/phyx_amd.h PINS): the list, its schedule and the pass that solves it (pins.hip, pin_kernels.h).
//
// Where the truth is: the host list always has the pins' bodies and anchors; the impulses are the device's once the list has been
// uploaded (`dirty_` clear) and come down only when a call needs them (get, add, remove: O(pins) bytes at such a change).  The
// schedule is built on the host from the pins' bodies and their static bits — gathered on the device, O(pins) bytes — lazily at the
// next step after the pin set or the static set changed.
//
// Links (include/phyx_amd.h LINKS) are the pass's second kind of unit: the units are the pins followed by the links, one schedule and
// one pass for both.  UnitList is the one copy of the list machinery (host and device copy, upload, fetch, remap, field edits) for either
// record, and UnitKind states what the World's one copy of the calls (world_units.hip) needs to know of a record.
//
// Angles (include/phyx_amd.h ANGLES) are the third kind, behind the links: a record without anchors, so nothing here may ask for any
// but through AnchorFields, which an angle never instantiates.
//
// Sliders (include/phyx_amd.h SLIDERS) are the fourth kind, behind the angles: anchors as a pin's, limits and a motor as an angle's.
//
// Breaks (include/phyx_amd.h BREAKS; tests/break_spec.py): a list may carry a column of break limits beside its records, the host copy
// the truth as for anchors.  A pass over lists with a column is followed by the break test (pin_kernels.h k_unit_breaks); what it found
// is settled lazily on the host (PinSet::settle): 4 bytes come down, the events only if there are any, and the broken units leave
// through UnitList::remove.
#pragma once

#include <limits>
#include <tuple>
#include <type_traits>

#include "body_view.h"
#include "schedule.h"

namespace phx {

constexpr int PIN_LANES = 256;          // pins per LDS group = lanes of its workgroup (the island kernel's ISL_T)
constexpr int PIN_BODIES = 768;         // bodies per LDS group (the island kernel's ISL_B): 12 KB of LDS, so 13 groups share a CU's 160 KB
constexpr int PIN_MAX_ITERATIONS = 64;

// the schedule of `count` pins (body2 = -1: the world, one virtual static body `nb`) as build_island_schedule makes it with one pin per unit
void build_pin_schedule(const int32_t* body1, const int32_t* body2, int count, const unsigned char* is_static, int nb, int group_pins, Schedule& out);

// what the calls know of a record: its nouns, the C calls' names, and `check`: entry k of an add beyond the body rules (the floats
// that must be finite, then the record's own rules); of a kind with limits and a motor also the name of the motor's bound
template <class P> struct UnitKind;
// the rules of a limited row's bounds and of a motor's two values (`P`: phx_angle or phx_slider): an add's, and phx_world_set_*_limits' / _motors'
template <class P> int check_limits(const char* what, int k, float lower, float upper, float hertz);
template <class P> int check_motor(const char* what, int k, float speed, float bound);
template <> struct UnitKind<phx_pin> {
    static constexpr const char* noun = "pin";
    static constexpr const char* plural = "pins";
    static constexpr const char* add = "phx_world_add_pins", *remove = "phx_world_remove_pins", *set_anchors = "phx_world_set_pin_anchors", *get = "phx_world_get_pins";
    static int check(const char* what, int k, const phx_pin& p);
};
template <> struct UnitKind<phx_link> {
    static constexpr const char* noun = "link";
    static constexpr const char* plural = "links";
    static constexpr const char* add = "phx_world_add_links", *remove = "phx_world_remove_links", *set_anchors = "phx_world_set_link_anchors", *get = "phx_world_get_links";
    static int check(const char* what, int k, const phx_link& p);
    static int check_lengths(const char* what, int k, float lo, float hi, float hertz);      // (also phx_world_set_link_lengths' rule)
};

template <> struct UnitKind<phx_angle> {
    static constexpr const char* noun = "angle";
    static constexpr const char* plural = "angles";
    static constexpr const char* add = "phx_world_add_angles", *remove = "phx_world_remove_angles", *get = "phx_world_get_angles";      // (no anchors to set)
    static constexpr const char* set_limits = "phx_world_set_angle_limits", *set_motors = "phx_world_set_angle_motors", *motor_bound = "max_torque";
    static int check(const char* what, int k, const phx_angle& p);
};

template <> struct UnitKind<phx_slider> {
    static constexpr const char* noun = "slider";
    static constexpr const char* plural = "sliders";
    static constexpr const char* add = "phx_world_add_sliders", *remove = "phx_world_remove_sliders", *set_anchors = "phx_world_set_slider_anchors", *get = "phx_world_get_sliders";
    static constexpr const char* set_limits = "phx_world_set_slider_limits", *set_motors = "phx_world_set_slider_motors", *motor_bound = "max_force";
    static int check(const char* what, int k, const phx_slider& p);
};

// the fields an edit between steps writes, `width` floats per record: on the host list and, by k_unit_fields, on the device copy
struct AnchorFields {
    static constexpr int width = 4;
    template <class P> static __host__ __device__ void write(P& p, const float* v) { p.anchor1 = phx_vec2{v[0], v[1]}; p.anchor2 = phx_vec2{v[2], v[3]}; }
};
struct LengthFields {
    static constexpr int width = 2;
    static __host__ __device__ void write(phx_link& p, const float* v) { p.min_length = v[0]; p.max_length = v[1]; }
};

struct LimitFields {
    static constexpr int width = 2;
    template <class P> static __host__ __device__ void write(P& p, const float* v) { p.lower = v[0]; p.upper = v[1]; }
};
struct MotorFields {
    static constexpr int width = 2;
    static __host__ __device__ void write(phx_angle& p, const float* v) { p.motor_speed = v[0]; p.max_torque = v[1]; }
    static __host__ __device__ void write(phx_slider& p, const float* v) { p.motor_speed = v[0]; p.max_force = v[1]; }
};

// a list of records `P` (phx_pin, phx_link, phx_angle, phx_slider: body1, body2 first; the impulses the device's once uploaded)
template <class P> class UnitList {
public:
    using record = P;
    int count() const { return (int)host_.size(); }
    bool on_device() const { return !dirty_ && !host_.empty(); }
    const std::vector<P>& host() const { return host_; }                      // (impulses: only after fetch)
    P* device() const { return d_.p; }
    int fetch(hipStream_t stream);       // the impulses come down: the host list is complete
    int upload(hipStream_t stream);
    int add(const P* recs, int count, hipStream_t stream);
    int remove(const int32_t* which, int count, hipStream_t stream);
    int get(P* out, hipStream_t stream);
    void clear() { host_.clear(); limits_.clear(); dirty_ = true; }
    // the break limits, one per record: a column that exists only once a finite limit was set in this list (without it every limit is +inf)
    bool limited() const { return !limits_.empty(); }
    const float* device_limits() const { return limited() ? d_limits_.p : nullptr; }      // (current with the records: upload)
    void get_limits(float* out) const;
    // already checked; `d_*`: the staged batch, needed where the list is on the device and has its column already
    int set_limits(const int32_t* which, const float* values, int count, const int* d_which, const float* d_values, hipStream_t stream);
    // an edit of fields that are the host's truth: written into the host list and, when on_device(), scattered from the staged batch `d_*`
    template <class Fields> int set_fields(const int32_t* which, const float* values, int count, const int* d_which, const float* d_values, hipStream_t stream);
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream, bool* changed);
    int adopt_device(const P* d_src, const float* d_limits, int count, hipStream_t stream);      // (d_limits null: no column)
    int statics(const float4* mpos, unsigned* d_bits, hipStream_t stream) const;      // queues the static bits of every record's bodies
private:
    std::vector<P> host_;
    bool dirty_ = true;                  // the host list is the truth, impulses included; the device copy is stale
    DevBuf<P> d_;
    DevBuf<int2> d_moved_;
    std::vector<float> limits_;          // empty, or a limit per record
    DevBuf<float> d_limits_;
    template <class Gone> void compact(Gone gone);      // the records (and limits) i with gone(i) leave, the rest keep their order
};

class PinSet {
public:
    int configure_from_env();            // PHX_PIN_GROUP_PINS
    template <class P> UnitList<P>& list() { return std::get<UnitList<P>>(lists_); }
    template <class P> const UnitList<P>& list() const { return std::get<UnitList<P>>(lists_); }
    // f(list) for the four lists in the order of the kinds among the pass's units, up to the first that fails
    template <class F> int each_list(F f)
    {
        int st = PHX_OK;
        std::apply([&](auto&... l) { ((st = st != PHX_OK ? st : f(l)), ...); }, lists_);
        return st;
    }
    int units() const { return std::apply([](const auto&... l) { return (l.count() + ...); }, lists_); }      // the pass's units
    int group_pins() const { return group_pins_; }
    long long builds() const { return builds_; }
    int iterations = 8;

    // the calls (world_units.hip) work on list<P>() with arguments already checked; what is the set's own: an add or a removal ...
    void units_changed() { sched_dirty_ = true; }
    void clear() { each_list([](auto& l) { l.clear(); return PHX_OK; }); sched_dirty_ = true; drop_breaks(); }
    void statics_changed() { if (units()) sched_dirty_ = true; }             // ... and a change of the static set make the schedule stale
    // a removal of bodies compacted them through `d_remap` (old index -> new or -1): the units of removed bodies go, the rest are renumbered
    int bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream);
    // snapshots: the device copies (list<P>().device()), current
    int upload(hipStream_t stream) { return each_list([&](auto& l) { return l.upload(stream); }); }
    // load: a list := a device array (queued; the host list follows at once)
    template <class P> int adopt_device(const P* d_src, const float* d_limits, int count, hipStream_t stream) { sched_dirty_ = true; return list<P>().adopt_device(d_src, d_limits, count, stream); }

    // the schedule, built unless current
    int prepare(const float4* mpos, int nb, Readback& rb, hipStream_t stream);
    const Schedule& schedule() const { return sched_; }
    // the pass: everything queued on `stream`; behind it, where some list has a limit column, the break test of step `step` (its ordinal
    // among the steps since the events were last taken)
    int solve(const WorldBodies& bodies, int nb, float dt, int step, Readback& rb, hipStream_t stream);
    // breaks: does some list have a limit column / has a break test run that settle() has not looked at yet
    bool limited() const { return std::apply([](const auto&... l) { return (l.limited() || ...); }, lists_); }
    bool breaks_pending() const { return breaks_pending_; }
    // the pending test's count comes down (4 bytes) and, only if it is not zero, its events: the broken units leave their lists as a
    // removal's would and the events join the queue.  Between steps; prepare() begins with it.
    int settle(Readback& rb, hipStream_t stream);
    std::vector<phx_break_event>& break_queue() { return queue_; }
    void drop_breaks() { breaks_pending_ = false; queue_.clear(); }         // an abandoned timeline: nothing pending, no events

private:
    std::tuple<UnitList<phx_pin>, UnitList<phx_link>, UnitList<phx_angle>, UnitList<phx_slider>> lists_;      // the kinds, in their order among the pass's units
    bool sched_dirty_ = true;
    int group_pins_ = 0;
    long long builds_ = 0;
    DevBuf<unsigned> d_bits_;
    DevBuf<char> d_tables_;              // slots | groups | group bodies, one upload per build
    DevBuf<char> d_work_;                // the trailing group's prestep results (with sliders: the PinWork array, then the RailWork array)
    size_t off_groups_ = 0, off_bodies_ = 0;
    Schedule sched_;
    std::vector<int> hbm_classes_;       // the trailing group's class offsets (absolute slots)
    bool breaks_pending_ = false; int pending_step_ = 0;
    DevBuf<phx_break_event> d_staged_, d_events_;      // a record per limited unit each (pin_kernels.h k_unit_breaks)
    DevBuf<unsigned> d_break_words_;
    std::vector<phx_break_event> queue_; // the events since phx_world_break_events last took them
};

} // namespace phx
