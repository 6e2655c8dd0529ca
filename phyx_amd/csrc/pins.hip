// pins.hip — PinSet: the World's pins, their schedule and the pass that solves them (include/phyx_amd.h PINS; kernels: pin_kernels.h).
//
// The data path.  At a change of the pin set or the static set: the pins' static bits come down (4 bytes per pin), the host builds the
// schedule with the contact schedule's own builder (one pin per unit, the world as one virtual static body) and one upload carries the
// slot, group and group-body tables.  Per step nothing crosses PCIe: k_solve_pins, one workgroup per LDS group, does the whole pass of
// those groups in one launch; the trailing group — components that do not fit a workgroup — takes a prestep launch and one launch per
// class for the warm start and per class and sweep.
// Links (include/phyx_amd.h LINKS) are the pass's second kind of unit: UnitList<P> is the list machinery for either record and
// UnitKind<P> what the World's calls check of one, the schedule is built over the pins followed by the links, and a world that has
// links launches the kernels' LINKS instantiations.  Angles (ANGLES) are the third, behind the links; a world that has angles
// launches the instantiations with both.  Sliders (SLIDERS) are the fourth, behind the angles; a world that has sliders launches the
// instantiations that know all four kinds.
#include "pins.h"
#include "pin_kernels.h"

namespace phx {

static inline int pgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }

void build_pin_schedule(const int32_t* body1, const int32_t* body2, int count, const unsigned char* is_static, int nb, int group_pins, Schedule& out)
{
    // the builder numbers a component per dynamic body and bins consecutive components (schedule.h BINNING): it is given the pins' own
    // bodies only, renumbered in body order, so that bodies no pin touches do not thin the groups out.  The world is the body behind
    // them, static; priority ids 2 k never differ in the lowest bit only, so no two pins are paired into a unit.
    std::vector<int> ids;
    ids.reserve(2 * (size_t)count);
    for (int k = 0; k < count; ++k) { ids.push_back(body1[k]); if (body2[k] >= 0) ids.push_back(body2[k]); }
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int dense = (int)ids.size();
    auto local = [&](int b) { return (int)(std::lower_bound(ids.begin(), ids.end(), b) - ids.begin()); };
    std::vector<int> b1((size_t)count), b2((size_t)count), prio((size_t)count);
    std::vector<unsigned char> st((size_t)dense + 1, 1);
    for (int i = 0; i < dense; ++i) st[(size_t)i] = is_static[ids[(size_t)i]];
    for (int k = 0; k < count; ++k) { b1[(size_t)k] = local(body1[k]); b2[(size_t)k] = body2[k] < 0 ? dense : local(body2[k]); prio[(size_t)k] = 2 * k; }
    LdsCaps caps;
    caps.max_units = group_pins; caps.max_joints = group_pins; caps.max_bodies = PIN_BODIES; caps.max_colours = 64;
    build_island_schedule(b1.data(), b2.data(), count, st.data(), dense + 1, caps, out, nullptr, prio.data());
    for (int& b : out.group_bodies) b = b == dense ? nb : ids[(size_t)b];  // (the LDS groups' bodies under their own numbers again; the world: nb)
}

int PinSet::configure_from_env()
{
    group_pins_ = PIN_LANES;
    const char* c = getenv("PHX_PIN_GROUP_PINS");
    if (!c) return PHX_OK;
    char* end = nullptr;
    const long v = strtol(c, &end, 10);
    if (!*c || *end || v < 1 || v > PIN_LANES) { set_error("PHX_PIN_GROUP_PINS=%s: expected an integer in [1, %d]", c, PIN_LANES); return PHX_ERR_INVALID; }
    group_pins_ = (int)v;
    return PHX_OK;
}

template <class P> int UnitList<P>::fetch(hipStream_t stream)
{
    if (dirty_ || host_.empty()) return PHX_OK;
    PHX_HIP(hipStreamSynchronize(stream));
    PHX_HIP(hipMemcpy(host_.data(), d_.p, host_.size() * sizeof(P), hipMemcpyDeviceToHost));
    return PHX_OK;
}

template <class P> int UnitList<P>::upload(hipStream_t stream)
{
    if (!dirty_ || host_.empty()) return PHX_OK;
    PHX_TRY(d_.reserve(host_.size()));
    PHX_HIP(hipMemcpyAsync(d_.p, host_.data(), host_.size() * sizeof(P), hipMemcpyHostToDevice, stream));
    if (limited()) {
        PHX_TRY(d_limits_.reserve(limits_.size()));
        PHX_HIP(hipMemcpyAsync(d_limits_.p, limits_.data(), limits_.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    }
    PHX_HIP(hipStreamSynchronize(stream));
    dirty_ = false;
    return PHX_OK;
}

template <class P> int UnitList<P>::add(const P* recs, int count, hipStream_t stream)
{
    PHX_TRY(fetch(stream));
    host_.insert(host_.end(), recs, recs + count);
    if (limited()) limits_.insert(limits_.end(), (size_t)count, std::numeric_limits<float>::infinity());      // (a new unit is unbreakable)
    dirty_ = true;
    return PHX_OK;
}

template <class P> int UnitList<P>::remove(const int32_t* which, int count, hipStream_t stream)
{
    PHX_TRY(fetch(stream));
    std::vector<unsigned char> gone(host_.size(), 0);
    for (int k = 0; k < count; ++k) gone[(size_t)which[k]] = 1;
    compact([&](size_t i) { return gone[i] != 0; });
    return PHX_OK;
}

template <class P> template <class Gone> void UnitList<P>::compact(Gone gone)
{
    size_t at = 0;
    for (size_t i = 0; i < host_.size(); ++i) {
        if (gone(i)) continue;
        host_[at] = host_[i];
        if (limited()) limits_[at] = limits_[i];
        ++at;
    }
    host_.resize(at);
    if (limited()) limits_.resize(at);
    dirty_ = true;
}

template <class P> void UnitList<P>::get_limits(float* out) const
{
    if (limited()) std::copy(limits_.begin(), limits_.end(), out);
    else std::fill(out, out + host_.size(), std::numeric_limits<float>::infinity());
}

template <class P> int UnitList<P>::set_limits(const int32_t* which, const float* values, int count, const int* d_which, const float* d_values, hipStream_t stream)
{
    const bool had = limited();
    if (!had) {
        bool finite = false;
        for (int k = 0; k < count; ++k) finite = finite || std::isfinite(values[k]);
        if (!finite) return PHX_OK;                                         // (+inf where every limit is +inf: the list stays without a column)
        limits_.assign(host_.size(), std::numeric_limits<float>::infinity());
    }
    for (int k = 0; k < count; ++k) limits_[(size_t)which[k]] = values[k];
    if (!on_device()) return PHX_OK;
    if (had) {
        hipLaunchKernelGGL(k_unit_limits, dim3(pgrid(count)), dim3(256), 0, stream, d_which, d_values, count, d_limits_.p);
        PHX_HIP(hipGetLastError());
        return PHX_OK;
    }
    // the column's first appearance beside records that are on the device already: it goes up whole, once
    PHX_TRY(d_limits_.reserve(limits_.size()));
    PHX_HIP(hipMemcpyAsync(d_limits_.p, limits_.data(), limits_.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    PHX_HIP(hipStreamSynchronize(stream));
    return PHX_OK;
}

template <class P> template <class Fields>
int UnitList<P>::set_fields(const int32_t* which, const float* values, int count, const int* d_which, const float* d_values, hipStream_t stream)
{
    for (int k = 0; k < count; ++k) Fields::write(host_[(size_t)which[k]], values + Fields::width * k);
    if (!on_device()) return PHX_OK;
    hipLaunchKernelGGL((k_unit_fields<P, Fields>), dim3(pgrid(count)), dim3(256), 0, stream, d_which, d_values, count, d_.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

template <class P> int UnitList<P>::get(P* out, hipStream_t stream)
{
    PHX_TRY(fetch(stream));
    if (!host_.empty()) std::memcpy(out, host_.data(), host_.size() * sizeof(P));
    return PHX_OK;
}

template <class P> int UnitList<P>::bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream, bool* changed)
{
    const int n = count();
    if (!n) return PHX_OK;
    PHX_TRY(upload(stream));
    PHX_TRY(d_moved_.reserve((size_t)n));
    hipLaunchKernelGGL(k_pin_remap<P>, dim3(pgrid(n)), dim3(256), 0, stream, (const P*)d_.p, n, d_remap, d_moved_.p);
    PHX_HIP(hipGetLastError());
    // one round trip: the remapped bodies and the records themselves (their impulses are the device's)
    std::vector<int2> moved((size_t)n);
    PHX_TRY(rb.add(moved.data(), d_moved_.p, (size_t)n * sizeof(int2), stream));
    PHX_TRY(rb.add(host_.data(), d_.p, (size_t)n * sizeof(P), stream));
    PHX_TRY(rb.wait(stream));
    for (size_t i = 0; i < host_.size(); ++i) { host_[i].body1 = moved[i].x; host_[i].body2 = moved[i].y == -2 ? -1 : moved[i].y; }
    compact([&](size_t i) { return moved[i].x == -1 || moved[i].y == -1; });
    *changed = true;
    return PHX_OK;
}

template <class P> int UnitList<P>::adopt_device(const P* d_src, const float* d_limits, int count, hipStream_t stream)
{
    host_.resize((size_t)count);
    limits_.assign(d_limits ? (size_t)count : 0, 0.f);
    dirty_ = true;
    if (!count) return PHX_OK;
    // (the bodies and anchors are needed on the host for the schedule and the later edits: the list comes down once, O(records))
    PHX_HIP(hipMemcpyAsync(host_.data(), d_src, (size_t)count * sizeof(P), hipMemcpyDeviceToHost, stream));
    if (d_limits) PHX_HIP(hipMemcpyAsync(limits_.data(), d_limits, (size_t)count * sizeof(float), hipMemcpyDeviceToHost, stream));
    PHX_HIP(hipStreamSynchronize(stream));
    return PHX_OK;
}

template <class P> int UnitList<P>::statics(const float4* mpos, unsigned* d_bits, hipStream_t stream) const
{
    const int n = count();
    if (!n) return PHX_OK;
    hipLaunchKernelGGL(k_pin_statics<P>, dim3(pgrid(n)), dim3(256), 0, stream, (const P*)d_.p, n, mpos, d_bits);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

template class UnitList<phx_pin>;
template class UnitList<phx_link>;
template class UnitList<phx_angle>;
template class UnitList<phx_slider>;

template int UnitList<phx_pin>::set_fields<AnchorFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_link>::set_fields<AnchorFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_link>::set_fields<LengthFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_angle>::set_fields<LimitFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_angle>::set_fields<MotorFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_slider>::set_fields<AnchorFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_slider>::set_fields<LimitFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);
template int UnitList<phx_slider>::set_fields<MotorFields>(const int32_t*, const float*, int, const int*, const float*, hipStream_t);

// ---- entry k of an add beyond the body rules (the order of the checks is the calls' contract: the first failure wins) ----
static int check_finite(const char* what, const char* noun, int k, std::initializer_list<float> values)
{
    int c = 0;
    for (const float v : values) {
        if (!std::isfinite(v)) { set_error("%s: %s %d: value %d is not finite", what, noun, k, c); return PHX_ERR_INVALID; }
        ++c;
    }
    return PHX_OK;
}

int UnitKind<phx_pin>::check(const char* what, int k, const phx_pin& p)
{
    return check_finite(what, noun, k, {p.anchor1.x, p.anchor1.y, p.anchor2.x, p.anchor2.y, p.impulse.x, p.impulse.y});
}

int UnitKind<phx_link>::check(const char* what, int k, const phx_link& p)
{
    PHX_TRY(check_finite(what, noun, k, {p.anchor1.x, p.anchor1.y, p.anchor2.x, p.anchor2.y, p.min_length, p.max_length, p.hertz, p.damping_ratio, p.impulse}));
    if (p.hertz < 0.f || p.damping_ratio < 0.f) { set_error("%s: link %d: negative hertz or damping_ratio", what, k); return PHX_ERR_INVALID; }
    PHX_TRY(check_lengths(what, k, p.min_length, p.max_length, p.hertz));
    if (p.reserved != 0) { set_error("%s: link %d: reserved must be 0", what, k); return PHX_ERR_INVALID; }
    return PHX_OK;
}

int UnitKind<phx_link>::check_lengths(const char* what, int k, float lo, float hi, float hertz)
{
    if (!std::isfinite(lo) || !std::isfinite(hi)) { set_error("%s: link %d: a length is not finite", what, k); return PHX_ERR_INVALID; }
    if (!(0.f <= lo && lo <= hi)) { set_error("%s: link %d: lengths [%g, %g] are not 0 <= min <= max", what, k, (double)lo, (double)hi); return PHX_ERR_INVALID; }
    if (hertz > 0.f && lo != hi) { set_error("%s: link %d: a spring (hertz %g) needs min_length == max_length", what, k, (double)hertz); return PHX_ERR_INVALID; }
    return PHX_OK;
}

int UnitKind<phx_angle>::check(const char* what, int k, const phx_angle& p)
{
    PHX_TRY(check_finite(what, noun, k, {p.lower, p.upper, p.hertz, p.damping_ratio, p.motor_speed, p.max_torque, p.impulse, p.motor_impulse}));
    if (p.hertz < 0.f || p.damping_ratio < 0.f) { set_error("%s: angle %d: negative hertz or damping_ratio", what, k); return PHX_ERR_INVALID; }
    PHX_TRY(check_limits<phx_angle>(what, k, p.lower, p.upper, p.hertz));
    return check_motor<phx_angle>(what, k, p.motor_speed, p.max_torque);
}

template <class P> int check_limits(const char* what, int k, float lower, float upper, float hertz)
{
    const char* const noun = UnitKind<P>::noun;
    if (!std::isfinite(lower) || !std::isfinite(upper)) { set_error("%s: %s %d: a limit is not finite", what, noun, k); return PHX_ERR_INVALID; }
    if (!(lower <= upper)) { set_error("%s: %s %d: limits [%g, %g] are not lower <= upper", what, noun, k, (double)lower, (double)upper); return PHX_ERR_INVALID; }
    if (hertz > 0.f && lower != upper) { set_error("%s: %s %d: a spring (hertz %g) needs lower == upper", what, noun, k, (double)hertz); return PHX_ERR_INVALID; }
    return PHX_OK;
}

template <class P> int check_motor(const char* what, int k, float speed, float bound)
{
    const char* const noun = UnitKind<P>::noun;
    if (!std::isfinite(speed) || !std::isfinite(bound)) { set_error("%s: %s %d: a motor value is not finite", what, noun, k); return PHX_ERR_INVALID; }
    if (bound < 0.f) { set_error("%s: %s %d: negative %s %g", what, noun, k, UnitKind<P>::motor_bound, (double)bound); return PHX_ERR_INVALID; }
    return PHX_OK;
}

template int check_limits<phx_angle>(const char*, int, float, float, float);
template int check_limits<phx_slider>(const char*, int, float, float, float);
template int check_motor<phx_angle>(const char*, int, float, float);
template int check_motor<phx_slider>(const char*, int, float, float);

int UnitKind<phx_slider>::check(const char* what, int k, const phx_slider& p)
{
    PHX_TRY(check_finite(what, noun, k, {p.anchor1.x, p.anchor1.y, p.anchor2.x, p.anchor2.y, p.axis.x, p.axis.y, p.lower, p.upper, p.hertz, p.damping_ratio,
                                         p.motor_speed, p.max_force, p.impulse, p.axis_impulse, p.motor_impulse}));
    if (!(p.axis.x * p.axis.x + p.axis.y * p.axis.y > 0x1p-20f)) { set_error("%s: slider %d: axis (%g, %g) is too short to give a direction", what, k, (double)p.axis.x, (double)p.axis.y); return PHX_ERR_INVALID; }
    if (p.hertz < 0.f || p.damping_ratio < 0.f) { set_error("%s: slider %d: negative hertz or damping_ratio", what, k); return PHX_ERR_INVALID; }
    PHX_TRY(check_limits<phx_slider>(what, k, p.lower, p.upper, p.hertz));
    PHX_TRY(check_motor<phx_slider>(what, k, p.motor_speed, p.max_force));
    if (p.reserved != 0) { set_error("%s: slider %d: reserved must be 0", what, k); return PHX_ERR_INVALID; }
    return PHX_OK;
}

int PinSet::bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream)
{
    return each_list([&](auto& l) { return l.bodies_removed(d_remap, rb, stream, &sched_dirty_); });
}

int PinSet::settle(Readback& rb, hipStream_t stream)
{
    if (!breaks_pending_) return PHX_OK;
    unsigned count = 0;
    PHX_TRY(rb.add(&count, d_break_words_.p + BREAK_COUNT, sizeof count, stream));
    PHX_TRY(rb.wait(stream));
    breaks_pending_ = false;
    if (!count) return PHX_OK;
    std::vector<phx_break_event> events((size_t)count);
    PHX_TRY(rb.add(events.data(), d_events_.p, (size_t)count * sizeof(phx_break_event), stream));
    PHX_TRY(rb.wait(stream));
    // the events are in (kind, index) order: each list removes its own stretch, through the one copy of a removal
    int kind = 0;
    size_t at = 0;
    PHX_TRY(each_list([&](auto& l) -> int {
        std::vector<int32_t> which;
        for (; at < events.size() && events[at].kind == kind; ++at) which.push_back(events[at].index);
        ++kind;
        return which.empty() ? PHX_OK : l.remove(which.data(), (int)which.size(), stream);
    }));
    units_changed();
    // (a world whose last unit broke has no schedule to build at the next step: the rebuild a break stands for is the empty one, counted here)
    if (!units()) { sched_ = Schedule(); hbm_classes_.clear(); ++builds_; sched_dirty_ = false; }
    for (phx_break_event& e : events) { e.step = pending_step_; queue_.push_back(e); }
    return PHX_OK;
}

int PinSet::prepare(const float4* mpos, int nb, Readback& rb, hipStream_t stream)
{
    PHX_TRY(settle(rb, stream));                                            // (the last step's breaks leave before the schedule is looked at)
    const int n = units();
    if (!n) return PHX_OK;
    PHX_TRY(upload(stream));
    if (!sched_dirty_) return PHX_OK;
    PHX_TRY(d_bits_.reserve((size_t)n));
    // the units, kind behind kind: each list queues its records' static bits and appends their bodies
    std::vector<int32_t> b1, b2;
    b1.reserve((size_t)n); b2.reserve((size_t)n);
    PHX_TRY(each_list([&](auto& l) -> int {
        PHX_TRY(l.statics(mpos, d_bits_.p + b1.size(), stream));
        for (const auto& p : l.host()) { b1.push_back(p.body1); b2.push_back(p.body2); }
        return PHX_OK;
    }));
    std::vector<unsigned> bits((size_t)n);
    PHX_TRY(rb.add(bits.data(), d_bits_.p, (size_t)n * sizeof(unsigned), stream));
    PHX_TRY(rb.wait(stream));
    std::vector<unsigned char> is_static((size_t)nb, 0);
    for (int k = 0; k < n; ++k) {
        if (bits[(size_t)k] & 1u) is_static[(size_t)b1[(size_t)k]] = 1;
        if (b2[(size_t)k] >= 0 && (bits[(size_t)k] & 2u)) is_static[(size_t)b2[(size_t)k]] = 1;
    }
    build_pin_schedule(b1.data(), b2.data(), n, is_static.data(), nb, group_pins_, sched_);
    ++builds_;
    const Schedule& s = sched_;
    // the kernels' tables: a slot per pin, a record per LDS group, the LDS groups' bodies (the world: -1)
    const int lds_slots = s.lds_groups ? s.group_offsets[(size_t)s.lds_groups] : 0;
    std::vector<PinSlot> slots((size_t)n);
    for (int k = 0; k < n; ++k) {
        const int u = s.order[(size_t)k], ub1 = b1[(size_t)u], ub2 = b2[(size_t)u];
        if (k < lds_slots) {
            const uint32_t local = s.slot_local[(size_t)k];
            slots[(size_t)k] = PinSlot{u, (int)(local & 0xFFFFu), ub2 >= 0 ? (int)(local >> 16) : -1, (int)s.slot_colour[(size_t)k]};
        } else slots[(size_t)k] = PinSlot{u, ub1, ub2, 0};
    }
    std::vector<PinGroup> groups((size_t)s.lds_groups);
    std::vector<int> gbodies(s.group_bodies);
    for (int g = 0; g < s.lds_groups; ++g) {
        PinGroup& G = groups[(size_t)g];
        G.slot_begin = s.group_offsets[(size_t)g]; G.slot_end = s.group_offsets[(size_t)g + 1];
        G.body_begin = s.group_body_offsets[(size_t)g]; G.body_count = s.group_body_offsets[(size_t)g + 1] - G.body_begin;
        G.classes = s.group_first_colour[(size_t)g + 1] - s.group_first_colour[(size_t)g];
        G.first_dynamic = 0; G.pad0 = G.pad1 = 0;
        for (int i = 0; i < G.body_count; ++i) {
            int& b = gbodies[(size_t)(G.body_begin + i)];
            const bool fixed = b == nb || is_static[(size_t)b];
            if (fixed) {
                if (G.first_dynamic != i) { set_error("pin schedule: a static body behind a dynamic one in a group's body table"); return PHX_ERR_STATE; }
                G.first_dynamic = i + 1;
            }
            if (b == nb) b = -1;
        }
        if (G.slot_end - G.slot_begin > PIN_LANES || G.body_count > PIN_BODIES) { set_error("pin schedule: a group exceeds the workgroup"); return PHX_ERR_STATE; }
    }
    hbm_classes_ = s.hbm_colour_offsets;
    auto pad16 = [](size_t v) { return (v + 15) & ~size_t(15); };
    off_groups_ = pad16(slots.size() * sizeof(PinSlot));
    off_bodies_ = off_groups_ + pad16(groups.size() * sizeof(PinGroup));
    std::vector<char> blob(off_bodies_ + pad16(gbodies.size() * sizeof(int)) + 16, 0);
    std::memcpy(blob.data(), slots.data(), slots.size() * sizeof(PinSlot));
    if (!groups.empty()) std::memcpy(blob.data() + off_groups_, groups.data(), groups.size() * sizeof(PinGroup));
    if (!gbodies.empty()) std::memcpy(blob.data() + off_bodies_, gbodies.data(), gbodies.size() * sizeof(int));
    PHX_HIP(hipStreamSynchronize(stream));                                  // (a pass still queued may read the old tables)
    PHX_TRY(d_tables_.reserve(blob.size()));
    PHX_HIP(hipMemcpyAsync(d_tables_.p, blob.data(), blob.size(), hipMemcpyHostToDevice, stream));
    PHX_HIP(hipStreamSynchronize(stream));                                  // (`blob` is a local)
    // (a world with sliders keeps their side records behind the work array: pin_kernels.h RailWork)
    if (s.has_hbm_group()) PHX_TRY(d_work_.reserve((size_t)(s.hbm_end() - s.hbm_begin()) * (sizeof(PinWork) + (list<phx_slider>().count() ? sizeof(RailWork) : 0))));
    sched_dirty_ = false;
    return PHX_OK;
}

int PinSet::solve(const WorldBodies& bodies, int nb, float dt, int step, Readback& rb, hipStream_t stream)
{
    if (!units()) return PHX_OK;
    PHX_TRY(prepare(bodies.s.mpos, nb, rb, stream));
    phx_pin* const d_pins = list<phx_pin>().device();
    phx_link* const d_links = list<phx_link>().device();
    phx_angle* const d_angles = list<phx_angle>().device();
    phx_slider* const d_sliders = list<phx_slider>().device();
    const int np = list<phx_pin>().count(), nl = list<phx_link>().count(), na = list<phx_angle>().count(), ns = list<phx_slider>().count();
    const float beta = 0.2f / dt;
    const PinSlot* slots = reinterpret_cast<const PinSlot*>(d_tables_.p);
    // The world's level, picked once: `launch(LINKS, the later kinds' kernel arguments...)` names the instantiation of a kernel that
    // knows the kinds the world has.  A world without links runs the pins' own instantiation of each kernel: what it ran before there
    // were links; one without angles what it ran before there were angles; one with angles the instantiation that knows three kinds
    // (whose kernels take the angles' two arguments behind the others': pin_kernels.h AngleArgs); one with sliders the one that knows
    // all four (the sliders' arguments behind the angles': SliderArgs, and in the trailing group's kernels the side array `rail...`).
    auto level = [&](auto launch, auto... rail) {
        if (ns) launch(std::true_type{}, d_angles, nl, d_sliders, na, rail...);
        else if (na) launch(std::true_type{}, d_angles, nl);
        else if (nl) launch(std::true_type{});
        else launch(std::false_type{});
    };
    const float4* const mpos = (const float4*)bodies.s.mpos, *const frame = (const float4*)bodies.frame;
    if (sched_.lds_groups) {
        const PinGroup* const groups = reinterpret_cast<const PinGroup*>(d_tables_.p + off_groups_);
        const int* const group_bodies = reinterpret_cast<const int*>(d_tables_.p + off_bodies_);
        level([&](auto links, auto... later) {
            hipLaunchKernelGGL((k_solve_pins<decltype(links)::value, decltype(later)...>), dim3(sched_.lds_groups), dim3(PIN_LANES), 0, stream, d_pins, d_links, np, slots, groups,
                               group_bodies, bodies.s.vel, mpos, frame, beta, dt, iterations, later...);
        });
    }
    if (hbm_classes_.size() > 1) {
        const int begin = hbm_classes_.front(), end = hbm_classes_.back();
        PinWork* work = reinterpret_cast<PinWork*>(d_work_.p);
        RailWork* const rail = reinterpret_cast<RailWork*>(work + (end - begin));      // (only a world with sliders has it)
        level([&](auto links, auto... later) {
            hipLaunchKernelGGL((k_pin_prestep<decltype(links)::value, decltype(later)...>), dim3(pgrid(end - begin)), dim3(256), 0, stream, d_pins, d_links, np, slots, begin, end,
                               mpos, frame, beta, dt, work, later...);
        }, rail);
        for (int sweep = 0; sweep <= iterations; ++sweep)
            for (size_t c = 0; c + 1 < hbm_classes_.size(); ++c) {
                const int b = hbm_classes_[c], e = hbm_classes_[c + 1];
                if (e <= b) continue;
                level([&](auto links, auto... later) {
                    hipLaunchKernelGGL((k_pin_class<decltype(links)::value, decltype(later)...>), dim3(pgrid(e - b)), dim3(256), 0, stream, d_pins, d_links, np, slots, b, e, begin,
                                       (const PinWork*)work, bodies.s.vel, sweep, later...);
                }, rail);
            }
    }
    PHX_HIP(hipGetLastError());
    if (!limited()) return PHX_OK;
    // the break test, behind the pass's last kernel: over the lists that have a limit column
    BreakLists l = {};
    l.pins = d_pins; l.links = d_links; l.angles = d_angles; l.sliders = d_sliders;
    l.pin_limits = list<phx_pin>().device_limits(); l.link_limits = list<phx_link>().device_limits();
    l.angle_limits = list<phx_angle>().device_limits(); l.slider_limits = list<phx_slider>().device_limits();
    l.end[0] = l.pin_limits ? np : 0;
    l.end[1] = l.end[0] + (l.link_limits ? nl : 0);
    l.end[2] = l.end[1] + (l.angle_limits ? na : 0);
    l.end[3] = l.end[2] + (l.slider_limits ? ns : 0);
    const int n = l.end[3];
    if (!n) return PHX_OK;
    if (!d_break_words_.p) {
        PHX_TRY(d_break_words_.reserve(BREAK_WORDS));
        PHX_HIP(hipMemsetAsync(d_break_words_.p, 0, BREAK_WORDS * sizeof(unsigned), stream));
    }
    PHX_TRY(d_staged_.reserve((size_t)n)); PHX_TRY(d_events_.reserve((size_t)n));
    const int tiles = div_up(n, BREAK_LANES), chunk = div_up(tiles, BREAK_BLOCKS) * BREAK_LANES;
    hipLaunchKernelGGL(k_unit_breaks, dim3(div_up(n, chunk)), dim3(BREAK_LANES), 0, stream, l, dt, chunk, d_staged_.p, d_break_words_.p, d_events_.p);
    PHX_HIP(hipGetLastError());
    breaks_pending_ = true; pending_step_ = step;
    return PHX_OK;
}

} // namespace phx

// ---- C ABI: the host-only builder (the world's calls: c_api_world.hip) ----
extern "C" int phx_pin_schedule(const int32_t* body1, const int32_t* body2, int32_t pin_count, const uint8_t* is_static, int32_t body_count, int32_t group_pins,
                                int32_t* order, int32_t* class_offsets, int32_t class_cap, int32_t* class_count,
                                int32_t* group_offsets, int32_t group_cap, int32_t* group_count, int32_t* lds_group_count)
{
    PHX_REQUIRE(pin_count >= 0 && body_count >= 0 && (pin_count == 0 || (body1 && body2)) && (body_count == 0 || is_static) && class_count && group_count && lds_group_count,
                "phx_pin_schedule: bad arguments");
    PHX_REQUIRE(group_pins >= 1 && group_pins <= phx::PIN_LANES, "phx_pin_schedule: group_pins out of [1, 256]");
    for (int k = 0; k < pin_count; ++k)
        PHX_REQUIRE((unsigned)body1[k] < (unsigned)body_count && (body2[k] == -1 || (unsigned)body2[k] < (unsigned)body_count) && body1[k] != body2[k], "phx_pin_schedule: bad body index");
    phx::Schedule s;
    phx::build_pin_schedule(body1, body2, pin_count, is_static, body_count, group_pins, s);
    *class_count = (int)s.colour_offsets.size() - 1; *group_count = s.ngroups(); *lds_group_count = s.lds_groups;
    if (!order && !class_offsets && !group_offsets) return PHX_OK;
    if ((pin_count && !order) || !class_offsets || !group_offsets) { phx::set_error("phx_pin_schedule: null output"); return PHX_ERR_INVALID; }
    if ((int)s.colour_offsets.size() > class_cap || s.ngroups() + 1 > group_cap) { phx::set_error("phx_pin_schedule: offsets arrays too small"); return PHX_ERR_CAPACITY; }
    std::copy(s.order.begin(), s.order.end(), order);
    std::copy(s.colour_offsets.begin(), s.colour_offsets.end(), class_offsets);
    std::copy(s.group_offsets.begin(), s.group_offsets.end(), group_offsets);
    return PHX_OK;
}
