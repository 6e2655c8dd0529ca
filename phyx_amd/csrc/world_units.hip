// world_units.hip — World (world.h): the World's side of pins.h, sleep.h and fields.h: the calls on units (pins, links, angles, sliders),
// breaks, sleeping and force fields, and the place of their passes in the step.
#include "world.h"

namespace phx {

// ---- units: pins, links, angles and sliders --------------------------------------------------------------------------------------------------------
// The rules and the arithmetic: include/phyx_amd.h PINS, LINKS, ANGLES, SLIDERS; the lists, the schedule and the pass: pins.h.  One copy of the calls for
// both records (`P`; what differs is UnitKind<P>): they check everything first — inside a step, sharded, count, null, overflow, the
// entries in order — then change the list; the schedule follows lazily at the next step.
template <class P>
int World::check_unit_indices(const char* what, const int32_t* which, const void* values, int count)
{
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(settle_breaks());
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && (!which || !values)) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    const int n = pins_.list<P>().count();
    const char* const noun = UnitKind<P>::noun;
    std::vector<unsigned char> seen((size_t)n, 0);
    for (int k = 0; k < count; ++k) {
        if (which[k] < 0 || which[k] >= n) { set_error("%s: %s index %d out of range [0, %d)", what, noun, which[k], n); return PHX_ERR_INVALID; }
        if (seen[(size_t)which[k]]) { set_error("%s: %s %d appears twice in one call", what, noun, which[k]); return PHX_ERR_INVALID; }
        seen[(size_t)which[k]] = 1;
    }
    return PHX_OK;
}

// the body rules of entry k of an add (the record's own: UnitKind<P>::check)
int World::check_unit_bodies(const char* what, const char* noun, int k, int body1, int body2)
{
    const int n = nb();
    if (body1 < 0 || body1 >= n) { set_error("%s: %s %d: body1 %d out of range [0, %d)", what, noun, k, body1, n); return PHX_ERR_INVALID; }
    if (body2 < -1 || body2 >= n) { set_error("%s: %s %d: body2 %d is neither -1 nor in [0, %d)", what, noun, k, body2, n); return PHX_ERR_INVALID; }
    if (body1 == body2) { set_error("%s: %s %d: both ends on body %d", what, noun, k, body1); return PHX_ERR_INVALID; }
    return PHX_OK;
}

template <class P>
int World::add_units(const P* recs, int count, int* first)
{
    using Kind = UnitKind<P>;
    const char* const what = Kind::add;
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, Kind::plural));
    PHX_TRY(settle_breaks());
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count && !recs) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    // (the schedule numbers the units, pins, links, angles and sliders together, in an int32)
    if ((long long)pins_.units() + count > (long long)INT32_MAX) { set_error("%s: %d + %d units exceed the int32 range", what, pins_.units(), count); return PHX_ERR_INVALID; }
    for (int k = 0; k < count; ++k) {
        PHX_TRY(check_unit_bodies(what, Kind::noun, k, recs[k].body1, recs[k].body2));
        PHX_TRY(Kind::check(what, k, recs[k]));
    }
    UnitList<P>& list = pins_.list<P>();
    if (first) *first = list.count();
    if (!count) return PHX_OK;
    if (sleep_col_.active) {                                                // (the new units' bodies)
        std::vector<int> named;
        for (int k = 0; k < count; ++k) { named.push_back(recs[k].body1); if (recs[k].body2 >= 0) named.push_back(recs[k].body2); }
        PHX_TRY(wake_named(named.data(), (int)named.size()));
    }
    PHX_TRY(settle_on_device());
    pins_.units_changed();
    return list.add(recs, count, stream_);
}

template <class P>
int World::remove_units(const int32_t* which, int count)
{
    PHX_TRY(check_unit_indices<P>(UnitKind<P>::remove, which, which, count));
    if (!count) return PHX_OK;
    PHX_TRY(wake_units<P>(which, count));
    PHX_TRY(settle_on_device());
    pins_.units_changed();
    return pins_.list<P>().remove(which, count, stream_);
}

template <class P, class Fields>
int World::set_unit_fields(const int32_t* which, const float* values, int count)
{
    if (!count) return PHX_OK;
    PHX_TRY(wake_units<P>(which, count));
    UnitList<P>& list = pins_.list<P>();
    const int* d_which = nullptr; const float* d_values = nullptr;
    if (list.on_device()) {
        PHX_TRY(settle_on_device());
        PHX_TRY(stage_.indexed(which, values, count, Fields::width, stream_, &d_which, &d_values));
    }
    return list.template set_fields<Fields>(which, values, count, d_which, d_values, stream_);
}

template <class P>
int World::set_unit_anchors(const int32_t* which, const float* anchors, int count)
{
    const char* const what = UnitKind<P>::set_anchors;
    PHX_TRY(check_unit_indices<P>(what, which, anchors, count));
    for (int k = 0; k < 4 * count; ++k)
        if (!std::isfinite(anchors[k])) { set_error("%s: entry %d: value %d is not finite", what, k / 4, k % 4); return PHX_ERR_INVALID; }
    return set_unit_fields<P, AnchorFields>(which, anchors, count);
}

int World::set_link_lengths(const int32_t* which, const float* lengths, int count)
{
    static const char* const what = "phx_world_set_link_lengths";
    PHX_TRY(check_unit_indices<phx_link>(what, which, lengths, count));
    const std::vector<phx_link>& links = pins_.list<phx_link>().host();     // (bodies, anchors, lengths, hertz: always current)
    for (int k = 0; k < count; ++k)
        PHX_TRY(UnitKind<phx_link>::check_lengths(what, k, lengths[2 * k], lengths[2 * k + 1], links[(size_t)which[k]].hertz));
    return set_unit_fields<phx_link, LengthFields>(which, lengths, count);
}

template <class P>
int World::set_unit_limits(const int32_t* which, const float* limits, int count)
{
    const char* const what = UnitKind<P>::set_limits;
    PHX_TRY(check_unit_indices<P>(what, which, limits, count));
    const std::vector<P>& units = pins_.list<P>().host();                   // (bodies, limits, hertz, motor: always current)
    for (int k = 0; k < count; ++k)
        PHX_TRY(check_limits<P>(what, k, limits[2 * k], limits[2 * k + 1], units[(size_t)which[k]].hertz));
    return set_unit_fields<P, LimitFields>(which, limits, count);
}

template <class P>
int World::set_unit_motors(const int32_t* which, const float* motors, int count)
{
    const char* const what = UnitKind<P>::set_motors;
    PHX_TRY(check_unit_indices<P>(what, which, motors, count));
    for (int k = 0; k < count; ++k) PHX_TRY(check_motor<P>(what, k, motors[2 * k], motors[2 * k + 1]));
    return set_unit_fields<P, MotorFields>(which, motors, count);
}

template <class P>
int World::get_units(P* out, int cap)
{
    PHX_TRY(settle_breaks());
    UnitList<P>& list = pins_.list<P>();
    const int n = list.count();
    if (cap < n) { set_error("%s: room for %d %s, the world has %d", UnitKind<P>::get, cap, UnitKind<P>::plural, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    return list.get(out, stream_);
}

template <class P>
int World::unit_count(int* out)
{
    PHX_TRY(settle_breaks());
    *out = pins_.list<P>().count();
    return PHX_OK;
}

// the C surface (c_api_world.hip) calls these for each record: instantiated here, where their bodies are
#define PHX_UNIT_CALLS(P)                                                       \
    template int World::add_units<P>(const P*, int, int*);                       \
    template int World::remove_units<P>(const int32_t*, int);                    \
    template int World::get_units<P>(P*, int);                                   \
    template int World::unit_count<P>(int*);
PHX_UNIT_CALLS(phx_pin) PHX_UNIT_CALLS(phx_link) PHX_UNIT_CALLS(phx_angle) PHX_UNIT_CALLS(phx_slider)
#undef PHX_UNIT_CALLS
#define PHX_UNIT_EDIT(call, P) template int World::call<P>(const int32_t*, const float*, int);
PHX_UNIT_EDIT(set_unit_anchors, phx_pin) PHX_UNIT_EDIT(set_unit_anchors, phx_link) PHX_UNIT_EDIT(set_unit_anchors, phx_slider)
PHX_UNIT_EDIT(set_unit_limits, phx_angle) PHX_UNIT_EDIT(set_unit_limits, phx_slider) PHX_UNIT_EDIT(set_unit_motors, phx_angle) PHX_UNIT_EDIT(set_unit_motors, phx_slider)
#undef PHX_UNIT_EDIT

// ---- breaks ---------------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h BREAKS; the test runs behind the pass (PinSet::solve) and is settled here, lazily.
int World::settle_breaks()
{
    if (mid_step_ || !pins_.breaks_pending()) return PHX_OK;
    PHX_TRY(use_device(device_));
    PHX_TRY(solver_.synchronize());
    return pins_.settle(rb_, stream_);
}

// f(a P*) for the record of `kind`
template <class F> static int with_kind(const char* what, int kind, F f)
{
    switch (kind) {
    case PHX_UNIT_PIN: return f((phx_pin*)nullptr);
    case PHX_UNIT_LINK: return f((phx_link*)nullptr);
    case PHX_UNIT_ANGLE: return f((phx_angle*)nullptr);
    case PHX_UNIT_SLIDER: return f((phx_slider*)nullptr);
    }
    set_error("%s: kind %d is none of PHX_UNIT_PIN ... PHX_UNIT_SLIDER [0, 3]", what, kind);
    return PHX_ERR_INVALID;
}

int World::set_break_limits(int kind, const int32_t* which, const float* limits, int count)
{
    static const char* const what = "phx_world_set_break_limits";
    PHX_TRY(refuse_mid_step(what));
    return with_kind(what, kind, [&](auto* tag) -> int {
        using P = std::remove_pointer_t<decltype(tag)>;
        PHX_TRY(check_unit_indices<P>(what, which, limits, count));
        for (int k = 0; k < count; ++k)
            if (!(limits[k] > 0.f)) { set_error("%s: %s %d: break limit %g is not > 0", what, UnitKind<P>::noun, k, (double)limits[k]); return PHX_ERR_INVALID; }
        if (!count) return PHX_OK;
        PHX_TRY(wake_units<P>(which, count));
        UnitList<P>& list = pins_.list<P>();
        const int* d_which = nullptr; const float* d_values = nullptr;
        if (list.on_device()) {
            PHX_TRY(settle_on_device());
            if (list.limited()) PHX_TRY(stage_.indexed(which, limits, count, 1, stream_, &d_which, &d_values));
        }
        return list.set_limits(which, limits, count, d_which, d_values, stream_);
    });
}

int World::get_break_limits(int kind, float* out, int cap)
{
    static const char* const what = "phx_world_get_break_limits";
    PHX_TRY(refuse_mid_step(what));
    return with_kind(what, kind, [&](auto* tag) -> int {
        using P = std::remove_pointer_t<decltype(tag)>;
        PHX_TRY(settle_breaks());
        const UnitList<P>& list = pins_.list<P>();
        if (cap < list.count()) { set_error("%s: room for %d %s, the world has %d", what, cap, UnitKind<P>::plural, list.count()); return PHX_ERR_CAPACITY; }
        list.get_limits(out);
        return PHX_OK;
    });
}

int World::break_events(phx_break_event* out, int cap, int64_t* total)
{
    static const char* const what = "phx_world_break_events";
    PHX_TRY(refuse_mid_step(what));
    if (cap < 0) { set_error("%s: negative cap %d", what, cap); return PHX_ERR_INVALID; }
    PHX_TRY(settle_breaks());
    std::vector<phx_break_event>& queue = pins_.break_queue();
    *total = (int64_t)queue.size();
    if ((int64_t)cap < *total) { set_error("%s: room for %d events, the queue holds %lld", what, cap, (long long)*total); return PHX_ERR_CAPACITY; }
    std::copy(queue.begin(), queue.end(), out);
    queue.clear();
    break_step_ = 0;
    return PHX_OK;
}

int World::set_pin_iterations(int n)
{
    PHX_TRY(refuse_mid_step("phx_world_set_pin_iterations"));
    if (n < 1 || n > PIN_MAX_ITERATIONS) { set_error("phx_world_set_pin_iterations: %d is not in [1, %d]", n, PIN_MAX_ITERATIONS); return PHX_ERR_INVALID; }
    pins_.iterations = n;
    return PHX_OK;
}

int World::pin_schedule(const Schedule** out)
{
    PHX_TRY(refuse_mid_step("phx_world_get_pin_schedule"));
    *out = nullptr;
    PHX_TRY(settle_breaks());
    if (!pins_.units()) return PHX_OK;
    PHX_TRY(settle_and_upload());
    PHX_TRY(settle_sleep_count());                                          // (bodies the last pass put to sleep or woke are part of the static set)
    PHX_TRY(pins_.prepare(bodies_.mpos.p, nb(), rb_, stream_));
    *out = &pins_.schedule();
    return PHX_OK;
}

// ---- sleeping ---------------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h SLEEPING, tests/sleep_spec.py; the column, the pass and the wake by list: sleep.h.  Here: the calls, the
// place of the pass in the step, and how the host learns that the static set changed — the device counts the bodies the pass (or a wake)
// put to sleep or woke, and the next step's joint-count readback brings the count along (refresh_contact_joints), in front of the
// solve and of the pin pass, which are what consult the static set.
SleepGraph World::sleep_graph()
{
    SleepGraph g = {};
    g.manifolds = d_manifolds_.p; g.nm = nm; g.flags = flags_col_.ptr();
    int kind = 0;
    pins_.each_list([&](auto& l) {
        using P = typename std::decay_t<decltype(l)>::record;
        static_assert(offsetof(P, body1) == 0 && offsetof(P, body2) == 4, "a unit's record begins with its bodies");
        g.units[kind++] = SleepGraph::List{reinterpret_cast<const char*>(l.device()), (int)sizeof(P), l.count()};
        return PHX_OK;
    });
    return g;
}

int World::sleep_pass(float dt)
{
    if (!nb()) return PHX_OK;
    if (pins_.units()) PHX_TRY(pins_.upload(stream_));                      // (current already behind a pin pass: nothing is copied)
    PHX_TRY(sleep_.pass(resident(), bodies_.records.p, sleep_col_.dev.p, nb(), sleep_graph(), dt, stream_));
    sleep_count_pending_ = true;
    return PHX_OK;
}

// ---- continuous bodies ---------------------------------------------------------------------------------------------------------------
// The rule: include/phyx_amd.h CONTINUOUS BODIES, tests/sweep_spec.py; the list, the launches and the hits: sweep.h.  Here: the place of
// the two launches in the step.  The pass moves a clamped body's position and AABB behind IntegratePosition, inside the step whose
// integrator has already moved the geometry epoch and whose pre_solve the contact epoch: neither index needs anything new.
int World::sweep_begin()
{
    if (!nb()) return PHX_OK;
    return sweep_.begin(bodies_.mpos.p, sweep_col_.dev.p, nb(), rb_, stream_);
}

int World::sweep_pass()
{
    if (!nb()) return PHX_OK;                                               // (an empty list still ends the last pass's hits)
    WorldBodies w = bodies_.view();
    w.kinds = shapes_.ptr(); w.polys = polygons() ? polys_.ptr() : nullptr;
    const ExclusionView* x = exclusions_.view();
    const SweepTables tables = {filters_.ptr(), flags_col_.ptr(), x ? x->table : nullptr, x ? x->mask : 0u, x ? x->member : nullptr};
    const int shapes = !shapes_.ptr() ? SWEEP_BOXES : (polygons() ? SWEEP_POLYGONS : (capsules() ? SWEEP_CAPSULES : SWEEP_SHAPES));
    return sweep_.pass(w, sweep_col_.dev.p, nb(), tables, shapes, stream_);
}

void World::take_sleep_count(unsigned changed)
{
    sleep_count_pending_ = false;
    if (!changed) return;
    joints_changed_ = true;                                                 // which bodies are static is part of the schedule's topology
    pins_.statics_changed();
}

int World::settle_sleep_count()
{
    if (!sleep_count_pending_) return PHX_OK;
    unsigned changed = 0;
    PHX_TRY(rb_.add(&changed, sleep_.words() + SLEEP_CHANGED, sizeof changed, stream_));
    PHX_TRY(rb_.wait(stream_));
    take_sleep_count(changed);
    return PHX_OK;
}

int World::wake_named(const int* bodies, int count, const unsigned* d_keep, bool all)
{
    if (!sleep_col_.active || !nb() || (!all && !d_keep && !count)) return PHX_OK;
    PHX_TRY(settle_breaks());                                               // (a unit that broke in the last step is no edge any more)
    PHX_TRY(settle_and_upload());                                           // (an unverified solve is settled before masses change; the column goes up with the bodies)
    if (pins_.units()) PHX_TRY(pins_.upload(stream_));
    const int* d_list = nullptr;
    if (!all && !d_keep) PHX_TRY(stage_.indices(bodies, count, stream_, &d_list));
    PHX_TRY(sleep_.wake(resident(), bodies_.records.p, sleep_col_.dev.p, nb(), sleep_graph(), d_list, count, d_keep, all, stream_));
    sleep_count_pending_ = true;
    return PHX_OK;
}

template <class P>
int World::wake_units(const int32_t* which, int count)
{
    if (!sleep_col_.active || !count) return PHX_OK;
    const std::vector<P>& units = pins_.list<P>().host();                   // (the bodies: always current)
    std::vector<int> named;
    for (int k = 0; k < count; ++k) {
        const P& u = units[(size_t)which[k]];
        named.push_back(u.body1);
        if (u.body2 >= 0) named.push_back(u.body2);
    }
    return wake_named(named.data(), (int)named.size());
}

int World::set_sleeping(const phx_sleep_params* p)
{
    static const char* const what = "phx_world_set_sleeping";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, SleepColumn::plural));
    if (!p) {
        if (!sleep_.on()) return PHX_OK;
        PHX_TRY(wake_named(nullptr, 0, nullptr, true));                     // every mass is its own again, byte for byte
        sleep_.disable();
        sleep_col_.reset();
        return PHX_OK;
    }
    const float v[3] = {p->linear_tolerance, p->angular_tolerance, p->time_to_sleep};
    static const char* const names[3] = {"linear_tolerance", "angular_tolerance", "time_to_sleep"};
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(v[k]) || !(v[k] >= 0.f)) { set_error("%s: %s %g must be finite and >= 0", what, names[k], (double)v[k]); return PHX_ERR_INVALID; }
    PHX_TRY(use_device(device_));
    if (!sleep_col_.active) {                                               // the column: every body awake, timer 0
        if (host_staged()) sleep_col_.host.assign((size_t)nb(), SleepColumn::initial());
        else {
            PHX_TRY(settle_on_device());
            PHX_TRY(sleep_col_.dev.reserve((size_t)std::max(nb(), 1)));
            PHX_TRY(sleep_.fill(sleep_col_.dev.p, nb(), stream_));
        }
        sleep_col_.active = true;
    }
    return sleep_.enable(*p, stream_);
}

int World::get_sleeping(phx_sleep_params* out, int32_t* enabled) const
{
    if (out) *out = sleep_.params();
    if (enabled) *enabled = sleep_.on() ? 1 : 0;
    return PHX_OK;
}

int World::get_sleep_states(phx_sleep_state* out, int cap)
{
    static const char* const what = "phx_world_get_sleep_states";
    PHX_TRY(refuse_mid_step(what));
    const int n = nb();
    if (cap < n) { set_error("%s: room for %d bodies, the world has %d", what, cap, n); return PHX_ERR_CAPACITY; }
    if (!n) return PHX_OK;
    PHX_TRY(settle_and_upload());
    PHX_TRY(sleep_out_.reserve((size_t)n));
    PHX_TRY(sleep_.states(bodies_.mpos.p, sleep_col_.ptr(), n, sleep_out_.p, stream_));
    PHX_TRY(rb_.add(out, sleep_out_.p, (size_t)n * sizeof(phx_sleep_state), stream_));
    return rb_.wait(stream_);
}

int World::wake_bodies(const int32_t* bodies, int count)
{
    static const char* const what = "phx_world_wake_bodies";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, SleepColumn::plural));
    PHX_TRY(check_batch(what, bodies, bodies, count, false));              // (no values: the indices stand in for them; a body may be named twice)
    return wake_named(bodies, count);
}

int World::sleep_counts(int32_t* asleep, int64_t* slept_total, int64_t* woken_total)
{
    PHX_TRY(refuse_mid_step("phx_world_sleep_counts"));
    unsigned long long totals[2] = {0, 0};
    if (sleep_.words()) {
        PHX_TRY(use_device(device_));
        PHX_TRY(solver_.synchronize());
        PHX_TRY(rb_.add(totals, sleep_.words() + SLEEP_SLEPT, sizeof totals, stream_));
        PHX_TRY(rb_.wait(stream_));
    }
    if (asleep) *asleep = (int32_t)(totals[0] - totals[1]);
    if (slept_total) *slept_total = (int64_t)totals[0];
    if (woken_total) *woken_total = (int64_t)totals[1];
    return PHX_OK;
}

int World::set_gravity(float g)
{
    if (sleep_.on()) {                                                      // a change of gravity disturbs every pile
        PHX_TRY(refuse_mid_step("phx_world_set_gravity"));
        PHX_TRY(wake_named(nullptr, 0, nullptr, true));
    }
    gravity = g;
    return PHX_OK;
}

// ---- force fields ---------------------------------------------------------------------------------------------------------------------
// The rules and the arithmetic: include/phyx_amd.h FORCE FIELDS; the list, its device copy and the launches: fields.h.  The world's part
// is the seam: the pass fills accel_, the dense pending accelerations the unchanged IntegrateVelocity consumes (fused into the
// broadphase's first kernel or on its own under phase timing), so no kernel of the step knows about fields.
int World::set_fields(const phx_field* fields, int count)
{
    static const char* const what = "phx_world_set_fields";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, "force fields"));
    PHX_TRY(phx_field_check(fields, count));
    const float* d_fields = nullptr;
    if (count) {
        PHX_TRY(use_device(device_));
        PHX_TRY(stage_.values(reinterpret_cast<const float*>(fields), count, (int)(sizeof(phx_field) / sizeof(float)), stream_, &d_fields));
    }
    return fields_.set(fields, count, reinterpret_cast<const phx_field*>(d_fields), stream_);
}

int World::get_fields(phx_field* out, int cap, int32_t* count) const
{
    const int n = fields_.count();
    if (count) *count = n;
    if (cap < n || (n && !out)) { set_error("phx_world_get_fields: room for %d fields, the world has %d", out ? cap : 0, n); return PHX_ERR_CAPACITY; }
    if (n) std::memcpy(out, fields_.list().data(), (size_t)n * sizeof(phx_field));
    return PHX_OK;
}

int World::field_pass(float dt)
{
    accel_from_fields_ = false;
    if (!fields_.count() || !nb()) return PHX_OK;
    // (pending accelerations fill accel_ for every body already; otherwise the kernel starts every slot from zero itself)
    if (!accel_pending_) PHX_TRY(accel_.reserve((size_t)nb()));
    PHX_TRY(fields_.apply(field_bodies(), accel_.p, accel_pending_, dt, stream_));
    accel_from_fields_ = !accel_pending_;
    accel_pending_ = true;
    return PHX_OK;
}

int World::pulse_fields(const phx_field* fields, int count)
{
    static const char* const what = "phx_world_pulse_fields";
    PHX_TRY(refuse_mid_step(what));
    PHX_TRY(refuse_sharded(what, "force fields"));
    PHX_TRY(phx_field_check(fields, count));
    if (!count || !nb()) return PHX_OK;
    PHX_TRY(settle_on_device());
    PHX_TRY(sync_bodies_to_device());                                       // (host-staged bodies go up as the next step would take them)
    const float* d_fields = nullptr;
    PHX_TRY(stage_.values(reinterpret_cast<const float*>(fields), count, (int)(sizeof(phx_field) / sizeof(float)), stream_, &d_fields));
    records_stale_ = true;
    return DeviceFields::pulse(field_bodies(), reinterpret_cast<const phx_field*>(d_fields), count, field_traits(fields, count), stream_);
}

int World::apply_impulses(const int* bodies, const float* impulses, int count)
{
    static const char* const what = "phx_world_apply_impulses";
    PHX_TRY(check_batch(what, bodies, impulses, count, true));
    for (int k = 0; k < 4 * count; ++k)
        if (!std::isfinite(impulses[k])) { set_error("%s: entry %d: value %d is not finite", what, k / 4, k % 4); return PHX_ERR_INVALID; }
    if (!count) return PHX_OK;
    PHX_TRY(wake_named(bodies, count));
    if (host_staged()) {                                    // the host-staged records are the world: the kernel's statements on them
        for (int k = 0; k < count; ++k) {
            phx_rigid_body& b = host_bodies_[(size_t)bodies[k]];
            if (!(b.inv_mass > 0.0f)) continue;
            const float* q = impulses + 4 * (size_t)k;
            const float rx = q[2] - b.pos.x, ry = q[3] - b.pos.y;
            b.velocity.x = b.velocity.x + b.inv_mass * q[0]; b.velocity.y = b.velocity.y + b.inv_mass * q[1];
            b.angular_velocity = b.angular_velocity - b.inv_inertia * (rx * q[1] - ry * q[0]);
        }
        return PHX_OK;
    }
    PHX_TRY(settle_on_device());
    const int* d_bodies = nullptr; const float* d_values = nullptr;
    PHX_TRY(stage_.indexed(bodies, impulses, count, 4, stream_, &d_bodies, &d_values));
    records_stale_ = true;
    return DeviceFields::impulses(field_bodies(), d_bodies, d_values, count, stream_);
}

} // namespace phx
