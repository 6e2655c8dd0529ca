// pin_kernels.h — the pin pass (include/phyx_amd.h PINS; the definition: tests/pin_spec.py).
//
// One copy of the arithmetic (pin_prestep, pin_delta, pin_apply_*), written operation for operation as the spec writes it; the library
// is built with -ffp-contract=off -fno-fast-math, so every product and sum below is rounded on its own in either PHX_ARITH mode.
//   k_solve_pins     one workgroup per LDS group, the whole pass in ONE launch: the group's body velocities are staged in LDS (16 bytes
//                    per body, the only thing staged), one lane owns one pin and keeps ra, rb, k11, k12, k22, 1/det, bias and the
//                    impulse in registers from the prestep to the write-back; classes are body-disjoint, so a class is one parallel
//                    step and a barrier separates it from the next.
//   k_pin_prestep /  the trailing group, out of HBM: the prestep leaves the lanes' registers in a work array, then one launch per
//   k_pin_class      class for the warm start and per class and sweep (the fallback, not the fast path).
// Static bodies (both inverses 0) and the world are read, never written: a class may share them among its lanes.
//
// The pass has four kinds of unit, in this order among the units: pins, links (include/phyx_amd.h LINKS; tests/link_spec.py), angles
// (ANGLES; tests/angle_spec.py) and sliders (SLIDERS; tests/slider_spec.py).  Unit u is pin u, else link u - npins, else angle
// u - npins - nlinks, else slider u - npins - nlinks - nangles: that ladder is written where a unit's record is first needed (the
// prestep in k_solve_pins and in k_pin_prestep, unit_store, work_unpack) and nowhere else.  Every kind keeps its lane state in PinRegs:
//   a link    fills the same registers under other names (PinRegs' unions); its sweep differs in the delta only (link_delta) and ends
//             in the same pin_apply;
//   an angle  has no anchors and no axis: its two rows, the motor M and the lock / spring / limit L, live in the registers a pin uses
//             for its anchors, and its sweep (angle_sweep) edits the two angular velocities only;
//   a slider  has three scalar rows (M and L along the rail, the hard row P across it) at one point with two arms: a link's registers
//             (ra, rb' = rb + e, n, row L) in PinRegs and seven words more (RailRegs), which exist only in the instantiations with sliders.
// What the kinds share is written once: the anchors (pin_anchors), a limited row's engagement (limit_row), the soft row (soft_row),
// the two clamped accumulations (row_accumulate, motor_accumulate), a class step (unit_step) and the trailing group's record
// (work_pack / work_unpack).
#pragma once

#include "pins.h"
#include "device_scan.h"

namespace phx {


// a slot of the schedule as the kernels read it
struct PinSlot { int pin; int a, b; int colour; };      // LDS groups: a, b local body indices (b = -1: the world); HBM group: global ones
// an LDS group: its slots, its bodies in `group_bodies` (the static ones first), its classes
struct PinGroup { int slot_begin, slot_end, body_begin, body_count; int first_dynamic, classes, pad0, pad1; };

// A unit's kind and bits, the one encoding of both PinRegs::kind (the kind and its engaged rows: the bits of UNIT_KIND) and the
// trailing group's PinWork::flags (those and the lane's four bools).  An angle is UNIT_ANGLE | its engaged rows, a slider UNIT_SLIDER | its rows L, M.
enum : int { UNIT_PIN = 0, UNIT_LINK = 1, UNIT_ANGLE = 2, UNIT_ROW_L = 4, UNIT_ROW_M = 8, UNIT_SLIDER = 16, UNIT_KIND = 31,
             UNIT_ACTIVE = 32, UNIT_WRITE_A = 64, UNIT_WRITE_B = 128, UNIT_CLAMPS = 256 };

// what a lane keeps of its pin from the prestep on
// (a link's names for the registers a pin calls otherwise: the axis n, gamma, 1/kinv, the scalar bias, the clamp's bounds, lambda;
//  an angle's: row L as a link's with 1/(kinv + gamma) beside 1/kinv, row M's speed, its largest impulse and its accumulated impulse)
struct PinRegs {
    float rax, ray, rbx, rby;           // (an angle's inv_kg, speed, mmax, mlambda: the accessors below)
    union { float k11; float nx; };
    union { float k12; float ny; };
    union { float k22; float gamma; };
    union { float inv_det; float inv_k; };
    union { float biasx; float bias; };
    union { float biasy; float lo; };
    float ma, ia, mb, ib;
    union { float px; float lambda; };  // the accumulated impulse
    union { float py; float hi; };
    bool active, write_a, write_b;
    unsigned char kind;                 // UNIT_PIN, UNIT_LINK, or UNIT_ANGLE / UNIT_SLIDER with UNIT_ROW_L / UNIT_ROW_M where those rows are engaged
    bool clamps;                        // a link, an angle or a slider whose row L is clamped to [lo, hi] (a rope or a limit)
    __device__ float& inv_kg() { return rax; }
    __device__ float& speed() { return ray; }
    __device__ float& mmax() { return rbx; }
    __device__ float& mlambda() { return rby; }
    __device__ float inv_kg() const { return rax; }
    __device__ float speed() const { return ray; }
    __device__ float mmax() const { return rbx; }
    __device__ float mlambda() const { return rby; }
    __device__ bool angle() const { return (kind & UNIT_ANGLE) != 0; }
    __device__ bool slider() const { return (kind & UNIT_SLIDER) != 0; }
    __device__ bool lrow() const { return (kind & UNIT_ROW_L) != 0; }
    __device__ bool mrow() const { return (kind & UNIT_ROW_M) != 0; }
};

// who is written: a body with a mass or an inertia (not the world, not a static body)
__device__ __forceinline__ void pin_writes(PinRegs& r, int body2)
{
    r.write_a = !(r.ma == 0.f && r.ia == 0.f);
    r.write_b = body2 >= 0 && !(r.mb == 0.f && r.ib == 0.f);
}

// the rotated anchors and the inverse masses; -> the separation of the two anchor points pa = posA + ra and pb = posB + rb: a pin's or a
// link's is pb - pa, a slider's (FROM_B) pa - pb, which is not the other negated: the two differ in the sign of a zero.
// `P` is a phx_pin, a phx_link or a phx_slider.  w: where given, `axis` (a direction fixed in B) rotated with B.
// (The subtraction and the axis stay in here, beside the loads: handed out as pa and pb and subtracted by the caller, or with B's frame
// loaded again for the axis, the same arithmetic costs k_solve_pins 4 to 14 instructions more: DESIGN.md, the pin pass's tidy-up.)
template <bool FROM_B = false, class P>
__device__ __forceinline__ void pin_anchors(const P& p, const float4* __restrict__ mpos, const float4* __restrict__ frame, PinRegs& r, float& cx, float& cy,
                                            phx_vec2 axis = phx_vec2{0.f, 0.f}, phx_vec2* w = nullptr)
{
    const float4 qa = mpos[p.body1], fa = frame[p.body1];
    r.ma = qa.x; r.ia = qa.y;
    r.rax = fa.x * p.anchor1.x + fa.z * p.anchor1.y;
    r.ray = fa.y * p.anchor1.x + fa.w * p.anchor1.y;
    const float pax = qa.z + r.rax, pay = qa.w + r.ray;
    float pbx, pby;
    if (p.body2 >= 0) {
        const float4 qb = mpos[p.body2], fb = frame[p.body2];
        r.mb = qb.x; r.ib = qb.y;
        r.rbx = fb.x * p.anchor2.x + fb.z * p.anchor2.y;
        r.rby = fb.y * p.anchor2.x + fb.w * p.anchor2.y;
        pbx = qb.z + r.rbx; pby = qb.w + r.rby;
        if (w) { w->x = fb.x * axis.x + fb.z * axis.y; w->y = fb.y * axis.x + fb.w * axis.y; }
    } else {
        r.mb = 0.f; r.ib = 0.f; r.rbx = 0.f; r.rby = 0.f;
        pbx = p.anchor2.x; pby = p.anchor2.y;
        if (w) *w = axis;
    }
    if (FROM_B) { cx = pax - pbx; cy = pay - pby; } else { cx = pbx - pax; cy = pby - pay; }
}

__device__ __forceinline__ PinRegs pin_prestep(const phx_pin& p, const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta)
{
    PinRegs r;
    float cx, cy;
    pin_anchors(p, mpos, frame, r, cx, cy);
    pin_writes(r, p.body2);
    r.kind = UNIT_PIN; r.clamps = false;
    const float ms = r.ma + r.mb;
    r.k11 = (ms + (r.ia * r.ray) * r.ray) + (r.ib * r.rby) * r.rby;
    r.k12 = -((r.ia * r.rax) * r.ray) - (r.ib * r.rbx) * r.rby;
    r.k22 = (ms + (r.ia * r.rax) * r.rax) + (r.ib * r.rbx) * r.rbx;
    const float det = r.k11 * r.k22 - r.k12 * r.k12;
    r.active = det > 0x1p-20f * (r.k11 * r.k22);              // above the rounding noise of the det expression (pin_spec.py DET_FLOOR)
    r.inv_det = 1.0f / det;
    r.biasx = cx * beta; r.biasy = cy * beta;
    r.px = r.active ? p.impulse.x : 0.f;
    r.py = r.active ? p.impulse.y : 0.f;
    return r;
}

// the clamp, written as comparisons so that a NaN passes through
__device__ __forceinline__ float link_clamp(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }

// Row L's engagement at position x between the bounds lo and hi: a row that does not clamp (`clamps` clear: a rod, a lock, a spring)
// holds x at `rest`; one that clamps pushes one way only, at the bound x has reached, or is idle this step between the two.
// Leaves clamps and the impulse's bounds in r and the position error in c, and clears `on` where the row is idle (a flag to clear,
// not a result: so the idle arm stays a select beside the others, as it was in each of the three copies).
__device__ __forceinline__ void limit_row(PinRegs& r, bool clamps, float x, float lo, float hi, float rest, float& c, bool& on)
{
    const float inf = __builtin_inff();
    r.clamps = clamps;
    r.lo = -inf; r.hi = inf;
    if (!r.clamps) c = x - rest;
    else if (x >= hi) { c = x - hi; r.hi = 0.f; }
    else if (x <= lo) { c = x - lo; r.lo = 0.f; }
    else { c = 0.f; on = false; }
}

// Row L's softness for the position error c: a spring (hertz > 0) gets gamma and its bias and kinv += gamma, a hard row the bias c beta
__device__ __forceinline__ void soft_row(PinRegs& r, float& kinv, float c, float hertz, float damping_ratio, float beta, float dt)
{
    if (hertz > 0.f) {
        const float mass = 1.0f / kinv;
        const float omega = 6.2831855f * hertz;
        const float dmp = ((2.0f * mass) * damping_ratio) * omega;
        const float k = (mass * omega) * omega;
        r.gamma = 1.0f / (dt * (dmp + dt * k));
        r.bias = ((c * dt) * k) * r.gamma;
        kinv = kinv + r.gamma;
    } else {
        r.gamma = 0.f;
        r.bias = c * beta;
    }
}

// row L's accumulation: lambda += d, clamped to [lo, hi] where the row clamps; -> the impulse actually applied
__device__ __forceinline__ float row_accumulate(PinRegs& r, float d)
{
    if (r.clamps) {
        const float next = link_clamp(r.lambda + d, r.lo, r.hi);
        d = next - r.lambda;
        r.lambda = next;
    } else r.lambda = r.lambda + d;
    return d;
}

// row M's accumulation at the relative speed cdot: towards `speed`, the accumulated impulse within [-mmax, mmax]; -> the impulse applied
__device__ __forceinline__ float motor_accumulate(float& mlambda, float inv_k, float cdot, float speed, float mmax)
{
    const float next = link_clamp(mlambda + -(inv_k * (cdot - speed)), -mmax, mmax);
    const float d = next - mlambda;
    mlambda = next;
    return d;
}

// tests/link_spec.py prestep, operation for operation
__device__ __forceinline__ PinRegs link_prestep(const phx_link& p, const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta, float dt)
{
    PinRegs r;
    float dx, dy;
    pin_anchors(p, mpos, frame, r, dx, dy);
    pin_writes(r, p.body2);
    r.kind = UNIT_LINK;
    const float len = sqrtf(dx * dx + dy * dy);                 // (sqrtf: correctly rounded under the library's flags)
    r.nx = dx / len; r.ny = dy / len;
    const float cra = r.rax * r.ny - r.ray * r.nx, crb = r.rbx * r.ny - r.rby * r.nx;
    float kinv = ((r.ma + r.mb) + (r.ia * cra) * cra) + (r.ib * crb) * crb;
    r.active = len > 0x1p-10f && kinv > 0.f;
    float c;
    limit_row(r, p.min_length < p.max_length, len, p.min_length, p.max_length, p.min_length, c, r.active);
    soft_row(r, kinv, c, p.hertz, p.damping_ratio, beta, dt);
    r.inv_k = 1.0f / kinv;
    r.lambda = r.active ? link_clamp(p.impulse, r.lo, r.hi) : 0.f;
    return r;
}

// tests/angle_spec.py prestep, operation for operation.  theta: the double-precision atan2 rounded to float, k_integrate_position's rule
// for cos / sin; here only, never in a sweep.
__device__ __forceinline__ PinRegs angle_prestep(const phx_angle& p, const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta, float dt)
{
    PinRegs r;
    const float4 qa = mpos[p.body1], fa = frame[p.body1];
    r.ma = qa.x; r.ia = qa.y;
    float xbx = 1.f, xby = 0.f;
    r.mb = 0.f; r.ib = 0.f;
    if (p.body2 >= 0) {
        const float4 qb = mpos[p.body2], fb = frame[p.body2];
        r.mb = qb.x; r.ib = qb.y;
        xbx = fb.x; xby = fb.y;
    }
    pin_writes(r, p.body2);
    r.nx = 0.f; r.ny = 0.f;                                     // (no axis: the trailing group's work record carries every word)
    const float c = fa.x * xbx + fa.y * xby, s = fa.x * xby - fa.y * xbx;
    const float theta = (float)atan2((double)(-s), (double)c);
    const float mid = (p.lower + p.upper) * 0.5f, half = (p.upper - p.lower) * 0.5f;
    float phi = theta - mid;
    if (phi > 3.1415927f) phi = phi - 6.2831855f;
    else if (phi < -3.1415927f) phi = phi + 6.2831855f;
    float kinv = r.ia + r.ib;
    const bool solvable = kinv > 0.f;
    float cl;
    bool lrow = true;
    limit_row(r, p.lower < p.upper, phi, -half, half, 0.f, cl, lrow);      // (phi is measured from the middle of the limits already)
    r.inv_k = 1.0f / kinv;
    soft_row(r, kinv, cl, p.hertz, p.damping_ratio, beta, dt);
    r.inv_kg() = 1.0f / kinv;
    r.speed() = p.motor_speed;
    r.mmax() = p.max_torque * dt;
    const bool mrow = solvable && p.max_torque > 0.f;
    lrow = solvable && lrow;
    r.kind = UNIT_ANGLE | (lrow ? UNIT_ROW_L : 0) | (mrow ? UNIT_ROW_M : 0);
    r.active = lrow || mrow;
    r.mlambda() = mrow ? link_clamp(p.motor_impulse, -r.mmax(), r.mmax()) : 0.f;
    r.lambda = lrow ? link_clamp(p.impulse, r.lo, r.hi) : 0.f;
    return r;
}

// an angle's apply: the two angular velocities only
__device__ __forceinline__ void angle_apply(const PinRegs& r, float d, float4& va, float4& vb)
{
    va.z = va.z - r.ia * d;
    vb.z = vb.z + r.ib * d;
}

// an angle's warm start: M's accumulated impulse, then L's, each where its row is on
__device__ __forceinline__ void angle_warm(const PinRegs& r, float4& va, float4& vb)
{
    if (r.mrow()) angle_apply(r, r.mlambda(), va, vb);
    if (r.lrow()) angle_apply(r, r.lambda, va, vb);
}

// one sweep of an angle: M, then L on the velocities M left; accumulates both
__device__ __forceinline__ void angle_sweep(PinRegs& r, float4& va, float4& vb)
{
    if (r.mrow()) angle_apply(r, motor_accumulate(r.mlambda(), r.inv_k, vb.z - va.z, r.speed(), r.mmax()), va, vb);
    if (r.lrow()) {
        const float cdot = vb.z - va.z;
        angle_apply(r, row_accumulate(r, -(r.inv_kg() * ((cdot + r.bias) + r.gamma * r.lambda))), va, vb);
    }
}

// what a slider's lane keeps beside PinRegs (which holds, under a link's names: ra, rb' in rbx / rby, n, gamma, inv_k = 1 / kinv_n, row L's
// bias, lo, hi and lambda): row P's 1 / kinv_t, bias and impulse, row L's 1 / (kinv_n + gamma), row M's speed, largest and accumulated impulse
struct RailRegs { float inv_kt, inv_kng, bias_t, speed, mmax, mlambda, plambda; };
struct NoRail {};                       // (the instantiations without sliders)

// tests/slider_spec.py prestep, operation for operation
__device__ __forceinline__ PinRegs slider_prestep(const phx_slider& p, const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta, float dt, RailRegs& x)
{
    PinRegs r;
    float ex, ey;                                               // e = pa - pb: from B's anchor point to the carriage's
    phx_vec2 w;                                                 // the rail: B's axis, rotated with B
    pin_anchors<true>(p, mpos, frame, r, ex, ey, p.axis, &w);
    const float wx = w.x, wy = w.y;
    pin_writes(r, p.body2);
    const float len = sqrtf(wx * wx + wy * wy);                 // (sqrtf: correctly rounded under the library's flags)
    r.nx = wx / len; r.ny = wy / len;
    r.rbx = r.rbx + ex; r.rby = r.rby + ey;                     // rb' = rb + e: B's arm to the carriage's anchor point
    const float s = r.nx * ex + r.ny * ey, ct = r.nx * ey - r.ny * ex;
    const float cat = r.rax * r.nx + r.ray * r.ny, cbt = r.rbx * r.nx + r.rby * r.ny;
    const float can = r.rax * r.ny - r.ray * r.nx, cbn = r.rbx * r.ny - r.rby * r.nx;
    const float ms = r.ma + r.mb;
    const float kinv_t = (ms + (r.ia * cat) * cat) + (r.ib * cbt) * cbt;
    float kinv = (ms + (r.ia * can) * can) + (r.ib * cbn) * cbn;
    r.active = kinv_t > 0.f;
    const bool solvable = r.active && kinv > 0.f;
    x.inv_kt = 1.0f / kinv_t;
    x.bias_t = ct * beta;
    float c;
    bool lrow = true;
    limit_row(r, p.lower < p.upper, s, p.lower, p.upper, p.lower, c, lrow);
    r.inv_k = 1.0f / kinv;
    soft_row(r, kinv, c, p.hertz, p.damping_ratio, beta, dt);
    x.inv_kng = 1.0f / kinv;
    x.speed = p.motor_speed;
    x.mmax = p.max_force * dt;
    const bool mrow = solvable && p.max_force > 0.f;
    lrow = solvable && lrow;
    r.kind = UNIT_SLIDER | (lrow ? UNIT_ROW_L : 0) | (mrow ? UNIT_ROW_M : 0);
    x.mlambda = mrow ? link_clamp(p.motor_impulse, -x.mmax, x.mmax) : 0.f;
    r.lambda = lrow ? link_clamp(p.axis_impulse, r.lo, r.hi) : 0.f;
    x.plambda = r.active ? p.impulse : 0.f;
    return r;
}

// a slider's apply, P at the carriage's anchor point: vA += mA P, wA -= iA (ra x P), vB -= mB P, wB += iB (rb' x P)
__device__ __forceinline__ void slider_apply(const PinRegs& r, float px, float py, float4& va, float4& vb)
{
    va.x = va.x + r.ma * px;
    va.y = va.y + r.ma * py;
    va.z = va.z - r.ia * (r.rax * py - r.ray * px);
    vb.x = vb.x - r.mb * px;
    vb.y = vb.y - r.mb * py;
    vb.z = vb.z + r.ib * (r.rbx * py - r.rby * px);
}

// (vA + wA x ra) - (vB + wB x rb')
__device__ __forceinline__ void slider_rel(const PinRegs& r, const float4& va, const float4& vb, float& rx, float& ry)
{
    const float uax = va.x + va.z * r.ray, uay = va.y - va.z * r.rax;
    const float ubx = vb.x + vb.z * r.rby, uby = vb.y - vb.z * r.rbx;
    rx = uax - ubx; ry = uay - uby;
}

// a slider's warm start: M's accumulated impulse, then L's, then P's
__device__ __forceinline__ void slider_warm(const PinRegs& r, const RailRegs& x, float4& va, float4& vb)
{
    if (r.mrow()) slider_apply(r, x.mlambda * r.nx, x.mlambda * r.ny, va, vb);
    if (r.lrow()) slider_apply(r, r.lambda * r.nx, r.lambda * r.ny, va, vb);
    slider_apply(r, x.plambda * -r.ny, x.plambda * r.nx, va, vb);
}

// one sweep of a slider: M, then L, then P, each on the velocities the row before left; accumulates the three
__device__ __forceinline__ void slider_sweep(PinRegs& r, RailRegs& x, float4& va, float4& vb)
{
    float rx, ry;
    if (r.mrow()) {
        slider_rel(r, va, vb, rx, ry);
        const float d = motor_accumulate(x.mlambda, r.inv_k, r.nx * rx + r.ny * ry, x.speed, x.mmax);
        slider_apply(r, d * r.nx, d * r.ny, va, vb);
    }
    if (r.lrow()) {
        slider_rel(r, va, vb, rx, ry);
        const float cdot = r.nx * rx + r.ny * ry;
        const float d = row_accumulate(r, -(x.inv_kng * ((cdot + r.bias) + r.gamma * r.lambda)));
        slider_apply(r, d * r.nx, d * r.ny, va, vb);
    }
    slider_rel(r, va, vb, rx, ry);
    const float cdot = r.nx * ry - r.ny * rx;
    const float d = -(x.inv_kt * (cdot + x.bias_t));
    x.plambda = x.plambda + d;
    slider_apply(r, d * -r.ny, d * r.nx, va, vb);
}
// (the instantiations without sliders have no RailRegs and never get here)
__device__ __forceinline__ PinRegs slider_prestep(const phx_slider&, const float4*, const float4*, float, float, NoRail&) { return PinRegs{}; }
__device__ __forceinline__ void slider_warm(const PinRegs&, const NoRail&, float4&, float4&) {}
__device__ __forceinline__ void slider_sweep(PinRegs&, NoRail&, float4&, float4&) {}

// The engine's angularVelocity is CLOCKWISE-positive: IntegratePosition rotates the frame by -w dt (ref: World.cpp:63) and the contact
// limiters project it with n x r (ref: Solver.cpp:559-560), so the velocity of a body's point at r is v - w x r = (v.x + w r.y, v.y - w r.x)
// and an impulse P at r changes w by -i (r x P).
// apply P to the two velocities {v.x, v.y, w, .}
__device__ __forceinline__ void pin_apply(const PinRegs& r, float px, float py, float4& va, float4& vb)
{
    va.x = va.x - r.ma * px;
    va.y = va.y - r.ma * py;
    va.z = va.z + r.ia * (r.rax * py - r.ray * px);
    vb.x = vb.x + r.mb * px;
    vb.y = vb.y + r.mb * py;
    vb.z = vb.z - r.ib * (r.rbx * py - r.rby * px);
}

// one sweep's impulse of the pin on velocities va, vb; accumulates it
__device__ __forceinline__ void pin_delta(PinRegs& r, const float4& va, const float4& vb, float& dx, float& dy)
{
    const float vbx = vb.x + vb.z * r.rby, vby = vb.y - vb.z * r.rbx;
    const float vax = va.x + va.z * r.ray, vay = va.y - va.z * r.rax;
    const float rx = -((vbx - vax) + r.biasx), ry = -((vby - vay) + r.biasy);
    dx = r.inv_det * (r.k22 * rx - r.k12 * ry);
    dy = r.inv_det * (r.k11 * ry - r.k12 * rx);
    r.px = r.px + dx;
    r.py = r.py + dy;
}

// one sweep's impulse of the link, as a vector along its axis; accumulates lambda
__device__ __forceinline__ void link_delta(PinRegs& r, const float4& va, const float4& vb, float& dx, float& dy)
{
    const float vbx = vb.x + vb.z * r.rby, vby = vb.y - vb.z * r.rbx;
    const float vax = va.x + va.z * r.ray, vay = va.y - va.z * r.rax;
    const float cdot = r.nx * (vbx - vax) + r.ny * (vby - vay);
    const float d = row_accumulate(r, -(r.inv_k * ((cdot + r.bias) + r.gamma * r.lambda)));
    dx = d * r.nx; dy = d * r.ny;
}

// The later kinds' kernel arguments: a pack that is empty in a world without angles, so that the instantiations without them keep the
// signature, the kernarg layout and the code they had before there were angles; with angles it is (phx_angle* angles, int nlinks).
// The sliders' ride behind them the same way: (phx_slider* sliders, int nangles) and, in the trailing group's kernels, (RailWork* rail).
// What a level lacks is a constant: the ladder's guards (kernels below) drop its arm at compile time.
struct RailWork;
struct NoAngles { static constexpr phx_angle* angles = nullptr; static constexpr int nlinks = 0; static constexpr phx_slider* sliders = nullptr; static constexpr int nangles = 0; static constexpr RailWork* rail = nullptr; };
struct AngleArgs { phx_angle* angles; int nlinks; static constexpr phx_slider* sliders = nullptr; static constexpr int nangles = 0; static constexpr RailWork* rail = nullptr; };
struct SliderArgs { phx_angle* angles; int nlinks; phx_slider* sliders; int nangles; RailWork* rail; };
__device__ __forceinline__ NoAngles angle_args() { return NoAngles{}; }
__device__ __forceinline__ AngleArgs angle_args(phx_angle* angles, int nlinks) { return AngleArgs{angles, nlinks}; }
__device__ __forceinline__ SliderArgs angle_args(phx_angle* angles, int nlinks, phx_slider* sliders, int nangles, RailWork* rail = nullptr) { return SliderArgs{angles, nlinks, sliders, nangles, rail}; }

// The world's level, from the kernels' template arguments <bool LINKS, class... A>: which kinds the units may be.  LINKS: the world has
// links; without them every kernel below is the pins' alone, instruction for instruction what it was before there were links (a lane's
// branch on the kind costs the pass 4 us of 30 on the world of DESIGN.md 5b, all pins: the launch is a chain of class steps, and each
// one pays for it).
template <bool LINKS, class... A> struct PinLevel {
    static constexpr bool links = LINKS, angles = sizeof...(A) > 0, sliders = sizeof...(A) > 2;
    using Rail = std::conditional_t<sliders, RailRegs, NoRail>;
};

// One class step of a unit on its two velocities: the warm start (sweep clear: the unit's accumulated impulses) or one sweep
template <class L>
__device__ __forceinline__ void unit_step(PinRegs& r, typename L::Rail& x, float4& va, float4& vb, bool sweep)
{
    if (L::sliders && r.slider()) { if (sweep) slider_sweep(r, x, va, vb); else slider_warm(r, x, va, vb); }
    else if (L::angles && r.angle()) { if (sweep) angle_sweep(r, va, vb); else angle_warm(r, va, vb); }
    else {
        float dx, dy;
        if (L::links && r.kind == UNIT_LINK) { if (sweep) link_delta(r, va, vb, dx, dy); else { dx = r.lambda * r.nx; dy = r.lambda * r.ny; } }
        else if (sweep) pin_delta(r, va, vb, dx, dy);
        else { dx = r.px; dy = r.py; }
        pin_apply(r, dx, dy, va, vb);
    }
}

// ... of the lane's unit on its two bodies in the LDS table (`zero`: the world's velocity)
template <class L>
__device__ __forceinline__ void lds_step(PinRegs& r, typename L::Rail& x, const PinSlot& s, float4* sv, const float4& zero, bool sweep)
{
    float4 va = sv[s.a], vb = s.b >= 0 ? sv[s.b] : zero;
    unit_step<L>(r, x, va, vb, sweep);
    if (r.write_a) sv[s.a] = va;
    if (r.write_b) sv[s.b] = vb;
}

// Unit u's accumulated impulses to its record (`pin` clear: a pin's stays as it is)
template <class L, class Args>
__device__ __forceinline__ void unit_store(phx_pin* __restrict__ pins, phx_link* __restrict__ links, int npins, const Args& ang, int u, const PinRegs& r,
                                           const typename L::Rail& x, bool pin = true)
{
    const int npl = npins + ang.nlinks, npla = npl + ang.nangles;
    if constexpr (L::sliders)
        if (r.slider()) { phx_slider& a = ang.sliders[u - npla]; a.impulse = x.plambda; a.axis_impulse = r.lambda; a.motor_impulse = x.mlambda; return; }
    if constexpr (L::angles)
        if (r.angle()) { phx_angle& a = ang.angles[u - npl]; a.impulse = r.lambda; a.motor_impulse = r.mlambda(); return; }
    if (L::links && r.kind == UNIT_LINK) links[u - npins].impulse = r.lambda;
    else if (pin) pins[u].impulse = phx_vec2{r.px, r.py};
}

// The LDS layout: one float4 per local body.  A lane's two bodies are anywhere in the table, so a class step is a gather / scatter of
// 16-byte granules (ds_read_b128 / ds_write_b128).  A 16-byte read is served in four groups of 16 lanes over the 64 banks: a group
// is conflict-free when its granules differ mod 16.  The two classes of a chain take every other pin, so a class's lanes sit two
// granules apart and read two-way conflicted (8 LDS cycles instead of 4 per wave); the 16-byte store's cost is its register transfer
// either way.  Both are small beside the dependent chain of a class step (read, ~20 dependent flops, write, barrier), which is what
// the pass waits for.
template <bool LINKS, class... A>
static __global__ void __launch_bounds__(PIN_LANES) k_solve_pins(phx_pin* __restrict__ pins, phx_link* __restrict__ links, int npins, const PinSlot* __restrict__ slots,
                                                                 const PinGroup* __restrict__ groups, const int* __restrict__ group_bodies, float4* __restrict__ vel,
                                                                 const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta, float dt, int iterations, A... angle_pack)
{
    using L = PinLevel<LINKS, A...>;
    const auto ang = angle_args(angle_pack...);
    __shared__ float4 sv[PIN_BODIES];
    const PinGroup g = groups[blockIdx.x];
    const int* const bodies = group_bodies + g.body_begin;
    for (int i = threadIdx.x; i < g.body_count; i += PIN_LANES) {
        const int b = bodies[i];
        sv[i] = b >= 0 ? vel[b] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    const int slot = g.slot_begin + (int)threadIdx.x;
    const bool mine = slot < g.slot_end;
    PinSlot s = {0, 0, -1, -1};
    PinRegs r = {};
    [[maybe_unused]] typename L::Rail x = {};
    if (mine) {
        s = slots[slot];
        const int npl = npins + ang.nlinks, npla = npl + ang.nangles;
        r = (!L::links || s.pin < npins) ? pin_prestep(pins[s.pin], mpos, frame, beta)
            : (!L::angles || s.pin < npl) ? link_prestep(links[s.pin - npins], mpos, frame, beta, dt)
            : (!L::sliders || s.pin < npla) ? angle_prestep(ang.angles[s.pin - npl], mpos, frame, beta, dt)
            : slider_prestep(ang.sliders[s.pin - npla], mpos, frame, beta, dt, x);
    }
    const bool work = mine && r.active;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    __syncthreads();
    for (int c = 0; c < g.classes; ++c) {                                   // warm start, class by class
        if (work && s.colour == c) lds_step<L>(r, x, s, sv, zero, false);
        __syncthreads();
    }
    for (int it = 0; it < iterations; ++it)
        for (int c = 0; c < g.classes; ++c) {
            if (work && s.colour == c) lds_step<L>(r, x, s, sv, zero, true);
            __syncthreads();
        }
    for (int i = g.first_dynamic + (int)threadIdx.x; i < g.body_count; i += PIN_LANES) vel[bodies[i]] = sv[i];
    if (mine) unit_store<L>(pins, links, npins, ang, s.pin, r, x);
}

// ---- the trailing group, out of HBM ----
// what the prestep leaves of a unit (k11 .. biasy hold a link's nx, ny, gamma, inv_k, bias, lo: PinRegs' unions; flags: PinRegs' kind and
// bools, the enum above; the accumulated impulses stay in the unit's record)
struct PinWork { float rax, ray, rbx, rby, k11, k12, k22, inv_det, biasx, biasy, ma, ia, mb, ib; int flags; float hi; };
// a slider's words beyond PinWork (which holds what a link's does, rb' in rbx / rby): a side array beside the work array, slot for slot,
// which exists only in a world with sliders
struct RailWork { float inv_kt, inv_kng, bias_t, speed, mmax, pad0, pad1, pad2; };
static_assert(sizeof(PinWork) == 64 && sizeof(RailWork) == 32, "the trailing group's records");

// a lane's state into the trailing group's record `slot`
template <class L>
__device__ __forceinline__ void work_pack(const PinRegs& r, const typename L::Rail& x, PinWork* __restrict__ work, RailWork* __restrict__ rail, int slot)
{
    PinWork w;
    w.rax = r.rax; w.ray = r.ray; w.rbx = r.rbx; w.rby = r.rby; w.k11 = r.k11; w.k12 = r.k12; w.k22 = r.k22; w.inv_det = r.inv_det;
    w.biasx = r.biasx; w.biasy = r.biasy; w.ma = r.ma; w.ia = r.ia; w.mb = r.mb; w.ib = r.ib;
    w.flags = r.kind | (r.active ? UNIT_ACTIVE : 0) | (r.write_a ? UNIT_WRITE_A : 0) | (r.write_b ? UNIT_WRITE_B : 0) | (r.clamps ? UNIT_CLAMPS : 0);
    w.hi = r.kind != UNIT_PIN ? r.hi : 0.f;                                // (a pin's second impulse word stays in its record)
    work[slot] = w;
    if constexpr (L::sliders)
        if (r.slider()) rail[slot] = RailWork{x.inv_kt, x.inv_kng, x.bias_t, x.speed, x.mmax, 0.f, 0.f, 0.f};
}

// ... and out of it again, with unit u's accumulated impulses from its record
template <class L, class Args>
__device__ __forceinline__ PinRegs work_unpack(const PinWork& w, const phx_pin* __restrict__ pins, const phx_link* __restrict__ links, int npins, const Args& ang, int u, int slot,
                                               typename L::Rail& x)
{
    PinRegs r;
    r.rax = w.rax; r.ray = w.ray; r.rbx = w.rbx; r.rby = w.rby; r.k11 = w.k11; r.k12 = w.k12; r.k22 = w.k22; r.inv_det = w.inv_det;
    r.biasx = w.biasx; r.biasy = w.biasy; r.ma = w.ma; r.ia = w.ia; r.mb = w.mb; r.ib = w.ib;
    r.kind = (unsigned char)(w.flags & UNIT_KIND);
    r.active = (w.flags & UNIT_ACTIVE) != 0; r.write_a = (w.flags & UNIT_WRITE_A) != 0; r.write_b = (w.flags & UNIT_WRITE_B) != 0; r.clamps = (w.flags & UNIT_CLAMPS) != 0;
    r.hi = w.hi;
    const int npl = npins + ang.nlinks, npla = npl + ang.nangles;
    if (L::sliders && r.slider()) {
        if constexpr (L::sliders) {
            const phx_slider& a = ang.sliders[u - npla];
            const RailWork k = ang.rail[slot];
            r.lambda = a.axis_impulse;
            x.inv_kt = k.inv_kt; x.inv_kng = k.inv_kng; x.bias_t = k.bias_t; x.speed = k.speed; x.mmax = k.mmax;
            x.mlambda = a.motor_impulse; x.plambda = a.impulse;
        }
    } else if (L::angles && r.angle()) { const phx_angle& a = ang.angles[u - npl]; r.lambda = a.impulse; r.mlambda() = a.motor_impulse; }
    else if (L::links && r.kind == UNIT_LINK) r.lambda = links[u - npins].impulse;
    else { const phx_vec2 p = pins[u].impulse; r.px = p.x; r.py = p.y; }
    return r;
}

// slots [begin, end): the prestep; an inactive pin's impulse becomes 0 here, a link's its warm start (clamped; 0 when inactive or idle),
// an angle's two and a slider's three likewise
template <bool LINKS, class... A>
static __global__ void __launch_bounds__(256) k_pin_prestep(phx_pin* __restrict__ pins, phx_link* __restrict__ links, int npins, const PinSlot* __restrict__ slots, int begin, int end,
                                                            const float4* __restrict__ mpos, const float4* __restrict__ frame, float beta, float dt, PinWork* __restrict__ work, A... angle_pack)
{
    using L = PinLevel<LINKS, A...>;
    const auto ang = angle_args(angle_pack...);
    for (int k = begin + blockIdx.x * blockDim.x + threadIdx.x; k < end; k += gridDim.x * blockDim.x) {
        const int pin = slots[k].pin;
        const int npl = npins + ang.nlinks, npla = npl + ang.nangles;
        [[maybe_unused]] typename L::Rail x;
        const PinRegs r = (!L::links || pin < npins) ? pin_prestep(pins[pin], mpos, frame, beta)
                          : (!L::angles || pin < npl) ? link_prestep(links[pin - npins], mpos, frame, beta, dt)
                          : (!L::sliders || pin < npla) ? angle_prestep(ang.angles[pin - npl], mpos, frame, beta, dt)
                          : slider_prestep(ang.sliders[pin - npla], mpos, frame, beta, dt, x);
        work_pack<L>(r, x, work, ang.rail, k - begin);
        unit_store<L>(pins, links, npins, ang, pin, r, x, !r.active);
    }
}

// one class, slots [begin, end) of a group whose work array starts at slot `base`: the warm start (sweep == 0) or one sweep
template <bool LINKS, class... A>
static __global__ void __launch_bounds__(256) k_pin_class(phx_pin* __restrict__ pins, phx_link* __restrict__ links, int npins, const PinSlot* __restrict__ slots, int begin, int end,
                                                          int base, const PinWork* __restrict__ work, float4* __restrict__ vel, int sweep, A... angle_pack)
{
    using L = PinLevel<LINKS, A...>;
    const auto ang = angle_args(angle_pack...);
    for (int k = begin + blockIdx.x * blockDim.x + threadIdx.x; k < end; k += gridDim.x * blockDim.x) {
        const PinSlot s = slots[k];
        const PinWork w = work[k - base];
        if (!(w.flags & UNIT_ACTIVE)) continue;
        [[maybe_unused]] typename L::Rail x;
        PinRegs r = work_unpack<L>(w, pins, links, npins, ang, s.pin, k - base, x);
        float4 va = vel[s.a], vb = s.b >= 0 ? vel[s.b] : make_float4(0.f, 0.f, 0.f, 0.f);
        unit_step<L>(r, x, va, vb, sweep != 0);
        if (r.write_a) vel[s.a] = va;
        if (r.write_b) vel[s.b] = vb;
        if (sweep) unit_store<L>(pins, links, npins, ang, s.pin, r, x);
    }
}

// ---- what the host asks between steps ----
// (`P`: phx_pin, phx_link, phx_angle or phx_slider, which begin alike: body1, body2; only those are read)
// per pin: are its bodies static (bit 0: body1, bit 1: body2)?  O(pins) bytes for the schedule build
template <class P>
static __global__ void __launch_bounds__(256) k_pin_statics(const P* __restrict__ pins, int n, const float4* __restrict__ mpos, unsigned* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const P& p = pins[i];
        const float4 a = mpos[p.body1];
        unsigned bits = (a.x == 0.f && a.y == 0.f) ? 1u : 0u;
        if (p.body2 >= 0) { const float4 b = mpos[p.body2]; if (b.x == 0.f && b.y == 0.f) bits |= 2u; }
        out[i] = bits;
    }
}

// a removal of bodies: every pin's bodies through new[] (-1: removed; the world stays -1 and is told apart by the old index)
template <class P>
static __global__ void __launch_bounds__(256) k_pin_remap(const P* __restrict__ pins, int n, const int* __restrict__ remap, int2* __restrict__ out)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const P& p = pins[i];
        out[i] = make_int2(remap[p.body1], p.body2 >= 0 ? remap[p.body2] : -2);
    }
}

// an edit of fields (pins.h AnchorFields, LengthFields: phx_world_set_pin_anchors / set_link_anchors / set_link_lengths) on the device copy
template <class P, class Fields>
static __global__ void __launch_bounds__(256) k_unit_fields(const int* __restrict__ which, const float* __restrict__ values, int count, P* __restrict__ units)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) Fields::write(units[which[k]], values + Fields::width * k);
}

// ---- breaks (include/phyx_amd.h BREAKS; the definition: tests/break_spec.py) ----
// an edit of break limits (phx_world_set_break_limits) on the device copy of a list's limit column
static __global__ void __launch_bounds__(256) k_unit_limits(const int* __restrict__ which, const float* __restrict__ values, int count, float* __restrict__ limits)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) limits[which[k]] = values[k];
}

// The lists that have a limit column, kind behind kind: limited unit i is a pin while i < end[0], else a link while i < end[1], and so
// on (a list without a column counts no unit: its end is the end before it), so i ascending is (kind, index) ascending.
struct BreakLists {
    const phx_pin* pins; const phx_link* links; const phx_angle* angles; const phx_slider* sliders;
    const float* pin_limits, *link_limits, *angle_limits, *slider_limits;
    int end[4];
};

constexpr int BREAK_LANES = 1024;       // block_exclusive_scan_1024's workgroup
constexpr int BREAK_BLOCKS = 1024;      // at most: the last workgroup scans the workgroups' counts in one block scan
// the words beside the events: a count per workgroup (zero between launches), the ticket the workgroups draw as they finish (64 bits,
// 8-byte aligned: the tickets drawn so far, and above them the events published so far), the step's event count
enum : int { BREAK_TICKET = BREAK_BLOCKS, BREAK_COUNT = BREAK_BLOCKS + 2, BREAK_WORDS = BREAK_BLOCKS + 4 };

// limited unit i after the pass: the reaction impulse R of the impulses in its record against L dt, break_spec.py operation for operation
__device__ __forceinline__ bool unit_breaks(const BreakLists& l, int i, float dt, phx_break_event& e)
{
    float r, limit;
    if (i < l.end[0]) {
        const phx_pin& p = l.pins[i];
        e.kind = PHX_UNIT_PIN; e.index = i; e.body1 = p.body1; e.body2 = p.body2;
        r = sqrtf(p.impulse.x * p.impulse.x + p.impulse.y * p.impulse.y);
        limit = l.pin_limits[i];
    } else if (i < l.end[1]) {
        const int k = i - l.end[0];
        const phx_link& p = l.links[k];
        e.kind = PHX_UNIT_LINK; e.index = k; e.body1 = p.body1; e.body2 = p.body2;
        r = fabsf(p.impulse);
        limit = l.link_limits[k];
    } else if (i < l.end[2]) {
        const int k = i - l.end[1];
        const phx_angle& p = l.angles[k];
        e.kind = PHX_UNIT_ANGLE; e.index = k; e.body1 = p.body1; e.body2 = p.body2;
        r = fabsf(p.impulse + p.motor_impulse);
        limit = l.angle_limits[k];
    } else {
        const int k = i - l.end[2];
        const phx_slider& p = l.sliders[k];
        e.kind = PHX_UNIT_SLIDER; e.index = k; e.body1 = p.body1; e.body2 = p.body2;
        const float a = p.axis_impulse + p.motor_impulse;
        r = sqrtf(p.impulse * p.impulse + a * a);
        limit = l.slider_limits[k];
    }
    e.step = 0;                                                             // (the host knows the step: PinSet::settle)
    e.reaction = r;
    e.threshold = limit * dt;
    e.reserved = 0;
    return r > e.threshold;                                                 // (strict, and false for a NaN)
}

// The break test behind the pass: the step's events, dense and in (kind, index) order, and their count.  An ordered compaction in one
// launch: workgroup b walks limited units [b chunk, (b + 1) chunk) tile by tile and writes its events, in order (a block scan of the
// tile's flags), to the front of its own stretch of `staged`; every workgroup then draws a ticket, one 64-bit atomic that also adds
// its count to the events published so far (the atomic orders nothing in the output), and the workgroup that draws the last one
// knows the step's total: if there are events it scans the workgroups' counts and moves the stretches together into `events`.
// A step in which nothing breaks, the common one, takes no fence: a workgroup without events publishes nothing (its count word is
// zero from the last launch), and the last workgroup reads nothing of the others.  `staged` and `events` hold one record per
// limited unit, so neither can overflow.  chunk: a multiple of BREAK_LANES; gridDim.x <= BREAK_BLOCKS.
static __global__ void __launch_bounds__(BREAK_LANES) k_unit_breaks(BreakLists l, float dt, int chunk, phx_break_event* __restrict__ staged, unsigned* __restrict__ words,
                                                                    phx_break_event* __restrict__ events)
{
    __shared__ unsigned lds[16];
    __shared__ unsigned offsets[BREAK_BLOCKS];
    __shared__ unsigned long long drawn;
    unsigned long long* const ticket = reinterpret_cast<unsigned long long*>(words + BREAK_TICKET);
    const int n = l.end[3];
    const long long begin = (long long)blockIdx.x * chunk;
    unsigned mine = 0;
    for (int t = 0; t < chunk; t += BREAK_LANES) {
        const long long i = begin + t + threadIdx.x;
        phx_break_event e;
        const bool breaks = i < n && unit_breaks(l, (int)i, dt, e);
        if (!__syncthreads_count(breaks)) continue;                         // (the same for every lane)
        unsigned total;
        const unsigned at = block_exclusive_scan_1024(breaks ? 1u : 0u, lds, &total);
        if (breaks) staged[begin + mine + at] = e;
        mine += total;
        __syncthreads();                                                    // (the next tile's scan writes `lds` again)
    }
    if (mine) {                                                             // this workgroup's events and count are out before its ticket is drawn
        if (threadIdx.x == 0) words[blockIdx.x] = mine;
        __threadfence();
    }
    __syncthreads();
    if (threadIdx.x == 0) drawn = atomicAdd(ticket, ((unsigned long long)mine << 32) | 1ull);
    __syncthreads();
    const unsigned long long before = drawn;
    if ((unsigned)before != gridDim.x - 1) return;
    const unsigned total = (unsigned)(before >> 32) + mine;
    if (total) {
        __threadfence();                                                    // ... and the others' are read behind the last ticket
        unsigned sum;
        const unsigned mine_begin = block_exclusive_scan_1024(threadIdx.x < gridDim.x ? words[threadIdx.x] : 0u, lds, &sum);
        offsets[threadIdx.x] = mine_begin;
        if (threadIdx.x < gridDim.x) words[threadIdx.x] = 0;                // (the next launch finds the counts zero)
        __syncthreads();
        for (unsigned j = threadIdx.x; j < total; j += BREAK_LANES) {
            unsigned lo = 0, hi = gridDim.x;                                // the last workgroup whose stretch begins at or before event j holds it
            while (hi - lo > 1) { const unsigned mid = (lo + hi) / 2; if (offsets[mid] <= j) lo = mid; else hi = mid; }
            events[j] = staged[(long long)lo * chunk + (j - offsets[lo])];
        }
    }
    if (threadIdx.x == 0) { words[BREAK_COUNT] = total; *ticket = 0; }
}

} // namespace phx
