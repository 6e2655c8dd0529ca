// field_kernels.h — the kernels of the force fields (fields.h; include/phyx_amd.h FORCE FIELDS).  tests/field_spec.py is the definition:
// float32, every operation rounded on its own (the library is built with -ffp-contract=off), IEEE division and square root.  The
// statements below follow it operation for operation.
//
// One lane per body.  The list is read through UNIFORM loads: the record's address depends on the loop counter alone, so the
// compiler fetches it with scalar loads into SGPRs (the record is read as three 16-byte granules, which come out as wide
// s_load_dwordx8 / x4 / x2, not the chain of dependent dword loads that reading the members one by one gave), the
// branches on kind, shape and flags are scalar branches the whole wave takes together, and no VGPR, no LDS and no barrier is spent
// on the list (DESIGN.md "Force fields").
#pragma once

#include "fields.h"

namespace phx {

// a record as the three granules the kernel loads (the device copies are 16-byte aligned: fields.hip)
struct FieldRec { int kind, shape; unsigned mask, flags; float region[4]; float value[4]; };
__device__ __forceinline__ FieldRec load_field(const phx_field* __restrict__ fields, int k)
{
    const uint4* g = reinterpret_cast<const uint4*>(fields + k);
    const uint4 a = g[0], b = g[1], c = g[2];
    return FieldRec{(int)a.x, (int)a.y, a.z, a.w, {__uint_as_float(b.x), __uint_as_float(b.y), __uint_as_float(b.z), __uint_as_float(b.w)},
                    {__uint_as_float(c.x), __uint_as_float(c.y), __uint_as_float(c.z), __uint_as_float(c.w)}};
}

// the acceleration field `f` gives a body, in the spec's order of operations; false: no contribution (nothing is added, not + 0)
template <bool DRAG>
__device__ __forceinline__ bool field_acceleration(const FieldRec& f, float dt, const float4 m, const float4 v, float& ax, float& ay, float& aa)
{
    const float x = m.z, y = m.w;
    if (f.shape == PHX_REGION_BOX) {                            // closed; a NaN centre fails every comparison
        if (!(x >= f.region[0] && x <= f.region[2] && y >= f.region[1] && y <= f.region[3])) return false;
    } else if (f.shape == PHX_REGION_DISC) {
        const float dx = x - f.region[0], dy = y - f.region[1];
        if (!(dx * dx + dy * dy <= f.region[2] * f.region[2])) return false;
    }
    if (f.kind == PHX_FIELD_UNIFORM) {
        ax = f.value[0]; ay = f.value[1]; aa = f.value[2];
    } else if (f.kind == PHX_FIELD_RADIAL) {
        const float dx = x - f.value[0], dy = y - f.value[1];
        const float d = sqrtf(dx * dx + dy * dy);               // (sqrtf and /: correctly rounded under the library's flags)
        if (!(d > 0.0009765625f)) return false;                 // 2^-10: no direction at the centre
        float mag = f.value[2];
        if (f.value[3] > 0.0f) {
            const float t = 1.0f - d / f.value[3];
            if (!(t > 0.0f)) return false;
            mag = f.value[2] * t;
        }
        ax = (dx / d) * mag; ay = (dy / d) * mag; aa = 0.0f;
    } else {                                                    // PHX_FIELD_DRAG (instantiated only for lists that hold one)
        if (!DRAG) return false;
        const float kl = f.value[2] * dt, ka = f.value[3] * dt;
        const float c = (kl < 1.0f ? kl : 1.0f) / dt, ca = (ka < 1.0f ? ka : 1.0f) / dt;
        ax = (f.value[0] - v.x) * c; ay = (f.value[1] - v.y) * c; aa = (0.0f - v.z) * ca;
    }
    if (f.flags & PHX_FIELD_FORCE) { ax *= m.x; ay *= m.x; aa *= m.y; }
    return true;
}

// DRAG: the list holds a DRAG field (the velocities are read); MASKED: the masks are tested — against the filter column's category
// where the column exists, against category 1 where it does not; PULSE: the destination is the velocity array itself and what the
// fields read as the velocity is what the sum starts from.
// `dst`: every body's slot is written.  `from_dst`: the sum starts from dst[i] (pending accelerations; always for a pulse), else from 0.
// (`vel` and `dst` may be the same array and `dst` is read and written: neither is __restrict__)
template <bool DRAG, bool MASKED, bool PULSE>
static __global__ void __launch_bounds__(256) k_apply_fields(const phx_field* __restrict__ fields, int count, float dt, const float4* __restrict__ mpos, const float4* vel,
                                                             const uint4* __restrict__ filters, float4* dst, int from_dst, int n)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const float4 m = mpos[i];
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (PULSE || from_dst) s = dst[i];
        float4 v = s;
        if (DRAG && !PULSE) v = vel[i];
        unsigned category = FILTER_DEFAULT_CATEGORY;
        if (MASKED && filters) category = filters[i].x;
        if (m.x > 0.0f) {                                       // the rule gravity uses (ref: World.cpp:44): statics and sleepers are not affected
            for (int k = 0; k < count; ++k) {
                const FieldRec f = load_field(fields, k);
                if (MASKED && !(category & f.mask)) continue;
                float ax, ay, aa;
                if (!field_acceleration<DRAG>(f, dt, m, v, ax, ay, aa)) continue;
                s.x = s.x + ax; s.y = s.y + ay; s.z = s.z + aa;
            }
        }
        dst[i] = s;
    }
}

// phx_world_apply_impulses: one lane per listed body (distinct: no two lanes touch the same body); the angular sign is the engine's
// clockwise-positive angular velocity (tests/pin_spec.py apply)
static __global__ void __launch_bounds__(256) k_apply_impulses(const int* __restrict__ idx, const float* __restrict__ q, int count, const float4* __restrict__ mpos,
                                                               float4* __restrict__ vel)
{
    for (int k = blockIdx.x * blockDim.x + threadIdx.x; k < count; k += gridDim.x * blockDim.x) {
        const int i = idx[k];
        const float4 m = mpos[i];
        if (!(m.x > 0.0f)) continue;
        const float jx = q[4 * k], jy = q[4 * k + 1];
        const float rx = q[4 * k + 2] - m.z, ry = q[4 * k + 3] - m.w;
        float4 o = vel[i];
        o.x = o.x + m.x * jx; o.y = o.y + m.x * jy;
        o.z = o.z - m.y * (rx * jy - ry * jx);
        vel[i] = o;
    }
}

} // namespace phx
