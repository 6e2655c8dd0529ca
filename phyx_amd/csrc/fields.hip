// fields.hip — force fields: the validator of the C ABI (host only) and the launches of field_kernels.h (fields.h).
#include "field_kernels.h"

#include <cmath>

namespace phx {

static inline int fgrid(int n) { return std::max(1, std::min(div_up(n, 256), 4096)); }      // (the world's per-body grid: grid-stride beyond 4096 workgroups)

FieldTraits field_traits(const phx_field* fields, int count)
{
    FieldTraits t = {false, true};
    for (int k = 0; k < count; ++k) {
        t.drag |= fields[k].kind == PHX_FIELD_DRAG;
        t.plain_masks &= fields[k].mask == 0xFFFFFFFFu;
    }
    return t;
}

// the eight instances: the three template arguments are host-side decisions
template <bool PULSE>
static void launch_fields(const FieldBodies& b, const phx_field* d_fields, int count, FieldTraits t, float dt, float4* dst, bool from_dst, hipStream_t stream)
{
    const bool masked = b.filters || !t.plain_masks;      // (a column may hold category 0, which no mask passes: it is read whenever it exists)
    const dim3 grid(fgrid(b.n)), block(256);
#define PHX_FIELDS(D, M) hipLaunchKernelGGL((k_apply_fields<D, M, PULSE>), grid, block, 0, stream, d_fields, count, dt, b.mpos, (const float4*)b.vel, b.filters, dst, from_dst ? 1 : 0, b.n)
    if (t.drag) { if (masked) PHX_FIELDS(true, true); else PHX_FIELDS(true, false); }
    else { if (masked) PHX_FIELDS(false, true); else PHX_FIELDS(false, false); }
#undef PHX_FIELDS
}

int DeviceFields::set(const phx_field* fields, int count, const phx_field* d_staged, hipStream_t stream)
{
    if (count) {
        PHX_TRY(dev_.reserve(PHX_MAX_FIELDS));
        PHX_HIP(hipMemcpyAsync(dev_.p, d_staged, (size_t)count * sizeof(phx_field), hipMemcpyDeviceToDevice, stream));
    }
    host_.assign(fields, fields + count);
    traits_ = field_traits(fields, count);
    return PHX_OK;
}

int DeviceFields::apply(const FieldBodies& b, float4* accel, bool from_pending, float dt, hipStream_t stream)
{
    if (!count() || !b.n) return PHX_OK;
    launch_fields<false>(b, dev_.p, count(), traits_, dt, accel, from_pending, stream);
    PHX_HIP(hipGetLastError());
    ++passes_;
    return PHX_OK;
}

int DeviceFields::pulse(const FieldBodies& b, const phx_field* d_fields, int count, FieldTraits traits, hipStream_t stream)
{
    if (!count || !b.n) return PHX_OK;
    launch_fields<true>(b, d_fields, count, traits, 1.0f, b.vel, true, stream);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceFields::impulses(const FieldBodies& b, const int* d_bodies, const float* d_impulses, int count, hipStream_t stream)
{
    if (!count) return PHX_OK;
    hipLaunchKernelGGL(k_apply_impulses, dim3(fgrid(count)), dim3(256), 0, stream, d_bodies, d_impulses, count, b.mpos, b.vel);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

} // namespace phx

extern "C" int phx_field_check(const phx_field* fields, int32_t count)
{
    using phx::set_error;
    static const char* const what = "phx_field_check";
    if (count < 0) { set_error("%s: negative count %d", what, count); return PHX_ERR_INVALID; }
    if (count > PHX_MAX_FIELDS) { set_error("%s: %d fields exceed PHX_MAX_FIELDS (%d)", what, count, PHX_MAX_FIELDS); return PHX_ERR_INVALID; }
    if (count && !fields) { set_error("%s: null array", what); return PHX_ERR_INVALID; }
    for (int k = 0; k < count; ++k) {
        const phx_field& f = fields[k];
        if (f.kind < PHX_FIELD_UNIFORM || f.kind > PHX_FIELD_DRAG) { set_error("%s: field %d: unknown kind %d", what, k, f.kind); return PHX_ERR_INVALID; }
        if (f.shape < PHX_REGION_ALL || f.shape > PHX_REGION_DISC) { set_error("%s: field %d: unknown shape %d", what, k, f.shape); return PHX_ERR_INVALID; }
        if (f.flags & ~PHX_FIELD_FORCE) { set_error("%s: field %d: flags 0x%x hold an unknown bit", what, k, f.flags); return PHX_ERR_INVALID; }
        if (!f.mask) { set_error("%s: field %d: mask 0 matches no body", what, k); return PHX_ERR_INVALID; }
        for (int c = 0; c < 4; ++c) {
            if (!std::isfinite(f.region[c])) { set_error("%s: field %d: region[%d] is not finite", what, k, c); return PHX_ERR_INVALID; }
            if (!std::isfinite(f.value[c])) { set_error("%s: field %d: value[%d] is not finite", what, k, c); return PHX_ERR_INVALID; }
        }
        if (f.shape == PHX_REGION_BOX && !(f.region[0] <= f.region[2] && f.region[1] <= f.region[3])) { set_error("%s: field %d: the box's min exceeds its max", what, k); return PHX_ERR_INVALID; }
        if (f.shape == PHX_REGION_DISC && !(f.region[2] >= 0.f)) { set_error("%s: field %d: negative disc radius %g", what, k, (double)f.region[2]); return PHX_ERR_INVALID; }
        // the words a shape or a kind does not use are exactly 0 (all bits)
        const int region_used = f.shape == PHX_REGION_ALL ? 0 : f.shape == PHX_REGION_DISC ? 3 : 4, value_used = f.kind == PHX_FIELD_UNIFORM ? 3 : 4;
        for (int c = region_used; c < 4; ++c) { uint32_t u; std::memcpy(&u, &f.region[c], 4); if (u) { set_error("%s: field %d: region[%d] is unused by its shape and must be 0", what, k, c); return PHX_ERR_INVALID; } }
        for (int c = value_used; c < 4; ++c) { uint32_t u; std::memcpy(&u, &f.value[c], 4); if (u) { set_error("%s: field %d: value[%d] is unused by its kind and must be 0", what, k, c); return PHX_ERR_INVALID; } }
        if (f.kind == PHX_FIELD_RADIAL && !(f.value[3] >= 0.f)) { set_error("%s: field %d: negative falloff radius %g", what, k, (double)f.value[3]); return PHX_ERR_INVALID; }
        if (f.kind == PHX_FIELD_DRAG && !(f.value[2] >= 0.f && f.value[3] >= 0.f)) { set_error("%s: field %d: negative drag coefficient", what, k); return PHX_ERR_INVALID; }
    }
    return PHX_OK;
}
