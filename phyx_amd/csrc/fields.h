// fields.h — force fields (include/phyx_amd.h FORCE FIELDS; the definition: tests/field_spec.py): wind, attractors, drag zones and
// blasts computed on the device from the bodies' own state.
//
// The list is a setting of the world, at most PHX_MAX_FIELDS records of 48 bytes: the host keeps the copy the getter returns, the
// device a copy the pass reads (uploaded by set(), never read back).  The pass of a step is ONE launch at the head of the step
// (field_kernels.h k_apply_fields): a lane per body sums the fields' accelerations in list order into the world's pending
// accelerations, which the unchanged IntegrateVelocity then consumes.  A pulse is the same kernel body with the velocities as its
// destination and dt = 1; an impulse batch is a scatter like the edits'.  A world with an empty list launches nothing.
#pragma once

#include "common.h"

namespace phx {

static_assert(sizeof(phx_field) == 48, "a field record is three 16-byte granules");

// what of the bodies a pass reads (resident arrays, body_view.h) and, null where absent, the collision filters' column
struct FieldBodies {
    const float4* mpos;
    float4* vel;
    const uint4* filters;
    int n;
};

// which instance of the kernel a list needs: decided once per list on the host (field_kernels.h)
struct FieldTraits { bool drag, plain_masks; };      // some field is a DRAG / every mask is all-ones
FieldTraits field_traits(const phx_field* fields, int count);

class DeviceFields {
public:
    int count() const { return (int)host_.size(); }
    const std::vector<phx_field>& list() const { return host_; }
    long long passes() const { return passes_; }
    // the list becomes `fields` (checked by the caller: phx_field_check); `d_staged`: the same records on the device, staged by the
    // caller, copied into the buffer the passes read behind whatever `stream` holds
    int set(const phx_field* fields, int count, const phx_field* d_staged, hipStream_t stream);
    // the pass of one step: accel[i] = (from_pending ? accel[i] : 0) + the fields' accelerations, for every body
    int apply(const FieldBodies& b, float4* accel, bool from_pending, float dt, hipStream_t stream);
    // a one-shot list `d_fields` (on the device): vel[i] += what it would add in a step of dt = 1
    static int pulse(const FieldBodies& b, const phx_field* d_fields, int count, FieldTraits traits, hipStream_t stream);
    // impulses {J.x, J.y, point.x, point.y} on the listed bodies (distinct, in range: checked by the caller)
    static int impulses(const FieldBodies& b, const int* d_bodies, const float* d_impulses, int count, hipStream_t stream);
private:
    std::vector<phx_field> host_;
    DevBuf<phx_field> dev_;
    FieldTraits traits_ = {false, true};
    long long passes_ = 0;
};

} // namespace phx
