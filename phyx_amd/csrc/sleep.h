// sleep.h — sleeping (include/phyx_amd.h SLEEPING; the definition: tests/sleep_spec.py): settled components rest on the device.
//
// A sleeper is a static body to every kernel of the step: mpos.xy == 0 and zero velocities, its own masses kept in the per-body
// column below (a World BodyTable: it travels with uploads, spawns, removals and resets like the other columns).  The pass that
// decides who sleeps and who wakes runs behind IntegratePosition (sleep.hip, sleep_kernels.h): timers, one label pass over the
// graph of manifolds and units, a reduction per root by order-free atomics (or, min), and the apply.  Every result is a min, an
// or, or a label equal to the smallest index — nothing depends on the order of the atomics, so the device equals the spec byte
// for byte.  The number of bodies whose static-ness changed stays in a device word that the next step's count readback brings
// along (world.hip refresh_contact_joints): no host wait of its own.
#pragma once

#include "body_view.h"

namespace phx {

struct SleepCell { float timer; int32_t asleep; float inv_mass, inv_inertia; };      // 16 B: the saved masses are a sleeper's own
static_assert(sizeof(SleepCell) == 16 && sizeof(phx_sleep_state) == 16, "one 16-byte granule per body");

struct SleepColumn {                   // include/phyx_amd.h SLEEPING
    using value = SleepCell;
    using api = phx_sleep_state;
    static constexpr const char* plural = "sleep states";
    static __host__ __device__ value initial() { return SleepCell{0.f, 0, 0.f, 0.f}; }      // awake, timer 0
    static bool is_initial(const value& v) { return v.asleep == 0; }
};

// the edges of the pass: the manifolds (with the flags column for the sensor rule, null: no flags) and every kind's unit list
// (records begin with body1, body2)
struct SleepGraph {
    const phx_manifold* manifolds; int nm;
    const uint32_t* flags;
    struct List { const char* records; int stride, count; } units[4];
};

// the words the device keeps (DeviceSleep::words()): [0] bodies whose static-ness changed since the pass last cleared it,
// [2..3] bodies put to sleep, [4..5] bodies woken, each a 64-bit total since the words were cleared
constexpr int SLEEP_WORDS = 8, SLEEP_CHANGED = 0, SLEEP_SLEPT = 2, SLEEP_WOKEN = 4;

class DeviceSleep {
public:
    bool on() const { return on_; }
    const phx_sleep_params& params() const { return params_; }
    int enable(const phx_sleep_params& p, hipStream_t stream);      // (the words are cleared by the first enable)
    void disable() { on_ = false; }
    int clear_totals(hipStream_t stream);
    const unsigned* words() const { return words_.p; }
    // the pass of one step, queued on `stream` behind IntegratePosition
    int pass(const WorldBodies& w, phx_rigid_body* records, SleepCell* cells, int nb, const SleepGraph& g, float dt, hipStream_t stream);
    // the sleeping components of the named bodies wake: `d_list` (count entries), or the bodies whose `d_keep` word is 0, or (`all`) every sleeper
    int wake(const WorldBodies& w, phx_rigid_body* records, SleepCell* cells, int nb, const SleepGraph& g, const int* d_list, int count,
             const unsigned* d_keep, bool all, hipStream_t stream);
    // out[i] = body i's phx_sleep_state (cells null: every body awake with timer 0)
    int states(const float4* mpos, const SleepCell* cells, int nb, phx_sleep_state* d_out, hipStream_t stream);
    int fill(SleepCell* cells, int nb, hipStream_t stream);      // every body the default
private:
    int scratch(int nb);
    int label(int nb, const SleepGraph& g, unsigned char* struck, const SleepCell* cells, const float4* vel, hipStream_t stream);
    bool on_ = false;
    phx_sleep_params params_ = {0.f, 0.f, 0.f};
    DevBuf<unsigned> words_;
    DevBuf<int> parent_, clear_;
    DevBuf<unsigned char> skip_, struck_;
    DevBuf<unsigned> root_bits_, root_timer_;
};

} // namespace phx
