// sweep.h — continuous bodies (include/phyx_amd.h CONTINUOUS BODIES; the definition: tests/sweep_spec.py): fast bodies swept so that
// they cannot tunnel through static ones.
//
// The per-body column {rc, start} is a World BodyTable (world_kernels.h SweepColumn): it travels with uploads, spawns, removals, resets
// and snapshots like the other columns.  Here: the compact list of the continuous bodies (rebuilt by one ordered compaction when the set
// or the body count changed), the two launches of a step — start := pos in front of the integrator, k_sweep_bodies behind it — and the
// clamps of the last pass, which stay on the device as one slot per listed body until somebody asks for them.
#pragma once

#include "body_view.h"

namespace phx {

// what the pass reads beside the resident arrays; a null pointer: the world has no such column (every body the default) or no exclusion
struct SweepTables {
    const uint4* filters;                // FilterColumn
    const uint32_t* flags;               // FlagsColumn
    const unsigned long long* xtable;    // the exclusions' table (exclusions.h ExclusionView)
    unsigned xmask;
    const unsigned* xmember;
};

// the instantiations, by the bits that pick UpdateManifolds' (world_kernels.h AllBoxes ... BodyPolygons)
enum { SWEEP_BOXES = 0, SWEEP_SHAPES = 1, SWEEP_CAPSULES = 2, SWEEP_POLYGONS = 3 };

// the words the device keeps (DeviceSweep): [0..1] the clamps since the world was made, a 64-bit total; [2] a list's length; [3] a hit list's length
constexpr int SWEEP_WORDS = 4, SWEEP_CLAMPS = 0, SWEEP_LISTED = 2, SWEEP_HITS = 3;

class DeviceSweep {
public:
    void changed() { stale_ = true; }                     // the set of continuous bodies, or the bodies' numbering, may have changed
    void forget() { stale_ = true; listed_ = 0; last_ = 0; }      // set_state / load: no list, and the last pass's clamps are another world's
    // in front of the integrator: the list, rebuilt unless current (one host round trip, then), and start := pos of the listed bodies
    int begin(const float4* mpos, float4* cells, int nb, Readback& rb, hipStream_t stream);
    // behind the integrator: the pass over the listed bodies (`w`: the resident arrays with kinds and polys; `shapes`: SWEEP_BOXES ...)
    int pass(const WorldBodies& w, const float4* cells, int nb, const SweepTables& tables, int shapes, hipStream_t stream);
    int listed() const { return listed_; }
    // the last pass's clamps, ascending by body: *total always; PHX_ERR_CAPACITY (nothing written) when cap is smaller
    int hits(phx_sweep_hit* out, int cap, int64_t* total, Readback& rb, hipStream_t stream);
    int counts(int64_t* passes, int64_t* clamps_total, Readback& rb, hipStream_t stream);
    // the measurement (tools/sweep_cost.py): while enabled every pass's kernel stands between two HIP events; pass_ms waits for the last one
    int timing(bool enable);
    int pass_ms(double* ms);
    void release();                      // the events go (the owner's device is current, its stream drained)

private:
    int words(hipStream_t stream);
    DevBuf<unsigned> words_;
    DevBuf<int> list_;
    DevBuf<phx_sweep_hit> slots_, hits_;
    bool stale_ = true;
    int listed_ = 0, list_nb_ = -1;      // the list's length and the body count it was built for
    int last_ = 0;                       // slots the last pass wrote
    long long passes_ = 0;
    bool timed_ = false, have_time_ = false;
    hipEvent_t t0_ = nullptr, t1_ = nullptr;
};

} // namespace phx
