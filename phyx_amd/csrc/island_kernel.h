// island_kernel.h — the island kernel (included by islands.hip only; see island_view.h for why it has a translation unit of
// its own).
#pragma once

#include "solver_kernels.h"

#include <type_traits>

namespace phx {

// ---- island kernel: one workgroup solves one GROUP of the schedule entirely out of LDS -----------------
// (Refresh, PreStep and every impulse / displacement sweep of ref: Solver.cpp:130-215 SolveJointIsland.)
// A lane owns one UNIT (schedule.h: the one or two joints of a body pair) for the whole solve: the refreshed constants and
// the accumulators of both joints live in registers, the group's body velocities live in LDS, classes are separated by
// workgroup barriers instead of kernel launches, and HBM is touched once on the way in and once on the way out.  A step
// sweeps the unit's leader and then its follower on one read and one write of the two bodies: half the barriers and LDS
// round trips per joint of the one-joint-per-lane kernel of round 2.  The early exit of ref: Solver.cpp:189 / :210 is per
// group, exactly like the reference's per-island loop.
// Two shapes: 256 lanes / 512 joints / 768 bodies (4 workgroups per CU — the 200-box columns of cfg 2 are ~205 units each)
// and 512 lanes / 1024 joints / 1024 bodies (2 per CU — the 500-box columns of cfg 5 are ~510 units each); both leave a
// lane 128 VGPRs.
// phase stamps of the island kernel (tools/island_trace.py; the constant 100 MHz clock all XCDs share): 0 start, 1 records loaded, 2 refreshed, 3 pre-stepped, 4 swept,
// 5 written back; word 6 = XCC id | s_memtime ticks of the whole workgroup << 4, word 7 = classes << 32 | impulse sweeps executed
#define PHX_ISL_STAMP(k) do { if (TRACE && threadIdx.x == 0) iv.trace[(size_t)group * 8 + (k)] = wall_clock64(); } while (0)
// ... and the stamps between them (island_view.h ISL_PHASE_WORDS; tools/island_phase_account.py)
#define PHX_ISL_PHASE(k) do { if (TRACE && threadIdx.x == 0 && iv.phase_trace) iv.phase_trace[(size_t)group * ISL_PHASE_WORDS + (k)] = wall_clock64(); } while (0)

// ---- body-state storage of the island kernel: fp32 (default) or the fp16 ablation ------------------------------
template <bool HALF> struct BodyStore { using type = float4; };
template <> struct BodyStore<true> { using type = uint2; };

__device__ __forceinline__ float4 body_load(const float4* p, int i) { return p[i]; }
__device__ __forceinline__ void body_store(float4* p, int i, float4 v) { p[i] = v; }
__device__ __forceinline__ unsigned f2h_bits(float f) { return (unsigned)__half_as_ushort(__float2half_rn(f)); }
__device__ __forceinline__ float h2f_bits(unsigned h) { return __half2float(__ushort_as_half((unsigned short)h)); }
__device__ __forceinline__ float4 body_load(const uint2* p, int i)
{
    const uint2 r = p[i];
    return make_float4(h2f_bits(r.x & 0xFFFFu), h2f_bits(r.x >> 16), h2f_bits(r.y & 0xFFFFu), __int_as_float((int)(short)(r.y >> 16)));
}
__device__ __forceinline__ void body_store(uint2* p, int i, float4 v)
{
    p[i] = make_uint2(f2h_bits(v.x) | (f2h_bits(v.y) << 16), f2h_bits(v.z) | ((unsigned)(unsigned short)(short)__float_as_int(v.w) << 16));
}

// fp16 ablation: what a store + load of the body record would leave in the registers (identity for fp32 state)
template <bool HALF> __device__ __forceinline__ float4 body_round(float4 v)
{
    if (!HALF) return v;
    return make_float4(h2f_bits(f2h_bits(v.x)), h2f_bits(f2h_bits(v.y)), h2f_bits(f2h_bits(v.z)), __int_as_float((int)(short)__float_as_int(v.w)));
}

// the refreshed constants and accumulators of one joint, in registers for the whole solve; the arithmetic is solver_kernels.h's
struct IslJoint : JointConsts { float accN, accF, accD; };

// MAT (materials, include/phyx_amd.h; k_solve_islands_mat): a lane gathers its bodies' {friction, restitution} beside their records and
// parks them in the displacement table until the refresh has read its unit's two (the displacing velocities go there behind the next
// barrier: nothing reads them before the sweeps); the unit's friction coefficient then lives in one register for the whole solve.
template <bool MAT, class V> __device__ __forceinline__ float2 view_material(const V& v, int body)
{
    if constexpr (MAT) return v.mat[body];
    else return make_float2(0.f, 0.f);
}

template <int T, int NB, bool HALF, bool TRACE = false>
__global__ void __launch_bounds__(T, 4) k_solve_islands(SolverView v, IslandView iv, BodyView bv,
                                                            phx_contact_joint* __restrict__ joints,
                                                            const phx_contact_point* __restrict__ cps, int ci, int pi)
{
    constexpr bool MAT = false;
#include "island_kernel_body.h"
}

// the same with materials (v.mat: per body {friction, restitution}; fp32 body state, no trace)
template <int T, int NB>
__global__ void __launch_bounds__(T, 4) k_solve_islands_mat(SolverViewMat v, IslandView iv, BodyView bv,
                                                                phx_contact_joint* __restrict__ joints,
                                                                const phx_contact_point* __restrict__ cps, int ci, int pi)
{
    constexpr bool MAT = true, HALF = false, TRACE = false;
#include "island_kernel_body.h"
}

} // namespace phx
