// sleep.hip — DeviceSleep: the launches of the sleep pass and of the wake by list (sleep.h, sleep_kernels.h).
#include "solver.h"
#include "island_view.h"
#include "schedule_kernels.h"      // (k_cc_compress_window, k_cc_compress)
#include "sleep_kernels.h"

namespace phx {

static inline int sgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }

int DeviceSleep::enable(const phx_sleep_params& p, hipStream_t stream)
{
    if (!words_.p) {
        PHX_TRY(words_.reserve(SLEEP_WORDS));
        PHX_HIP(hipMemsetAsync(words_.p, 0, SLEEP_WORDS * sizeof(unsigned), stream));
    }
    params_ = p;
    on_ = true;
    return PHX_OK;
}

int DeviceSleep::clear_totals(hipStream_t stream)
{
    if (words_.p) PHX_HIP(hipMemsetAsync(words_.p, 0, SLEEP_WORDS * sizeof(unsigned), stream));
    return PHX_OK;
}

int DeviceSleep::scratch(int nb)
{
    const size_t n = (size_t)std::max(nb, 1);
    PHX_TRY(parent_.reserve(n)); PHX_TRY(skip_.reserve(n)); PHX_TRY(struck_.reserve(n));
    PHX_TRY(root_bits_.reserve(n)); PHX_TRY(root_timer_.reserve(n));
    return clear_.reserve(1);
}

int DeviceSleep::fill(SleepCell* cells, int nb, hipStream_t stream)
{
    if (nb) hipLaunchKernelGGL(k_sleep_fill, dim3(sgrid(nb)), dim3(256), 0, stream, cells, nb);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

// link (the manifolds, then every kind's list), then the flattening pass in its two launches: parent_[i] = the smallest body of i's
// component, -1 outside the graph
int DeviceSleep::label(int nb, const SleepGraph& g, unsigned char* struck, const SleepCell* cells, const float4* vel, hipStream_t stream)
{
    if (g.nm) hipLaunchKernelGGL(k_sleep_link_manifolds, dim3(sgrid(g.nm)), dim3(256), 0, stream, g.manifolds, g.nm, nb, parent_.p, (const unsigned char*)skip_.p, g.flags,
                                 struck, cells, vel);
    for (const SleepGraph::List& l : g.units)
        if (l.count) hipLaunchKernelGGL(k_sleep_link_units, dim3(sgrid(l.count)), dim3(256), 0, stream, l.records, l.stride, l.count, nb, parent_.p, (const unsigned char*)skip_.p);
    hipLaunchKernelGGL(k_cc_compress_window, dim3(std::max(1, div_up(nb, CCW_BODIES))), dim3(CCW_T), 0, stream, parent_.p, nb);
    hipLaunchKernelGGL(k_cc_compress, dim3(sgrid(nb)), dim3(256), 0, stream, parent_.p, nb, clear_.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceSleep::pass(const WorldBodies& w, phx_rigid_body* records, SleepCell* cells, int nb, const SleepGraph& g, float dt, hipStream_t stream)
{
    if (!nb) return PHX_OK;
    PHX_TRY(scratch(nb));
    const float lin2 = params_.linear_tolerance * params_.linear_tolerance, ang2 = params_.angular_tolerance * params_.angular_tolerance;
    hipLaunchKernelGGL(k_sleep_begin, dim3(sgrid(nb)), dim3(256), 0, stream, (const float4*)w.s.mpos, (const float4*)w.s.vel, cells, nb, lin2, ang2, dt, parent_.p, skip_.p,
                       struck_.p, root_bits_.p, root_timer_.p, words_.p);
    PHX_TRY(label(nb, g, struck_.p, cells, w.s.vel, stream));
    hipLaunchKernelGGL(k_sleep_reduce, dim3(sgrid(nb)), dim3(256), 0, stream, (const int*)parent_.p, (const SleepCell*)cells, (const unsigned char*)struck_.p, nb,
                       root_bits_.p, root_timer_.p);
    hipLaunchKernelGGL(k_sleep_apply, dim3(sgrid(nb)), dim3(256), 0, stream, (const int*)parent_.p, cells, nb, w.s.mpos, w.s.vel, records, (const unsigned*)root_bits_.p,
                       (const unsigned*)root_timer_.p, params_.time_to_sleep, words_.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceSleep::wake(const WorldBodies& w, phx_rigid_body* records, SleepCell* cells, int nb, const SleepGraph& g, const int* d_list, int count,
                      const unsigned* d_keep, bool all, hipStream_t stream)
{
    if (!nb || (!all && !d_keep && !count)) return PHX_OK;
    PHX_TRY(scratch(nb));
    if (!all) {
        hipLaunchKernelGGL(k_sleep_wake_begin, dim3(sgrid(nb)), dim3(256), 0, stream, (const SleepCell*)cells, nb, parent_.p, skip_.p, root_bits_.p);
        PHX_TRY(label(nb, g, nullptr, cells, w.s.vel, stream));
        hipLaunchKernelGGL(k_sleep_name, dim3(sgrid(d_keep ? nb : count)), dim3(256), 0, stream, d_list, count, d_keep, nb, (const int*)parent_.p, root_bits_.p);
    }
    hipLaunchKernelGGL(k_sleep_wake_apply, dim3(sgrid(nb)), dim3(256), 0, stream, (const int*)parent_.p, cells, nb, w.s.mpos, records, (const unsigned*)root_bits_.p,
                       all ? 1 : 0, words_.p);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceSleep::states(const float4* mpos, const SleepCell* cells, int nb, phx_sleep_state* d_out, hipStream_t stream)
{
    if (nb) hipLaunchKernelGGL(k_sleep_states, dim3(sgrid(nb)), dim3(256), 0, stream, mpos, cells, nb, d_out);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

} // namespace phx
