// sweep.hip — DeviceSweep: the launches of the continuous bodies' pass (sweep.h, sweep_kernels.h).
#include "sweep.h"
#include "sweep_kernels.h"

namespace phx {

static inline int sweep_grid(int items) { return std::max(1, std::min(div_up(items, 256), 2048)); }

int DeviceSweep::words(hipStream_t stream)
{
    if (words_.p) return PHX_OK;
    PHX_TRY(words_.reserve(SWEEP_WORDS));
    PHX_HIP(hipMemsetAsync(words_.p, 0, SWEEP_WORDS * sizeof(unsigned), stream));
    return PHX_OK;
}

int DeviceSweep::begin(const float4* mpos, float4* cells, int nb, Readback& rb, hipStream_t stream)
{
    if (stale_ || list_nb_ != nb) {
        PHX_TRY(words(stream));
        PHX_TRY(list_.reserve((size_t)std::max(nb, 1)));
        hipLaunchKernelGGL(k_sweep_list, dim3(1), dim3(256), 0, stream, (const float4*)cells, nb, list_.p, words_.p + SWEEP_LISTED);
        PHX_HIP(hipGetLastError());
        unsigned listed = 0;
        PHX_TRY(rb.add(&listed, words_.p + SWEEP_LISTED, sizeof listed, stream));
        PHX_TRY(rb.wait(stream));
        listed_ = (int)listed; list_nb_ = nb; stale_ = false;
    }
    if (!listed_) return PHX_OK;
    hipLaunchKernelGGL(k_sweep_start, dim3(sweep_grid(listed_)), dim3(256), 0, stream, (const int*)list_.p, listed_, mpos, cells);
    PHX_HIP(hipGetLastError());
    return PHX_OK;
}

int DeviceSweep::pass(const WorldBodies& w, const float4* cells, int nb, const SweepTables& tables, int shapes, hipStream_t stream)
{
    if (!listed_) { last_ = 0; return PHX_OK; }
    PHX_TRY(slots_.reserve((size_t)listed_));
    const dim3 grid(std::max(1, std::min(div_up(listed_, 4), 4096))), block(256);      // one wave per listed body, four to a workgroup
    unsigned long long* const totals = reinterpret_cast<unsigned long long*>(words_.p + SWEEP_CLAMPS);
    if (timed_) PHX_HIP(hipEventRecord(t0_, stream));
    switch (shapes) {
    case SWEEP_POLYGONS: hipLaunchKernelGGL(k_sweep_bodies<SWEEP_POLYGONS>, grid, block, 0, stream, w, nb, (const int*)list_.p, listed_, cells, tables, slots_.p, totals); break;
    case SWEEP_CAPSULES: hipLaunchKernelGGL(k_sweep_bodies<SWEEP_CAPSULES>, grid, block, 0, stream, w, nb, (const int*)list_.p, listed_, cells, tables, slots_.p, totals); break;
    case SWEEP_SHAPES: hipLaunchKernelGGL(k_sweep_bodies<SWEEP_SHAPES>, grid, block, 0, stream, w, nb, (const int*)list_.p, listed_, cells, tables, slots_.p, totals); break;
    default: hipLaunchKernelGGL(k_sweep_bodies<SWEEP_BOXES>, grid, block, 0, stream, w, nb, (const int*)list_.p, listed_, cells, tables, slots_.p, totals); break;
    }
    PHX_HIP(hipGetLastError());
    if (timed_) { PHX_HIP(hipEventRecord(t1_, stream)); have_time_ = true; }
    last_ = listed_;
    ++passes_;
    return PHX_OK;
}

int DeviceSweep::hits(phx_sweep_hit* out, int cap, int64_t* total, Readback& rb, hipStream_t stream)
{
    if (total) *total = 0;
    if (!last_) return PHX_OK;
    PHX_TRY(hits_.reserve((size_t)last_));
    hipLaunchKernelGGL(k_sweep_hits, dim3(1), dim3(256), 0, stream, (const phx_sweep_hit*)slots_.p, last_, hits_.p, words_.p + SWEEP_HITS);
    PHX_HIP(hipGetLastError());
    unsigned found = 0;
    PHX_TRY(rb.add(&found, words_.p + SWEEP_HITS, sizeof found, stream));
    PHX_TRY(rb.wait(stream));
    if (total) *total = (int64_t)found;
    if ((int64_t)found > (int64_t)cap) { set_error("phx_world_sweep_hits: %u hits, room for %d", found, cap); return PHX_ERR_CAPACITY; }
    if (!found) return PHX_OK;
    PHX_TRY(rb.add(out, hits_.p, (size_t)found * sizeof(phx_sweep_hit), stream));
    return rb.wait(stream);
}

int DeviceSweep::timing(bool enable)
{
    if (enable && !t0_) { PHX_HIP(hipEventCreate(&t0_)); PHX_HIP(hipEventCreate(&t1_)); }
    timed_ = enable;
    have_time_ = have_time_ && enable;
    return PHX_OK;
}

int DeviceSweep::pass_ms(double* ms)
{
    *ms = 0.0;
    if (!have_time_) return PHX_OK;
    float t = 0.f;
    PHX_HIP(hipEventSynchronize(t1_));
    PHX_HIP(hipEventElapsedTime(&t, t0_, t1_));
    *ms = (double)t;
    return PHX_OK;
}

void DeviceSweep::release()
{
    if (t0_) (void)hipEventDestroy(t0_);
    if (t1_) (void)hipEventDestroy(t1_);
    t0_ = t1_ = nullptr; timed_ = have_time_ = false;
}

int DeviceSweep::counts(int64_t* passes, int64_t* clamps_total, Readback& rb, hipStream_t stream)
{
    unsigned long long clamps = 0;
    if (words_.p) {
        PHX_TRY(rb.add(&clamps, words_.p + SWEEP_CLAMPS, sizeof clamps, stream));
        PHX_TRY(rb.wait(stream));
    }
    if (passes) *passes = (int64_t)passes_;
    if (clamps_total) *clamps_total = (int64_t)clamps;
    return PHX_OK;
}

} // namespace phx
