// solver_bench.hip — DeviceSolver's bench harness: staged copies of the input, the timed loop, the checksum of its results.
#include "solver.h"
#include "solver_kernels.h"

#include <algorithm>
#include <cstdlib>

namespace phx {

// One private copy of the solver's in/out arrays per timed step — the resident velocities (body_view.h) and the joints — made
// outside the timed region: bench() then solves copy k in step k instead of restoring one working copy in front of every step (copy
// dispatches that are the bench's own scaffolding, not SolveJoints).  The records the caller hands over are converted to the
// resident layout here, before the clock starts: the timed solves run on HBM-resident inputs in the layout the World keeps
// them in.  Consumed by the next bench() call on the same arrays.
int DeviceSolver::bench_stage(const void* d_bodies, int nb, const void* d_joints, int nj, int steps)
{
    PHX_REQUIRE(nb >= 0 && nj >= 0 && steps >= 0 && steps <= 4096, "bad bench_stage arguments");
    PHX_TRY(use_device(device_));
    PHX_TRY(synchronize());
    bench_.staged_steps = 0;
    const size_t bytes = (size_t)steps * ((size_t)nb * 2 * sizeof(float4) + (size_t)nj * sizeof(phx_contact_joint));
    if (!steps || bytes > (8ull << 30)) return PHX_OK;      // too big to stage: bench() restores in front of every step
    PHX_TRY(bench_.stage_vel.reserve(std::max<size_t>((size_t)steps * nb, 1)));
    PHX_TRY(bench_.stage_dvel.reserve(std::max<size_t>((size_t)steps * nb, 1)));
    PHX_TRY(bench_.stage_mpos.reserve(std::max<size_t>(nb, 1)));
    PHX_TRY(bench_.stage_joints.reserve(std::max<size_t>((size_t)steps * nj, 1)));
    for (int k = 0; k < steps; ++k) {
        if (nb) hipLaunchKernelGGL(k_bodies_to_view, dim3(grid_for(nb)), dim3(256), 0, stream_, static_cast<const phx_rigid_body*>(d_bodies), nb,
                                   BodyView{bench_.stage_vel.p + (size_t)k * nb, bench_.stage_dvel.p + (size_t)k * nb, bench_.stage_mpos.p});
        if (nj) PHX_HIP(hipMemcpyAsync(bench_.stage_joints.p + (size_t)k * nj, d_joints, (size_t)nj * sizeof(phx_contact_joint), hipMemcpyDeviceToDevice, stream_));
    }
    PHX_HIP(hipGetLastError());
    PHX_HIP(hipStreamSynchronize(stream_));
    bench_.staged_src_bodies = d_bodies; bench_.staged_src_joints = d_joints; bench_.staged_nb = nb; bench_.staged_nj = nj; bench_.staged_steps = steps;
    return PHX_OK;
}

int DeviceSolver::bench(const void* d_bodies, int nb, const void* d_cps, int ncp, const void* d_joints, int nj,
                        const phx_config& cfg, int warmup, int steps, phx_bench_result* out, phx_step_hook hook, void* user)
{
    PHX_REQUIRE(out && warmup >= 0 && steps >= 0 && steps <= 4096, "bad bench arguments");
    PHX_TRY(use_device(device_));
    PHX_TRY(bench_.snap_vel.reserve(std::max(nb, 1))); PHX_TRY(bench_.snap_dvel.reserve(std::max(nb, 1))); PHX_TRY(bench_.snap_mpos.reserve(std::max(nb, 1)));
    PHX_TRY(bench_.snap_joints.reserve(std::max(nj, 1)));
    std::memset(out, 0, sizeof *out);
    while ((int)bench_.events.size() < 2 * steps + 2) { hipEvent_t e; PHX_HIP(hipEventCreate(&e)); bench_.events.push_back(e); }
    // every step solves the SAME input: its own staged copy (bench_stage, made before the clock started), or — warm-up steps, or
    // nothing staged — a working copy restored from the caller's (untouched) arrays in front of the step
    const bool staged = bench_.staged_steps >= steps && steps > 0 && bench_.staged_src_bodies == d_bodies && bench_.staged_src_joints == d_joints && bench_.staged_nb == nb && bench_.staged_nj == nj;
    bench_.staged_steps = 0;                                       // (consumed: the solves overwrite the copies)
    auto one_step = [&](int k) -> int {
        BodyView b{bench_.snap_vel.p, bench_.snap_dvel.p, bench_.snap_mpos.p}; phx_contact_joint* j = bench_.snap_joints.p;
        if (staged && k >= 0) { b = BodyView{bench_.stage_vel.p + (size_t)k * nb, bench_.stage_dvel.p + (size_t)k * nb, bench_.stage_mpos.p}; j = bench_.stage_joints.p + (size_t)k * nj; }
        else {
            if (nb) hipLaunchKernelGGL(k_bodies_to_view, dim3(grid_for(nb)), dim3(256), 0, stream_, static_cast<const phx_rigid_body*>(d_bodies), nb, b);
            if (nj) PHX_HIP(hipMemcpyAsync(j, d_joints, (size_t)nj * sizeof(phx_contact_joint), hipMemcpyDeviceToDevice, stream_));
        }
        PHX_TRY(solve_resident(b, nb, d_cps, ncp, j, nj, cfg));
        bench_.last_b = b; bench_.last_j = j; bench_.last_nb = nb; bench_.last_nj = nj;
        if (xch_send_) {       // island-sharded solve: pack, the caller's all-gather (hook phase 2), unpack — all on the stream
            PHX_TRY(exchange_pack_resident(&b, j, nullptr));
            if (comm_) PHX_TRY(exchange_all_gather());      // native transport: RCCL on this stream, no callback
            else if (hook && hook(user, bench_.step_hook_step, 2)) { set_error("bench: step hook failed"); return PHX_ERR_STATE; }
            PHX_TRY(exchange_unpack_resident(b, j));
        }
        return PHX_OK;
    };
    // the hook's phase 1 fires inside solve_device, between the step's fingerprint and its sweeps
    struct HookScope {
        DeviceSolver& s;
        HookScope(DeviceSolver& s_, phx_step_hook h, void* u) : s(s_) { s.bench_.step_hook = h; s.bench_.step_hook_user = u; }
        ~HookScope() { s.bench_.step_hook = nullptr; s.bench_.step_hook_user = nullptr; }
    } scope(*this, hook, user);
    for (int i = 0; i < warmup; ++i) {
        bench_.step_hook_step = i - warmup;
        PHX_TRY(one_step(-1));
        if (hook && hook(user, i - warmup, 0)) { set_error("bench: step hook failed"); return PHX_ERR_STATE; }
        PHX_TRY(synchronize());
    }
    if (!steps) { if (hook && warmup && hook(user, 0, 1)) { set_error("bench: step hook failed"); return PHX_ERR_STATE; } return PHX_OK; }
    // timed steps are queued back to back; the device never waits for the host between them
    // (the handle's own sweep events are put back — and the bracketing returned to whole solves — however this function leaves)
    struct SweepEvents {
        DeviceSolver& s; hipEvent_t b, e;
        explicit SweepEvents(DeviceSolver& s_) : s(s_), b(s_.ev_sweep_begin_), e(s_.ev_sweep_end_) { s.time_sweeps_ = true; }
        ~SweepEvents() { s.ev_sweep_begin_ = b; s.ev_sweep_end_ = e; s.time_sweeps_ = false; s.timed_sweeps_ = false; }
    } sweep_events(*this);
    int st = PHX_OK;
    struct InLoop { DeviceSolver& s; explicit InLoop(DeviceSolver& s_) : s(s_) { s.bench_.in_loop = true; } ~InLoop() { s.bench_.in_loop = false; } } in_loop(*this);
    struct Trusted { DeviceSolver& s; Trusted(DeviceSolver& s_, bool on) : s(s_) { s.bench_.trusted = on; } ~Trusted() { s.bench_.trusted = false; } } trusted(*this, staged && reuse_schedule_ && opt_.speculate);
    PHX_HIP(hipEventRecord(bench_.events[2 * steps], stream_));
    // HIP events bracket the sweep launches of every 4th step only: an event record is a barrier packet of its own (~3 us of idle
    // queue), and bracketing every step's sweeps cost 6.4 us per step — 7 % of the value being measured (tools/exp_events.py)
    // (PHX_BENCH_BRACKET_STRIDE=n, measurement of the measurement: 1 = every step, 0 = no events at all — tools/exp_events.py)
    const char* bs_env = getenv("PHX_BENCH_BRACKET_STRIDE");
    const int bracket_stride = bs_env ? (atoi(bs_env) > 0 ? atoi(bs_env) : steps + 1) : (steps >= 8 ? 4 : 1);
    const bool bracket_any = !(bs_env && atoi(bs_env) <= 0);
    for (int i = 0; i < steps && st == PHX_OK; ++i) {
        time_sweeps_ = bracket_any && i % bracket_stride == 0;
        if (time_sweeps_) { ev_sweep_begin_ = bench_.events[2 * i]; ev_sweep_end_ = bench_.events[2 * i + 1]; }      // (else: still the last bracketed step's pair — a
                                                                                                                  //  solve settled later reads the pair it recorded)
        bench_.step_hook_step = i;
        st = one_step(i);
        if (st == PHX_OK && hook && hook(user, i, 0)) { set_error("bench: step hook failed"); st = PHX_ERR_STATE; }
    }
    if (st == PHX_OK && hook && hook(user, steps, 1)) { set_error("bench: step hook failed"); st = PHX_ERR_STATE; }      // drain the last exchange
    PHX_TRY(st);
    PHX_HIP(hipEventRecord(bench_.events[2 * steps + 1], stream_));
    const unsigned replays = replays_;
    if (bench_.trusted && !pending_.active) {       // staged copies: the last step's fingerprint comes back with its counters
        unsigned long long fp = 0;
        PHX_TRY(collect_stats(&fp, hash_.p + hash_slot_));
        if (fp != gate_expected_) { set_error("bench: a staged copy of the input did not match the schedule's topology"); return PHX_ERR_STATE; }
    } else PHX_TRY(synchronize());
    if (replays_ != replays && reuse_schedule_) { set_error("bench: topology changed during the timed region"); return PHX_ERR_STATE; }
    float ms = 0.f;
    PHX_HIP(hipEventSynchronize(bench_.events[2 * steps + 1]));      // (reached long ago — the mailbox post ran behind it — but the runtime may not have looked yet)
    PHX_HIP(hipEventElapsedTime(&ms, bench_.events[2 * steps], bench_.events[2 * steps + 1]));
    out->total_ms = ms;
    for (int i = 0; bracket_any && i < steps; i += bracket_stride) {
        PHX_HIP(hipEventElapsedTime(&ms, bench_.events[2 * i], bench_.events[2 * i + 1]));
        out->impulse_kernel_ms += ms;
    }
    // identical input every step => identical counters every step
    out->impulse_launches = (long long)sweep_launches_ * steps;
    out->bracketed_launches = bracket_any ? (long long)sweep_launches_ * ((steps + bracket_stride - 1) / bracket_stride) : 0;
    out->impulse_iterations = (long long)stats_.impulse_iterations * steps;
    out->joint_visits = stats_.joint_visits * steps;
    return PHX_OK;
}

// position-sensitive sum of the result words (order of the threads does not matter: a sum of mixed (index, bits) terms)
static __global__ void __launch_bounds__(256) k_result_checksum(BodyView b, int nb, const phx_contact_joint* __restrict__ joints, int nj, unsigned long long* out)
{
    unsigned long long h = 0;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nb; i += gridDim.x * blockDim.x) {
        const float4 v = b.vel[i], d = b.dvel[i];
        const unsigned w[6] = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(d.x), __float_as_uint(d.y), __float_as_uint(d.z)};
        for (int k = 0; k < 6; ++k) h += mix64(((unsigned long long)(6u * (unsigned)i + k + 1u) << 32) | w[k]);
    }
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nj; i += gridDim.x * blockDim.x) {
        const phx_contact_joint j = joints[i];
        h += mix64(0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1) + __float_as_uint(j.normal_accumulated_impulse));
        h += mix64(0xC2B2AE3D27D4EB4Full * (unsigned long long)(i + 1) + __float_as_uint(j.friction_accumulated_impulse));
    }
    for (int off = 32; off > 0; off >>= 1) h += __shfl_down(h, off);
    if ((threadIdx.x & 63) == 0 && h) atomicAdd(out, h);
}

int DeviceSolver::bench_checksum(unsigned long long* out)
{
    PHX_REQUIRE(out, "null output");
    PHX_TRY(use_device(device_));
    PHX_TRY(synchronize());
    if (!bench_.last_j && !bench_.last_b.vel) { set_error("bench_checksum: no bench step has run"); return PHX_ERR_STATE; }
    unsigned long long* d = nullptr;
    PHX_HIP(hipMalloc(reinterpret_cast<void**>(&d), sizeof *d));
    hipError_t e = hipMemsetAsync(d, 0, sizeof *d, stream_);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_result_checksum, dim3(512), dim3(256), 0, stream_, bench_.last_b, bench_.last_nb, bench_.last_j, bench_.last_nj, d);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d, sizeof *out, hipMemcpyDeviceToHost, stream_);
    if (e == hipSuccess) e = hipStreamSynchronize(stream_);
    (void)hipFree(d);
    if (e != hipSuccess) { set_error("bench_checksum: %s", hipGetErrorString(e)); return PHX_ERR_HIP; }
    return PHX_OK;
}

} // namespace phx
