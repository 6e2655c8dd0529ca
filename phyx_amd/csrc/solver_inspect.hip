// solver_inspect.hip — DeviceSolver: what a caller asks for after the fact — statistics, the schedule, the groups and their lanes, the
// refreshed constants of a joint, the island kernel's traces.  Everything here settles the solve first; nothing here is run by a step.
#include "solver.h"
#include "island_view.h"

#include <algorithm>

namespace phx {

// The tables of the last speculative build, on demand (collect_stats): what a build with a host round trip would have left in
// sched_ and stats_.  Callers have settled the solve (synchronize()), so nothing queued since can have overwritten them.
int DeviceSolver::fetch_build_tables()
{
    if (!tables_pending_) return PHX_OK;
    PHX_TRY(use_device(device_));
    const int nbins = tables_bins_, ncomp = tables_comps_;
    std::vector<int> goff((size_t)nbins + 1, 0), ncol((size_t)std::max(nbins, 1), 0);
    std::vector<unsigned> comp_size((size_t)std::max(ncomp, 1), 0u);
    PHX_TRY(rb_.add(goff.data(), bld_.bin_tables_s[tables_set_].p + 2 * BINC_MAX, goff.size() * sizeof(int), stream_));
    if (nbins) PHX_TRY(rb_.add(ncol.data(), isl_.ncol.p, (size_t)nbins * sizeof(int), stream_));
    if (ncomp) PHX_TRY(rb_.add(comp_size.data(), bld_.comp_size_s[tables_set_].p, (size_t)ncomp * sizeof(unsigned), stream_));
    PHX_TRY(rb_.wait(stream_));
    tables_pending_ = false;
    sched_.group_offsets.assign(goff.begin(), goff.end());
    const IslandNumbers isl = coalesce_islands(comp_size.data(), ncomp);      // (as the builder's long way computes them)
    sched_.island_count = isl.count; sched_.island_max_size = isl.max_size;
    sched_.lds_colours = 0;
    for (int g = 0; g < nbins; ++g) sched_.lds_colours += ncol[(size_t)g];
    publish_schedule_stats(last_island_mode_, nj_);
    return PHX_OK;
}

// The LDS groups of a device-built schedule live in HBM; the query API (and the parity tests that replay the
// schedule through the oracle) need them on the host.
int DeviceSolver::materialise_schedule()
{
    PHX_TRY(fetch_build_tables());
    if (sched_.lds_on_host) return PHX_OK;
    const int lg = sched_.lds_groups;
    const int lds_slots = lg ? sched_.group_offsets[lg] : 0;
    std::vector<int> order(std::max(nj_, 1)), ncol(std::max(lg, 1));
    std::vector<unsigned char> colour(std::max(lds_slots, 1));
    PHX_TRY(use_device(device_));
    if (nj_) PHX_HIP(hipMemcpy(order.data(), hbm_.order.p, (size_t)nj_ * sizeof(int), hipMemcpyDeviceToHost));
    if (lds_slots) {
        PHX_HIP(hipMemcpy(colour.data(), isl_.slot_colour.p, (size_t)lds_slots, hipMemcpyDeviceToHost));
        PHX_HIP(hipMemcpy(ncol.data(), isl_.ncol.p, (size_t)lg * sizeof(int), hipMemcpyDeviceToHost));
    }
    sched_.order.assign(order.begin(), order.begin() + nj_);
    sched_.colour_offsets.assign(1, 0);
    sched_.group_first_colour.assign(1, 0);
    for (int g = 0; g < lg; ++g) {
        std::vector<int> count(ncol[g], 0);
        for (int s = sched_.group_offsets[g]; s < sched_.group_offsets[g + 1]; ++s) count[colour[s]]++;
        int at = sched_.group_offsets[g];
        for (int c = 0; c < ncol[g]; ++c) { at += count[c]; sched_.colour_offsets.push_back(at); }
        sched_.group_first_colour.push_back((int)sched_.colour_offsets.size() - 1);
    }
    if (sched_.has_hbm_group()) {
        for (size_t c = 1; c < sched_.hbm_colour_offsets.size(); ++c) sched_.colour_offsets.push_back(sched_.hbm_colour_offsets[c]);
        sched_.group_first_colour.push_back((int)sched_.colour_offsets.size() - 1);
    }
    sched_.lds_on_host = true;
    return PHX_OK;
}

int DeviceSolver::get_stats(phx_solve_stats* out)
{
    PHX_REQUIRE(out, "null out");
    if (!have_solve_) { set_error("no solve has run yet"); return PHX_ERR_STATE; }
    PHX_TRY(synchronize());
    PHX_TRY(fetch_build_tables());
    *out = stats_;
    return PHX_OK;
}

int DeviceSolver::get_schedule(int* order, int order_cap, int* offsets, int offsets_cap, int* ncolours)
{
    if (!sched_.valid) { set_error("no solve has run yet"); return PHX_ERR_STATE; }
    PHX_TRY(synchronize());                            // (an unverified device build is settled first)
    PHX_TRY(materialise_schedule());
    const int ncol = sched_.ncolours();
    if (ncolours) *ncolours = ncol;
    if ((order && order_cap < nj_) || (offsets && offsets_cap < ncol + 1)) { set_error("schedule buffers too small"); return PHX_ERR_CAPACITY; }
    if (order) std::copy(sched_.order.begin(), sched_.order.end(), order);
    if (offsets) std::copy(sched_.colour_offsets.begin(), sched_.colour_offsets.end(), offsets);
    return PHX_OK;
}

// The island kernel's trace (diagnostics: tools/island_trace.py; laid out by enqueue_sweeps): 8 words of phase stamps per group, then 8
// words per wave — 16 waves at most — of every group, then ISL_PHASE_WORDS per group.  One section of it, `skip` words per group into the
// buffer and `words` per group long (per_wave: per wave of the group's shape): settles the solve, reports the group and wave counts and,
// if `out`, checks that the trace is on and that cap_words suffice, and copies the section.
int DeviceSolver::copy_trace(unsigned long long* out, long long cap_words, int skip, int words, bool per_wave, const char* too_small, int* groups, int* waves_per_group)
{
    PHX_TRY(synchronize());
    const int lg = sched_.valid ? sched_.lds_groups : 0;
    const int wpg = sched_.lds_lanes > ISL_T ? ISL_T_BIG / 64 : ISL_T / 64;
    if (groups) *groups = lg;
    if (waves_per_group) *waves_per_group = wpg;
    if (!out) return PHX_OK;
    const size_t section = (size_t)lg * words * (per_wave ? wpg : 1);
    if (!trace_islands_ || !isl_.trace.p) { set_error("island trace is off (phx_solver_set_trace)"); return PHX_ERR_STATE; }
    if (cap_words < (long long)section) { set_error("%s", too_small); return PHX_ERR_CAPACITY; }
    if (lg) PHX_HIP(hipMemcpy(out, isl_.trace.p + (size_t)lg * skip, section * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return PHX_OK;
}

int DeviceSolver::get_island_trace(unsigned long long* out, int cap_groups, int* groups)
{
    return copy_trace(out, 8ll * cap_groups, 0, 8, false, "island trace buffer too small", groups, nullptr);
}

int DeviceSolver::get_phase_trace(unsigned long long* out, int cap_words, int* words_per_group)
{
    if (words_per_group) *words_per_group = ISL_PHASE_WORDS;
    return copy_trace(out, cap_words, 8 + 128, ISL_PHASE_WORDS, false, "phase trace buffer too small", nullptr, nullptr);
}

int DeviceSolver::get_wave_trace(unsigned long long* out, int cap_words, int* waves_per_group)
{
    return copy_trace(out, cap_words, 8, 8, true, "wave trace buffer too small", nullptr, waves_per_group);
}

int DeviceSolver::get_groups(int* offsets, int cap, int* count, int* lds_count)
{
    if (!sched_.valid) { set_error("no solve has run yet"); return PHX_ERR_STATE; }
    PHX_TRY(synchronize());
    PHX_TRY(materialise_schedule());
    if (count) *count = sched_.ngroups();
    if (lds_count) *lds_count = sched_.lds_groups;
    if (offsets) {
        if (cap < (int)sched_.group_offsets.size()) { set_error("group_offsets too small"); return PHX_ERR_CAPACITY; }
        std::copy(sched_.group_offsets.begin(), sched_.group_offsets.end(), offsets);
    }
    return PHX_OK;
}

int DeviceSolver::get_lanes(int* leader_slot, int* lane, int cap, int* count)
{
    if (!sched_.valid) { set_error("no solve has run yet"); return PHX_ERR_STATE; }
    PHX_TRY(synchronize());
    PHX_TRY(materialise_schedule());
    const int lg = sched_.lds_groups, lanes = sched_.lds_lanes;
    std::vector<int4> recs(2 * (size_t)std::max(lg, 1) * std::max(lanes, 1));
    PHX_TRY(use_device(device_));
    if (lg) PHX_HIP(hipMemcpy(recs.data(), isl_.unit_recs.p, 2 * (size_t)lg * lanes * sizeof(int4), hipMemcpyDeviceToHost));
    int n = 0;
    for (int g = 0; g < lg; ++g)
        for (int l = 0; l < lanes; ++l) {
            const int4 a = recs[2 * ((size_t)g * lanes + l)], b = recs[2 * ((size_t)g * lanes + l) + 1];
            if (a.x < 0) continue;                                      // nobody's lane
            if (leader_slot && lane) {
                if (n >= cap) { set_error("lane arrays too small"); return PHX_ERR_CAPACITY; }
                leader_slot[n] = b.z; lane[n] = l;
            }
            ++n;
        }
    if (count) *count = n;
    return PHX_OK;
}

int DeviceSolver::get_refreshed(int joint, float out[30])
{
    if (!have_solve_) { set_error("no solve has run yet"); return PHX_ERR_STATE; }
    PHX_REQUIRE(joint >= 0 && joint < nj_ && out, "joint index out of range");
    PHX_TRY(synchronize());
    PHX_TRY(materialise_schedule());
    const int slot = (int)(std::find(sched_.order.begin(), sched_.order.end(), joint) - sched_.order.begin());
    if (sched_.lds_groups && slot < sched_.group_offsets[sched_.lds_groups]) {
        set_error("joint %d was solved by the island kernel, whose refreshed constants live only in registers; query it under island mode Single", joint);
        return PHX_ERR_STATE;
    }
    float4 a, f, c; int4 k; float2 acc, d;
    PHX_HIP(hipMemcpy(&a, hbm_.q0.p + slot, sizeof a, hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(&f, hbm_.q1.p + slot, sizeof f, hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(&c, hbm_.q2.p + slot, sizeof c, hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(&k, hbm_.q3.p + slot, sizeof k, hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(&acc, hbm_.acc.p + slot, sizeof acc, hipMemcpyDeviceToHost));
    PHX_HIP(hipMemcpy(&d, hbm_.dd.p + slot, sizeof d, hipMemcpyDeviceToHost));
    float ii2; std::memcpy(&ii2, &k.x, 4);
    const float im1 = c.y, ii1 = c.z, im2 = c.w;
    const float nx = a.x, ny = a.y, tx = -ny, ty = nx;
    // expand to ContactLimiterPacked order (ref: Solver.h:7-24): projectors, angular, compMass, compInvMass
    float* o = out;
    *o++ = nx; *o++ = ny; *o++ = -nx; *o++ = -ny; *o++ = a.z; *o++ = a.w;
    *o++ = nx * im1; *o++ = ny * im1; *o++ = (-nx) * im2; *o++ = (-ny) * im2; *o++ = a.z * ii1; *o++ = a.w * ii2; *o++ = c.x;
    *o++ = 0.f; *o++ = f.w; *o++ = d.x; *o++ = d.y;
    *o++ = tx; *o++ = ty; *o++ = -tx; *o++ = -ty; *o++ = f.x; *o++ = f.y;
    *o++ = tx * im1; *o++ = ty * im1; *o++ = (-tx) * im2; *o++ = (-ty) * im2; *o++ = f.x * ii1; *o++ = f.y * ii2; *o++ = f.z;
    (void)acc;
    return PHX_OK;
}

} // namespace phx
