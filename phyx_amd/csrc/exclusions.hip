// exclusions.hip — the device side of a World's collision exclusions (exclusions.h): the upload of the list, the table of its keys
// (filled by the broadphase's own insert kernel: pair_table_fill), the per-body words, and the list's way through a removal of bodies.
#include "exclusions.h"
#include "broadphase.h"
#include "pair_set.h"

#include <algorithm>
#include <iterator>

namespace phx {

static inline int xgrid(int n) { return std::max(1, std::min(div_up(n, 256), 2048)); }

// member[body] = 1 for both bodies of every pair (the words were cleared; every writer of a word stores the same value)
static __global__ void __launch_bounds__(256) k_exclusion_members(const uint2* __restrict__ pairs, int n, unsigned* __restrict__ member)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint2 p = pairs[i];
        member[p.x] = 1u;
        member[p.y] = 1u;
    }
}

// moved[i] = the pair's bodies through new[] (-1: removed)
static __global__ void __launch_bounds__(256) k_exclusion_remap(const uint2* __restrict__ pairs, int n, const int* __restrict__ remap, int2* __restrict__ moved)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint2 p = pairs[i];
        moved[i] = make_int2(remap[p.x], remap[p.y]);
    }
}

void ExclusionSet::add(const std::vector<unsigned long long>& keys)
{
    std::vector<unsigned long long> sorted(keys), merged;
    std::sort(sorted.begin(), sorted.end());
    std::set_union(keys_.begin(), keys_.end(), sorted.begin(), sorted.end(), std::back_inserter(merged));
    if (merged.size() == keys_.size()) return;                              // every pair was present: nothing changes
    keys_.swap(merged);
    stale_ = true;
}

void ExclusionSet::remove(const std::vector<unsigned long long>& keys)
{
    std::vector<unsigned long long> sorted(keys), rest;
    std::sort(sorted.begin(), sorted.end());
    std::set_difference(keys_.begin(), keys_.end(), sorted.begin(), sorted.end(), std::back_inserter(rest));
    if (rest.size() == keys_.size()) return;                                // every pair was absent
    keys_.swap(rest);
    stale_ = true;
}

void ExclusionSet::clear()
{
    if (keys_.empty()) return;
    keys_.clear();
    stale_ = true;
}

int ExclusionSet::upload_pairs(hipStream_t stream)
{
    const size_t n = keys_.size();
    staged_.resize(n);
    for (size_t i = 0; i < n; ++i) staged_[i] = make_uint2((unsigned)(keys_[i] >> 32), (unsigned)keys_[i]);
    PHX_TRY(d_pairs_.reserve(n));
    PHX_HIP(hipMemcpyAsync(d_pairs_.p, staged_.data(), n * sizeof(uint2), hipMemcpyHostToDevice, stream));
    PHX_HIP(hipStreamSynchronize(stream));                                  // (`staged_` is pageable and reused)
    return PHX_OK;
}

int ExclusionSet::sync(int nb, hipStream_t stream)
{
    if (keys_.empty()) { stale_ = false; member_n_ = 0; return PHX_OK; }    // (an empty set has no device side: the plain sweep)
    if (!stale_ && member_n_ == nb) return PHX_OK;
    if (!stale_ && member_n_ && member_n_ < nb) {                           // bodies were appended: they are in no pair
        PHX_TRY(member_.reserve_keep((size_t)nb, (size_t)member_n_, stream));
        PHX_HIP(hipMemsetAsync(member_.p + member_n_, 0, (size_t)(nb - member_n_) * sizeof(unsigned), stream));
        member_n_ = nb;
        view_.member = member_.p;
        return PHX_OK;
    }
    const int n = count();
    PHX_TRY(upload_pairs(stream));
    unsigned cap = 64u;
    while (cap < 2u * (unsigned)n) cap <<= 1;                               // at most half full
    PHX_TRY(table_.reserve(cap));
    PHX_TRY(pair_table_fill(table_.p, cap, d_pairs_.p, n, stream));
    PHX_TRY(member_.reserve((size_t)std::max(nb, 1)));
    PHX_HIP(hipMemsetAsync(member_.p, 0, (size_t)std::max(nb, 1) * sizeof(unsigned), stream));
    hipLaunchKernelGGL(k_exclusion_members, dim3(xgrid(n)), dim3(256), 0, stream, (const uint2*)d_pairs_.p, n, member_.p);
    PHX_HIP(hipGetLastError());
    member_n_ = nb;
    stale_ = false;
    view_ = ExclusionView{table_.p, cap - 1u, member_.p};
    return PHX_OK;
}

int ExclusionSet::bodies_removed(const int* d_remap, Readback& rb, hipStream_t stream)
{
    const int n = count();
    if (!n) return PHX_OK;
    if (stale_) PHX_TRY(upload_pairs(stream));
    PHX_TRY(d_moved_.reserve((size_t)n));
    hipLaunchKernelGGL(k_exclusion_remap, dim3(xgrid(n)), dim3(256), 0, stream, (const uint2*)d_pairs_.p, n, d_remap, d_moved_.p);
    PHX_HIP(hipGetLastError());
    std::vector<int2> moved((size_t)n);
    PHX_TRY(rb.add(moved.data(), d_moved_.p, (size_t)n * sizeof(int2), stream));
    PHX_TRY(rb.wait(stream));
    keys_.clear();
    for (const int2& m : moved)
        if (m.x >= 0 && m.y >= 0) keys_.push_back(ps_unordered_key((unsigned)m.x, (unsigned)m.y));
    stale_ = true;
    return PHX_OK;
}

int ExclusionSet::adopt_device(const uint2* d_src, int count, hipStream_t stream)
{
    keys_.clear();
    stale_ = true;
    if (!count) return PHX_OK;
    staged_.resize((size_t)count);
    PHX_HIP(hipMemcpyAsync(staged_.data(), d_src, (size_t)count * sizeof(uint2), hipMemcpyDeviceToHost, stream));
    PHX_HIP(hipStreamSynchronize(stream));
    for (const uint2& p : staged_) keys_.push_back(((unsigned long long)p.x << 32) | p.y);
    return PHX_OK;
}

} // namespace phx
