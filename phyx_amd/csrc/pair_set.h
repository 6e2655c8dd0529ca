// pair_set.h — the open-addressing table of 64-bit body-pair keys, as the device reads it: the broadphase's persistent pair set
// (broadphase_kernels.h, which also owns the kernels that write one) and the collision exclusions' table (exclusions.h) are both one.
// Linear probing from ps_hash(key) & mask; a table holds PS_EMPTY wherever nothing was ever stored, so a probe ends there.
#pragma once

#include "common.h"

namespace phx {

constexpr unsigned long long PS_EMPTY = 0xFFFFFFFFFFFFFFFFull;
constexpr unsigned long long PS_TOMB = 0xFFFFFFFFFFFFFFFEull;

__device__ __forceinline__ unsigned ps_hash(unsigned long long k)
{
    // same mixing idea as the reference's pair hash (ref: Collider.h:10-18), finished with a multiply
    const unsigned lb = (unsigned)(k >> 32), rb = (unsigned)k;
    return (lb ^ (rb + 0x9e3779b9u + (lb << 6) + (lb >> 2))) * 0x9E3779B1u;
}

__device__ __forceinline__ bool ps_contains(const unsigned long long* __restrict__ table, unsigned mask, unsigned long long k)
{
    unsigned p = ps_hash(k) & mask;
    for (;;) {
        const unsigned long long s = table[p];
        if (s == k) return true;
        if (s == PS_EMPTY) return false;
        p = (p + 1) & mask;
    }
}

// the pair set's own key: the ORDERED pair, as the sweep met it (a: the row's body, b: the candidate's)
__host__ __device__ __forceinline__ unsigned long long ps_ordered_key(unsigned a, unsigned b)
{
    return ((unsigned long long)a << 32) | b;
}

// the key of an UNORDERED pair: {min, max} (an exclusion does not know which of its two bodies the sweep meets first)
__host__ __device__ __forceinline__ unsigned long long ps_unordered_key(unsigned a, unsigned b)
{
    return a < b ? ps_ordered_key(a, b) : ps_ordered_key(b, a);
}

} // namespace phx
