// snapshot_kernels.h — the two kernels of phx_world_save / phx_world_load (include/phyx_amd.h SNAPSHOTS, snapshot.h).
//
// A save or a load moves eight arrays.  One launch does it: the grid walks the 16-byte granules of seven of them, which a by-value
// table names (as MailArgs names the items of a post), one array after the other, and then the bodies (one 128-byte record each, the
// only array that is not a plain copy).  Every walk is grid-strided, so consecutive lanes move consecutive granules.
// An array whose size is no multiple of 16 bytes (20-byte joints, 8-byte materials, 4-byte flags, 8-byte baseline keys) ends in a TAIL of
// one to three 4-byte words: nothing is read or written past the end of a world's array, and the snapshot's copy of the tail is
// padded with zeros to the granule (snapshot_blob.h: sections start at multiples of 16 and the bytes between them are zero).
#pragma once

#include "body_view.h"
#include "snapshot_blob.h"

namespace phx {

constexpr int SNAP_COPIES = SNAP_SECTIONS - 1;      // every section but the bodies
struct SnapCopy {
    const uint4* src;
    uint4* dst;
    unsigned long long granules;      // whole 16-byte granules
    unsigned tail_words;              // then 0 .. 3 words of 4 bytes
};
struct SnapTable {
    SnapCopy seg[SNAP_COPIES];        // in snapshot_blob.h's order: seg[k] is section k + 1 (seg[0]: the manifolds)
    int nb;
};

typedef unsigned u4v __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void store_nt(uint4* p, const uint4& v)
{
    u4v q; q.x = v.x; q.y = v.y; q.z = v.z; q.w = v.w;
    __builtin_nontemporal_store(q, reinterpret_cast<u4v*>(p));
}

// The plain copies, one after the other, each walked by the whole grid (the table entry is uniform: it stays in scalar registers).
// SAVE: the destination is the snapshot (non-temporal stores: nobody reads it before the kernel ends; a tail is padded to its
// granule).  Otherwise the destination is a world's array (plain stores, a tail word by word), and `pairs` receives (body1, body2) of
// every manifold: the broadphase's new pair set (DeviceBroadphase::reset_pairs_device).
template <bool SAVE>
__device__ __forceinline__ void snap_copies(const SnapTable& t, uint2* __restrict__ pairs)
{
    const unsigned long long lane = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x, lanes = (unsigned long long)gridDim.x * blockDim.x;
    for (int s = 0; s < SNAP_COPIES; ++s) {
        const uint4* __restrict__ src = t.seg[s].src;
        uint4* __restrict__ dst = t.seg[s].dst;
        const unsigned long long granules = t.seg[s].granules;
        const unsigned tail = t.seg[s].tail_words;
        for (unsigned long long k = lane; k < granules; k += lanes) {
            const uint4 v = src[k];
            if (SAVE) store_nt(dst + k, v);
            else {
                dst[k] = v;
                if (s == 0) pairs[k] = make_uint2(v.x, v.y);      // phx_manifold {body1, body2, point_count, point_index}
            }
        }
        if (tail && lane == 0) {
            const unsigned* sw = reinterpret_cast<const unsigned*>(src + granules);
            if (SAVE) {
                uint4 v = make_uint4(sw[0], 0u, 0u, 0u);
                if (tail > 1) v.y = sw[1];
                if (tail > 2) v.z = sw[2];
                store_nt(dst + granules, v);
            } else {
                unsigned* dw = reinterpret_cast<unsigned*>(dst + granules);
                dw[0] = sw[0];
                if (tail > 1) dw[1] = sw[1];
                if (tail > 2) dw[2] = sw[2];
            }
        }
    }
}

// s := the world.  Body i's record as phx_world_get_bodies would return it: `refresh` (the records are stale) brings it up to date
// from the resident arrays first (world_record), as the getter and k_remove_bodies do.  The world is only read.
static __global__ void __launch_bounds__(256) k_snapshot_save(SnapTable t, const phx_rigid_body* __restrict__ records, WorldBodies w, int refresh,
                                                              float4* __restrict__ out_records)
{
    static_assert(sizeof(phx_rigid_body) == 8 * sizeof(float4), "a record is one 128-byte line");
    snap_copies<true>(t, nullptr);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.nb; i += gridDim.x * blockDim.x) {
        const float4* src = reinterpret_cast<const float4*>(records) + 8 * (size_t)i;
        float4 line[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) line[k] = src[k];
        if (refresh) {
            phx_rigid_body b;
            __builtin_memcpy(&b, line, sizeof b);
            world_record(w, i, b);
            __builtin_memcpy(line, &b, sizeof b);
        }
        float4* dst = out_records + 8 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 8; ++k) store_nt(dst + k, line[k].x, line[k].y, line[k].z, line[k].w);
    }
}

// the world := s.  The saved record becomes the world's record, and the six resident arrays (and, where the snapshot carries pending
// accelerations, `accel`) are made from it by the upload's own conversion (record_to_world): phx_world_set_state's result by construction.
static __global__ void __launch_bounds__(256) k_snapshot_load(SnapTable t, const float4* __restrict__ saved_records, phx_rigid_body* __restrict__ records, WorldBodies w,
                                                              float4* __restrict__ accel, uint2* __restrict__ pairs)
{
    snap_copies<false>(t, pairs);
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < t.nb; i += gridDim.x * blockDim.x) {
        const float4* src = saved_records + 8 * (size_t)i;
        float4 line[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) line[k] = src[k];
        float4* dst = reinterpret_cast<float4*>(records) + 8 * (size_t)i;
#pragma unroll
        for (int k = 0; k < 8; ++k) dst[k] = line[k];
        phx_rigid_body b;
        __builtin_memcpy(&b, line, sizeof b);
        record_to_world(b, w, i);
        if (accel) accel[i] = make_float4(b.acceleration.x, b.acceleration.y, b.angular_acceleration, 0.f);
    }
}

} // namespace phx
