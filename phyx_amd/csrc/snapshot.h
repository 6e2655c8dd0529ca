// snapshot.h — a saved world in HBM (include/phyx_amd.h SNAPSHOTS): one device allocation in the blob's own layout
// (snapshot_blob.h, bytes [128, total)), filled and emptied by the two kernels of snapshot_kernels.h on the stream of the world
// that saves or loads.  The World (world_state.hip) hands out its arrays as a SnapshotWorld; everything else lives here: the layout, the
// growth of the allocation, and the two events that order a save by one world against a load by another without a host wait.
#pragma once

#include <tuple>

#include "body_view.h"
#include "snapshot_blob.h"

namespace phx {

// a world's arrays as a save reads them / a load writes them (the load's buffers hold at least `counts` elements each)
struct SnapshotWorld {
    phx_rigid_body* records;
    WorldBodies resident;
    bool records_stale;                  // save: the records must be refreshed from the resident arrays on the way
    float4* accel;                       // the pending accelerations' own array (load: null unless the snapshot carries some)
    phx_manifold* manifolds;
    phx_contact_point* cps;
    phx_contact_joint* joints;
    uint4* filters; float2* materials; uint32_t* flags;      // a column the counts' bits do not name is not looked at
    unsigned long long* baseline;
    uint2* pairs;                        // load: receives the manifolds' body pairs
    SnapCounts counts;                   // save: the world's
    bool accel_pending;                  // save: some record may carry an acceleration
};

class Snapshot {
public:
    explicit Snapshot(int device) : device_(device) {}
    ~Snapshot();
    Snapshot(const Snapshot&) = delete;
    Snapshot& operator=(const Snapshot&) = delete;
    int init();
    int device() const { return device_; }
    bool filled() const { return filled_; }
    const SnapCounts& counts() const { return counts_; }
    bool accel_pending() const { return accel_pending_; }

    int save(const SnapshotWorld& w, hipStream_t stream);      // queued on `stream` behind the loads that still read the old contents
    int load(const SnapshotWorld& w, hipStream_t stream);      // queued on `stream` behind the save that wrote the contents
    // the world's pins (include/phyx_amd.h PINS) ride beside the blob's layout, which holds none: room first (nothing changes if that
    // fails), then a device copy queued behind the save, in front of the event the loads wait for
    // (a save that fails afterwards leaves the old ones whole).  The links (LINKS) ride the same way.
    // The angles (ANGLES) are the third rider, the sliders (SLIDERS) the fourth: `P` is any of the four records, and the caller
    // goes through the kinds (PinSet::each_list).  A list's break limits (BREAKS) ride beside its records, where it has a column
    // (`limited`, d_limits non-null); a list without one allocates and copies what it did before there were limits.
    template <class P> int reserve_units(int n, bool limited, hipStream_t stream) { return riders<P>().reserve(n, limited, stream); }
    template <class P> int save_units(const P* d_src, const float* d_limits, int count, hipStream_t stream)
    {
        riders<P>().count = count;
        riders<P>().limited = count && d_limits;
        if (!count) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(riders<P>().buf.p, d_src, (size_t)count * sizeof(P), hipMemcpyDeviceToDevice, stream));
        if (d_limits) PHX_HIP(hipMemcpyAsync(riders<P>().limits.p, d_limits, (size_t)count * sizeof(float), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(saved_, stream));                            // (the event moves behind the copy)
        return PHX_OK;
    }
    template <class P> const P* units() const { return std::get<Riders<P>>(riders_).buf.p; }
    template <class P> const float* unit_limits() const { const Riders<P>& r = std::get<Riders<P>>(riders_); return r.limited ? r.limits.p : nullptr; }
    template <class P> int unit_count() const { return std::get<Riders<P>>(riders_).count; }
    // the collision exclusions (COLLISION EXCLUSIONS) ride the same way: the sorted {lo, hi} list as the world's device side holds it
    int reserve_exclusions(int n, hipStream_t stream) { return n ? exclusions_.reserve_keep((size_t)n, (size_t)exclusion_count_, stream) : PHX_OK; }
    int save_exclusions(const uint2* d_src, int count, hipStream_t stream)
    {
        exclusion_count_ = count;
        if (!count) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(exclusions_.p, d_src, (size_t)count * sizeof(uint2), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(saved_, stream));                            // (the event moves behind the copy)
        return PHX_OK;
    }
    const uint2* exclusions() const { return exclusions_.p; }
    int exclusion_count() const { return exclusion_count_; }
    // the shapes' kinds (SHAPES) ride the same way: one word per body of a world whose shape column was active, none otherwise
    int reserve_shapes(int n, hipStream_t stream) { return n ? shapes_.reserve_keep((size_t)n, (size_t)shape_count_, stream) : PHX_OK; }
    // (`capsules`: the world's "a capsule was named" bit, which a load hands to the loading world)
    int save_shapes(const uint32_t* d_src, int count, bool capsules, hipStream_t stream)
    {
        shape_count_ = count; shape_capsules_ = count && capsules;
        if (!count) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(shapes_.p, d_src, (size_t)count * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(saved_, stream));                            // (the event moves behind the copy)
        return PHX_OK;
    }
    int load_shapes(uint32_t* d_dst, hipStream_t stream)                    // (queued behind Snapshot::load on the same stream)
    {
        if (!shape_count_) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(d_dst, shapes_.p, (size_t)shape_count_ * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(loaded_, stream));                           // (the next save into this snapshot waits for this copy too)
        return PHX_OK;
    }
    int shape_count() const { return shape_count_; }
    // the polygon records (POLYGONS) ride the same way: 33 words per body of a world whose polygon column was active, with its
    // "a polygon was named" bit
    static constexpr size_t POLY_WORDS = 33;
    int reserve_polygons(int n, hipStream_t stream) { return n ? polygons_.reserve_keep((size_t)n * POLY_WORDS, (size_t)polygon_count_ * POLY_WORDS, stream) : PHX_OK; }
    int save_polygons(const void* d_src, int count, bool named, hipStream_t stream)
    {
        polygon_count_ = count; polygons_named_ = count && named;
        if (!count) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(polygons_.p, d_src, (size_t)count * POLY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(saved_, stream));                            // (the event moves behind the copy)
        return PHX_OK;
    }
    int load_polygons(void* d_dst, hipStream_t stream)                      // (queued behind Snapshot::load on the same stream)
    {
        if (!polygon_count_) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(d_dst, polygons_.p, (size_t)polygon_count_ * POLY_WORDS * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(loaded_, stream));
        return PHX_OK;
    }
    int polygon_count() const { return polygon_count_; }
    // ... and the continuous bodies' column (CONTINUOUS BODIES): one 16-byte granule {rc, start} per body of a world whose column was active
    int reserve_sweep(int n, hipStream_t stream) { return n ? sweep_.reserve_keep((size_t)n, (size_t)sweep_count_, stream) : PHX_OK; }
    int save_sweep(const void* d_src, int count, hipStream_t stream)
    {
        sweep_count_ = count;
        if (!count) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(sweep_.p, d_src, (size_t)count * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(saved_, stream));                            // (the event moves behind the copy)
        return PHX_OK;
    }
    int load_sweep(void* d_dst, hipStream_t stream)                         // (queued behind Snapshot::load on the same stream)
    {
        if (!sweep_count_) return PHX_OK;
        PHX_HIP(hipMemcpyAsync(d_dst, sweep_.p, (size_t)sweep_count_ * sizeof(float4), hipMemcpyDeviceToDevice, stream));
        PHX_HIP(hipEventRecord(loaded_, stream));
        return PHX_OK;
    }
    int sweep_count() const { return sweep_count_; }
    bool polygons_named() const { return polygons_named_; }
    bool shape_capsules() const { return shape_capsules_; }
    int blob_bytes(size_t* bytes);
    int export_blob(void* blob, size_t cap);
    int import_blob(const void* blob, size_t bytes);

private:
    int settle();                        // the host waits for the queued save and loads (export, import, destroy)
    int refuse_empty(const char* what) const;
    int refuse_pins(const char* what);            // the blob is layout version 1 and holds no pins, no links, no angles, no sliders, no exclusions and no circles
    template <class P> struct Riders {            // a list of records beside the blob
        using record = P;
        DevBuf<P> buf; int count = 0;
        DevBuf<float> limits; bool limited = false;      // the records' break limits, where the saved list had a column
        int reserve(int n, bool with_limits, hipStream_t stream)                // (none: nothing is allocated)
        {
            if (n && with_limits) PHX_TRY(limits.reserve_keep((size_t)n, limited ? (size_t)count : 0, stream));
            return n ? buf.reserve_keep((size_t)n, (size_t)count, stream) : PHX_OK;
        }
    };
    std::tuple<Riders<phx_pin>, Riders<phx_link>, Riders<phx_angle>, Riders<phx_slider>> riders_;      // (the kinds in the pass's order)
    template <class P> Riders<P>& riders() { return std::get<Riders<P>>(riders_); }
    DevBuf<uint2> exclusions_; int exclusion_count_ = 0;
    DevBuf<uint32_t> shapes_; int shape_count_ = 0; bool shape_capsules_ = false;
    DevBuf<uint32_t> polygons_; int polygon_count_ = 0; bool polygons_named_ = false;
    DevBuf<float4> sweep_; int sweep_count_ = 0;

    int device_;
    DevBuf<uint4> buf_;                  // the blob behind its header; grows geometrically, reused by every save
    bool filled_ = false, accel_pending_ = false;
    SnapCounts counts_;
    SnapLayout layout_ = {};
    hipEvent_t saved_ = nullptr, loaded_ = nullptr;      // recorded behind the last save / the last load
    bool saved_pending_ = false, loaded_pending_ = false;
};

} // namespace phx

struct phx_snapshot {
    phx::Snapshot impl;
    explicit phx_snapshot(int device) : impl(device) {}
};
