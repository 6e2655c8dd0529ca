// snapshot.hip — Snapshot: the device side of phx_world_save / phx_world_load and the blob that leaves the device
// (include/phyx_amd.h SNAPSHOTS; the layout and its validator: snapshot_blob.h; the kernels: snapshot_kernels.h).
//
// One allocation holds the saved world in the blob's own layout, so a save is ONE kernel that walks a table of {source, destination,
// granules}, a load is its inverse fused with what a load derives (resident arrays, pending accelerations, the pair list), and
// export / import are one copy each behind / after the 128-byte header.  Ordering between streams: a save records `saved_`, which a
// later load's stream waits for; a load records `loaded_`, which the next save into this snapshot waits for — a fork (world A saves,
// world B loads) needs no host wait and no extra stream.  The host waits only in export, import and destroy.
#include "snapshot.h"
#include "pins.h"
#include "snapshot_kernels.h"

namespace phx {

static inline int snap_grid(unsigned long long items) { return (int)std::max<unsigned long long>(1, std::min<unsigned long long>((items + 255) / 256, 2048)); }

Snapshot::~Snapshot()
{
    if (hipSetDevice(device_) != hipSuccess) return;
    (void)settle();
    if (saved_) (void)hipEventDestroy(saved_);
    if (loaded_) (void)hipEventDestroy(loaded_);
}

int Snapshot::init()
{
    PHX_TRY(use_device(device_));
    PHX_HIP(hipEventCreateWithFlags(&saved_, hipEventDisableTiming));
    PHX_HIP(hipEventCreateWithFlags(&loaded_, hipEventDisableTiming));
    return PHX_OK;
}

int Snapshot::settle()
{
    if (saved_pending_) { PHX_HIP(hipEventSynchronize(saved_)); saved_pending_ = false; }
    if (loaded_pending_) { PHX_HIP(hipEventSynchronize(loaded_)); loaded_pending_ = false; }
    return PHX_OK;
}

int Snapshot::refuse_empty(const char* what) const
{
    if (filled_) return PHX_OK;
    set_error("%s: the snapshot was never filled (phx_world_save, phx_snapshot_import)", what);
    return PHX_ERR_STATE;
}

int Snapshot::refuse_pins(const char* what)
{
    int count = 0;                                                          // the first kind that has riders names the refusal
    const char* plural = nullptr;
    auto look = [&](const auto& r) { if (!count && r.count) { count = r.count; plural = UnitKind<typename std::decay_t<decltype(r)>::record>::plural; } };
    std::apply([&](const auto&... r) { (look(r), ...); }, riders_);
    if (!count && exclusion_count_) { count = exclusion_count_; plural = "collision exclusions"; }
    if (!count && shape_count_) {                                           // the saved kinds: refused while one of them is not a box
        PHX_TRY(use_device(device_));
        PHX_TRY(settle());
        std::vector<uint32_t> kinds((size_t)shape_count_);
        PHX_HIP(hipMemcpy(kinds.data(), shapes_.p, kinds.size() * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (const uint32_t k : kinds) count += k != (uint32_t)PHX_SHAPE_BOX;
        plural = "circles, capsules or polygons";
    }
    if (!count) return PHX_OK;
    set_error("%s: the snapshot holds %d %s, which the blob (layout version 1) does not carry", what, count, plural);
    return PHX_ERR_STATE;
}

// the largest walk of a launch: the bodies, or the granules of the largest array
static unsigned long long snap_items(const SnapTable& t)
{
    unsigned long long items = (unsigned long long)t.nb;
    for (const SnapCopy& c : t.seg) items = std::max(items, c.granules + (c.tail_words ? 1 : 0));
    return items;
}

// the seven plain copies between a world's arrays and the snapshot's sections
static SnapTable snap_table(const SnapshotWorld& w, const SnapCounts& c, const SnapLayout& l, uint4* buf, bool to_snapshot)
{
    void* const world[SNAP_COPIES] = {w.manifolds, w.cps, w.joints, (c.columns & SNAP_HAS_FILTERS) ? w.filters : nullptr,
                                      (c.columns & SNAP_HAS_MATERIALS) ? (void*)w.materials : nullptr, (c.columns & SNAP_HAS_FLAGS) ? (void*)w.flags : nullptr, w.baseline};
    SnapTable t;
    t.nb = c.bodies;
    for (int k = 0; k < SNAP_COPIES; ++k) {
        const int section = k + 1;
        uint4* mine = buf + (l.offset[section] - SNAP_HEADER_BYTES) / 16;
        SnapCopy& s = t.seg[k];
        s.src = to_snapshot ? static_cast<const uint4*>(world[k]) : mine;
        s.dst = to_snapshot ? mine : static_cast<uint4*>(world[k]);
        s.granules = l.bytes[section] / 16;
        s.tail_words = (unsigned)((l.bytes[section] % 16) / 4);
    }
    return t;
}

int Snapshot::save(const SnapshotWorld& w, hipStream_t stream)
{
    PHX_TRY(use_device(device_));
    const SnapLayout l = snap_layout(w.counts);
    PHX_TRY(buf_.reserve((size_t)((l.total - SNAP_HEADER_BYTES) / 16)));      // (a buffer that grows frees the old one, which waits for the device)
    // the loads that still read the old contents, and a save another world may have queued, go first
    if (loaded_pending_) PHX_HIP(hipStreamWaitEvent(stream, loaded_, 0));
    if (saved_pending_) PHX_HIP(hipStreamWaitEvent(stream, saved_, 0));
    const SnapTable t = snap_table(w, w.counts, l, buf_.p, true);
    const unsigned long long items = snap_items(t);
    if (items) hipLaunchKernelGGL(k_snapshot_save, dim3(snap_grid(items)), dim3(256), 0, stream, t, (const phx_rigid_body*)w.records, w.resident, w.records_stale ? 1 : 0,
                                  reinterpret_cast<float4*>(buf_.p));
    PHX_HIP(hipGetLastError());
    PHX_HIP(hipEventRecord(saved_, stream));
    saved_pending_ = true;
    counts_ = w.counts; layout_ = l; accel_pending_ = w.accel_pending; filled_ = true;
    return PHX_OK;
}

int Snapshot::load(const SnapshotWorld& w, hipStream_t stream)
{
    PHX_TRY(refuse_empty("phx_world_load"));
    PHX_TRY(use_device(device_));
    if (saved_pending_) PHX_HIP(hipStreamWaitEvent(stream, saved_, 0));
    // (one event stands for every load so far: a load on another stream goes behind the one before it, and the event behind both)
    if (loaded_pending_) PHX_HIP(hipStreamWaitEvent(stream, loaded_, 0));
    const SnapTable t = snap_table(w, counts_, layout_, buf_.p, false);
    const unsigned long long items = snap_items(t);
    if (items) hipLaunchKernelGGL(k_snapshot_load, dim3(snap_grid(items)), dim3(256), 0, stream, t, reinterpret_cast<const float4*>(buf_.p), w.records, w.resident,
                                  accel_pending_ ? w.accel : (float4*)nullptr, w.pairs);
    PHX_HIP(hipGetLastError());
    PHX_HIP(hipEventRecord(loaded_, stream));
    loaded_pending_ = true;
    return PHX_OK;
}

int Snapshot::blob_bytes(size_t* bytes)
{
    PHX_TRY(refuse_empty("phx_snapshot_blob_bytes"));
    PHX_TRY(refuse_pins("phx_snapshot_blob_bytes"));
    *bytes = (size_t)layout_.total;
    return PHX_OK;
}

int Snapshot::export_blob(void* blob, size_t cap)
{
    PHX_TRY(refuse_empty("phx_snapshot_export"));
    PHX_TRY(refuse_pins("phx_snapshot_export"));
    if (!blob) { set_error("phx_snapshot_export: null buffer"); return PHX_ERR_INVALID; }
    if ((uint64_t)cap < layout_.total) { set_error("phx_snapshot_export: the blob needs %llu bytes, room for %zu", (unsigned long long)layout_.total, cap); return PHX_ERR_CAPACITY; }
    PHX_TRY(use_device(device_));
    PHX_TRY(settle());
    unsigned char* out = static_cast<unsigned char*>(blob);
    snap_write_header(out, counts_, layout_);
    const size_t rest = (size_t)(layout_.sweep_offset - SNAP_HEADER_BYTES);      // (the eight sections; the continuous bodies' column rides beside them)
    if (rest) PHX_HIP(hipMemcpy(out + SNAP_HEADER_BYTES, buf_.p, rest, hipMemcpyDeviceToHost));
    if (layout_.sweep_bytes) PHX_HIP(hipMemcpy(out + layout_.sweep_offset, sweep_.p, (size_t)layout_.sweep_bytes, hipMemcpyDeviceToHost));
    return PHX_OK;
}

int Snapshot::import_blob(const void* blob, size_t bytes)
{
    char why[256] = "";
    SnapCounts c; SnapLayout l; bool accelerations = false;
    if (snap_blob_check(blob, bytes, why, sizeof why, &c, &l, &accelerations) != PHX_OK) { set_error("phx_snapshot_import: %s", why); return PHX_ERR_INVALID; }
    PHX_TRY(use_device(device_));
    PHX_TRY(settle());
    const size_t rest = (size_t)(l.sweep_offset - SNAP_HEADER_BYTES);
    PHX_TRY(buf_.reserve(rest / 16));
    if (rest) PHX_HIP(hipMemcpy(buf_.p, static_cast<const unsigned char*>(blob) + SNAP_HEADER_BYTES, rest, hipMemcpyHostToDevice));
    if (l.sweep_bytes) {
        PHX_TRY(sweep_.reserve((size_t)c.bodies));
        PHX_HIP(hipMemcpy(sweep_.p, static_cast<const unsigned char*>(blob) + l.sweep_offset, (size_t)l.sweep_bytes, hipMemcpyHostToDevice));
    }
    counts_ = c; layout_ = l; accel_pending_ = accelerations; filled_ = true;
    std::apply([](auto&... r) { ((r.count = 0), ...); }, riders_);
    exclusion_count_ = 0;
    shape_count_ = 0; shape_capsules_ = false;
    polygon_count_ = 0; polygons_named_ = false;
    sweep_count_ = l.sweep_bytes ? c.bodies : 0;
    return PHX_OK;
}

} // namespace phx

// ---- C ABI (phx_world_save / phx_world_load: c_api_world.hip) ----------------------------------------------------------------------------
extern "C" {

int phx_snapshot_create(phx_snapshot** out, int device)
{
    PHX_REQUIRE(out, "null out");
    *out = nullptr;
    PHX_TRY(phx::use_device(device));
    phx_snapshot* s = new (std::nothrow) phx_snapshot(device);
    PHX_REQUIRE(s, "out of host memory");
    const int st = s->impl.init();
    if (st != PHX_OK) { delete s; return st; }
    *out = s;
    return PHX_OK;
}

void phx_snapshot_destroy(phx_snapshot* s) { delete s; }

int phx_snapshot_counts(phx_snapshot* s, int32_t* bodies, int32_t* manifolds, int32_t* contact_points, int32_t* joints)
{
    PHX_REQUIRE(s, "phx_snapshot_counts: null handle");
    if (!s->impl.filled()) { phx::set_error("phx_snapshot_counts: the snapshot was never filled (phx_world_save, phx_snapshot_import)"); return PHX_ERR_STATE; }
    const phx::SnapCounts& c = s->impl.counts();
    if (bodies) *bodies = c.bodies;
    if (manifolds) *manifolds = c.manifolds;
    if (contact_points) *contact_points = 2 * c.manifolds;
    if (joints) *joints = c.joints;
    return PHX_OK;
}

int phx_snapshot_blob_bytes(phx_snapshot* s, size_t* bytes)
{
    PHX_REQUIRE(s && bytes, "phx_snapshot_blob_bytes: null handle / output");
    return s->impl.blob_bytes(bytes);
}

int phx_snapshot_export(phx_snapshot* s, void* blob, size_t cap)
{
    PHX_REQUIRE(s, "phx_snapshot_export: null handle");
    return s->impl.export_blob(blob, cap);
}

int phx_snapshot_import(phx_snapshot* s, const void* blob, size_t bytes)
{
    PHX_REQUIRE(s, "phx_snapshot_import: null handle");
    return s->impl.import_blob(blob, bytes);
}

int phx_snapshot_blob_check(const void* blob, size_t bytes)
{
    char why[256] = "";
    const int st = phx::snap_blob_check(blob, bytes, why, sizeof why);
    if (st != PHX_OK) phx::set_error("%s", why);
    return st;
}

int phx_snapshot_blob_pack(const phx_rigid_body* bodies, int32_t body_count, const phx_manifold* manifolds, int32_t manifold_count,
                           const phx_contact_point* cps, int32_t cp_count, const phx_contact_joint* joints, int32_t joint_count,
                           const phx_collision_filter* filters, const phx_material* materials, const uint32_t* flags,
                           const int32_t* baseline_pairs, int32_t baseline_count, void* blob, size_t cap, size_t* bytes)
{
    char why[256] = "";
    const int st = phx::snap_blob_pack(bodies, body_count, manifolds, manifold_count, cps, cp_count, joints, joint_count, filters, materials, flags,
                                       baseline_pairs, baseline_count, blob, cap, bytes, why, sizeof why);
    if (st != PHX_OK) phx::set_error("%s", why);
    return st;
}

} // extern "C"
