// snapshot_blob.h — the one serialised form of a saved world (include/phyx_amd.h, SNAPSHOTS): its layout, the validator and the
// packer.  Host only: no HIP include, so it also builds into a stand-alone program.  Everything is read and written through memcpy
// and byte-wise little-endian helpers: a blob may sit at any address.
//
// Layout (little-endian; every section starts at a multiple of 16 bytes from the start of the blob, the bytes between a section's end
// and the next start are zero):
//     0  char[8]   magic "PHXSNAP\0"
//     8  uint32    layout version (1)
//    12  uint32    header bytes (128)
//    16  int32     body count n
//    20  int32     manifold count m
//    24  int32     contact point count (2 m)
//    28  int32     joint count j
//    32  uint32    column bits: 1 collision filters, 2 materials, 4 body flags, 8 continuous bodies (a clear bit: every body has the
//                  default, no section)
//    36  int32     baseline count t
//    40  uint64    total bytes of the blob
//    48  uint64[8] section offsets, in this order (a section of no bytes still has the offset the layout gives it):
//                    bodies          n x 128   phx_rigid_body
//                    manifolds       m x 16    phx_manifold
//                    contact points  2m x 32   phx_contact_point
//                    joints          j x 20    phx_contact_joint
//                    filters         n x 16    {category, mask, group, 0}: the resident column's granule, so that it is copied as it is
//                    materials       n x 8     phx_material
//                    flags           n x 4     uint32
//                    baseline        t x 8     uint64 (body1 << 32) | body2, strictly increasing
//   112  uint64    offset of the continuous bodies' section, n x 16 {rc, start.x, start.y, 0}, behind the baseline: written only with
//                  column bit 8; without it these bytes are zero and the blob is what it was before the bit existed
//   120  8 bytes   zero
// The first section starts at 128, every other at the end of the one before rounded up to 16, and the total is the last end rounded
// up to 16.  The device side of a snapshot (snapshot.h) holds bytes [128, total) of this, so export and import are one copy each.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/phyx_amd.h"

namespace phx {

constexpr unsigned char SNAP_MAGIC[8] = {'P', 'H', 'X', 'S', 'N', 'A', 'P', 0};
constexpr uint32_t SNAP_VERSION = 1;
constexpr uint64_t SNAP_HEADER_BYTES = 128;
enum { SNAP_BODIES = 0, SNAP_MANIFOLDS, SNAP_CPS, SNAP_JOINTS, SNAP_FILTERS, SNAP_MATERIALS, SNAP_FLAGS, SNAP_BASELINE, SNAP_SECTIONS };
enum { SNAP_HAS_FILTERS = 1, SNAP_HAS_MATERIALS = 2, SNAP_HAS_FLAGS = 4, SNAP_HAS_SWEEP = 8, SNAP_COLUMN_BITS = 15 };
constexpr uint64_t SNAP_SWEEP_OFFSET_AT = 112;      // (the ninth offset: not one of the kernels' sections, the column rides beside them: snapshot.h)
constexpr const char* SNAP_SECTION_NAME[SNAP_SECTIONS] = {"bodies", "manifolds", "contact points", "joints", "filters", "materials", "flags", "baseline"};
constexpr uint64_t SNAP_ELEMENT_BYTES[SNAP_SECTIONS] = {128, 16, 32, 20, 16, 8, 4, 8};

struct SnapCounts {
    int32_t bodies = 0, manifolds = 0, joints = 0, baseline = 0;
    uint32_t columns = 0;
};
struct SnapLayout {
    uint64_t offset[SNAP_SECTIONS], bytes[SNAP_SECTIONS], total;
    uint64_t sweep_offset, sweep_bytes;      // the continuous bodies' section (SNAP_HAS_SWEEP), behind the eight: no bytes without the bit
};

// counts are non-negative int32: the largest section is 2^31 x 128 bytes, nothing here can overflow 64 bits
inline SnapLayout snap_layout(const SnapCounts& c)
{
    const uint64_t n = (uint64_t)c.bodies;
    const uint64_t elements[SNAP_SECTIONS] = {n, (uint64_t)c.manifolds, 2 * (uint64_t)c.manifolds, (uint64_t)c.joints,
                                              (c.columns & SNAP_HAS_FILTERS) ? n : 0, (c.columns & SNAP_HAS_MATERIALS) ? n : 0,
                                              (c.columns & SNAP_HAS_FLAGS) ? n : 0, (uint64_t)c.baseline};
    SnapLayout l;
    uint64_t at = SNAP_HEADER_BYTES;
    for (int k = 0; k < SNAP_SECTIONS; ++k) {
        l.offset[k] = at;
        l.bytes[k] = elements[k] * SNAP_ELEMENT_BYTES[k];
        at = (at + l.bytes[k] + 15) & ~uint64_t(15);
    }
    l.sweep_offset = at;
    l.sweep_bytes = (c.columns & SNAP_HAS_SWEEP) ? n * 16 : 0;
    l.total = at + l.sweep_bytes;
    return l;
}

inline void snap_put32(unsigned char* p, uint32_t v) { for (int k = 0; k < 4; ++k) p[k] = (unsigned char)(v >> (8 * k)); }
inline void snap_put64(unsigned char* p, uint64_t v) { for (int k = 0; k < 8; ++k) p[k] = (unsigned char)(v >> (8 * k)); }
inline uint32_t snap_get32(const unsigned char* p) { uint32_t v = 0; for (int k = 0; k < 4; ++k) v |= (uint32_t)p[k] << (8 * k); return v; }
inline uint64_t snap_get64(const unsigned char* p) { uint64_t v = 0; for (int k = 0; k < 8; ++k) v |= (uint64_t)p[k] << (8 * k); return v; }
template <class T> inline T snap_load(const void* base, uint64_t i)
{
    T v;
    std::memcpy(&v, static_cast<const unsigned char*>(base) + i * sizeof(T), sizeof(T));
    return v;
}

inline void snap_write_header(unsigned char* h, const SnapCounts& c, const SnapLayout& l)
{
    std::memset(h, 0, SNAP_HEADER_BYTES);
    std::memcpy(h, SNAP_MAGIC, 8);
    snap_put32(h + 8, SNAP_VERSION); snap_put32(h + 12, (uint32_t)SNAP_HEADER_BYTES);
    snap_put32(h + 16, (uint32_t)c.bodies); snap_put32(h + 20, (uint32_t)c.manifolds); snap_put32(h + 24, 2u * (uint32_t)c.manifolds);
    snap_put32(h + 28, (uint32_t)c.joints); snap_put32(h + 32, c.columns); snap_put32(h + 36, (uint32_t)c.baseline);
    snap_put64(h + 40, l.total);
    for (int k = 0; k < SNAP_SECTIONS; ++k) snap_put64(h + 48 + 8 * k, l.offset[k]);
    if (c.columns & SNAP_HAS_SWEEP) snap_put64(h + SNAP_SWEEP_OFFSET_AT, l.sweep_offset);
}

// The invariants the step's kernels rely on, shared by phx_world_set_state and the blob's validator: manifold i owns slots 2i and
// 2i + 1, body indices are in range, every joint's bodies are its manifold's and its contact point points back at it.  The arrays
// may be unaligned.  Returns the first violated rule, or null.
inline const char* snap_check_state(int body_count, const void* manifolds, int manifold_count, const void* cps, int cp_count, const void* joints, int joint_count)
{
    if (body_count < 0 || manifold_count < 0 || joint_count < 0 || (int64_t)cp_count != 2 * (int64_t)manifold_count) return "bad counts (two contact-point slots per manifold)";
    if ((manifold_count && (!manifolds || !cps)) || (joint_count && !joints)) return "null array";
    for (int i = 0; i < manifold_count; ++i) {
        const phx_manifold m = snap_load<phx_manifold>(manifolds, (uint64_t)i);
        if (!((uint32_t)m.body1 < (uint32_t)body_count && (uint32_t)m.body2 < (uint32_t)body_count)) return "manifold: body index out of range";
        if (!((int64_t)m.point_index == 2 * (int64_t)i && m.point_count >= 0 && m.point_count <= 2)) return "manifold: its contact points are slots 2i, 2i + 1";
    }
    for (int j = 0; j < joint_count; ++j) {
        const phx_contact_joint q = snap_load<phx_contact_joint>(joints, (uint64_t)j);
        if (!((uint32_t)q.contact_point_index < (uint32_t)cp_count)) return "joint: contact point out of range";
        const phx_manifold m = snap_load<phx_manifold>(manifolds, (uint64_t)(q.contact_point_index / 2));
        if (!(q.body1 == m.body1 && q.body2 == m.body2)) return "joint: bodies differ from its manifold's";
        if (snap_load<phx_contact_point>(cps, (uint64_t)q.contact_point_index).solver_index != j) return "joint: its contact point does not point back at it";
    }
    return nullptr;
}

// the ranges the setters enforce (phx_world_set_materials, phx_world_set_body_flags)
inline bool snap_material_ok(const phx_material& m) { return m.friction >= 0.f && m.friction <= 1e6f && m.restitution >= 0.f && m.restitution <= 1.f; }      // (NaN fails)
inline bool snap_flags_ok(uint32_t f) { return (f & ~(uint32_t)PHX_BODY_SENSOR) == 0; }

// The single validator.  PHX_OK, or PHX_ERR_INVALID with the first violated rule in `msg`.  On success *counts / *layout describe
// the blob and *accelerations says whether some body record carries an acceleration (each may be null).
inline int snap_blob_check(const void* blob, size_t bytes, char* msg, size_t msg_cap, SnapCounts* counts = nullptr, SnapLayout* layout = nullptr,
                           bool* accelerations = nullptr)
{
#define PHX_SNAP_FAIL(...) do { if (msg && msg_cap) std::snprintf(msg, msg_cap, __VA_ARGS__); return PHX_ERR_INVALID; } while (0)
    if (!blob) PHX_SNAP_FAIL("snapshot blob: null pointer");
    if ((uint64_t)bytes < SNAP_HEADER_BYTES) PHX_SNAP_FAIL("snapshot blob: %zu bytes are shorter than the %u-byte header", bytes, (unsigned)SNAP_HEADER_BYTES);
    const unsigned char* h = static_cast<const unsigned char*>(blob);
    if (std::memcmp(h, SNAP_MAGIC, 8) != 0) PHX_SNAP_FAIL("snapshot blob: wrong magic");
    if (snap_get32(h + 8) != SNAP_VERSION) PHX_SNAP_FAIL("snapshot blob: layout version %u, this library reads %u", snap_get32(h + 8), SNAP_VERSION);
    if (snap_get32(h + 12) != SNAP_HEADER_BYTES) PHX_SNAP_FAIL("snapshot blob: header size %u, expected %u", snap_get32(h + 12), (unsigned)SNAP_HEADER_BYTES);
    SnapCounts c;
    c.bodies = (int32_t)snap_get32(h + 16); c.manifolds = (int32_t)snap_get32(h + 20); c.joints = (int32_t)snap_get32(h + 28);
    c.columns = snap_get32(h + 32); c.baseline = (int32_t)snap_get32(h + 36);
    const int32_t cp_count = (int32_t)snap_get32(h + 24);
    if (c.bodies < 0 || c.manifolds < 0 || c.joints < 0 || c.baseline < 0 || cp_count < 0) PHX_SNAP_FAIL("snapshot blob: negative count");
    if ((int64_t)cp_count != 2 * (int64_t)c.manifolds) PHX_SNAP_FAIL("snapshot blob: %d contact points for %d manifolds (two slots per manifold)", cp_count, c.manifolds);
    if (c.columns & ~(uint32_t)SNAP_COLUMN_BITS) PHX_SNAP_FAIL("snapshot blob: unknown column bit in 0x%x", c.columns);
    for (int k = (c.columns & SNAP_HAS_SWEEP) ? 120 : 112; k < 128; ++k)
        if (h[k]) PHX_SNAP_FAIL("snapshot blob: reserved header byte %d is not zero", k);
    // sizes and offsets against `bytes`: every comparison is between values that exist, nothing is added before it is known to fit
    const SnapLayout l = snap_layout(c);
    const uint64_t total = snap_get64(h + 40);
    if (total != (uint64_t)bytes) PHX_SNAP_FAIL("snapshot blob: the header says %llu bytes, %zu were given", (unsigned long long)total, bytes);
    for (int k = 0; k < SNAP_SECTIONS; ++k) {
        const uint64_t off = snap_get64(h + 48 + 8 * k);
        if (off > (uint64_t)bytes || l.bytes[k] > (uint64_t)bytes - off) PHX_SNAP_FAIL("snapshot blob: section %s (offset %llu, %llu bytes) reaches beyond the end (%zu bytes)", SNAP_SECTION_NAME[k], (unsigned long long)off, (unsigned long long)l.bytes[k], bytes);
        if (off != l.offset[k]) PHX_SNAP_FAIL("snapshot blob: section %s is at offset %llu, the layout puts it at %llu", SNAP_SECTION_NAME[k], (unsigned long long)off, (unsigned long long)l.offset[k]);
    }
    if (l.total != (uint64_t)bytes) PHX_SNAP_FAIL("snapshot blob: %zu bytes, its counts need %llu", bytes, (unsigned long long)l.total);
    if ((c.columns & SNAP_HAS_SWEEP) && snap_get64(h + SNAP_SWEEP_OFFSET_AT) != l.sweep_offset)
        PHX_SNAP_FAIL("snapshot blob: section continuous bodies is at offset %llu, the layout puts it at %llu", (unsigned long long)snap_get64(h + SNAP_SWEEP_OFFSET_AT), (unsigned long long)l.sweep_offset);
    for (int k = 0; k < SNAP_SECTIONS; ++k) {
        const uint64_t end = k + 1 < SNAP_SECTIONS ? l.offset[k + 1] : l.sweep_offset;
        for (uint64_t at = l.offset[k] + l.bytes[k]; at < end; ++at)
            if (h[at]) PHX_SNAP_FAIL("snapshot blob: byte %llu behind section %s is not zero", (unsigned long long)at, SNAP_SECTION_NAME[k]);
    }
    // the state's invariants
    if (const char* bad = snap_check_state(c.bodies, h + l.offset[SNAP_MANIFOLDS], c.manifolds, h + l.offset[SNAP_CPS], cp_count, h + l.offset[SNAP_JOINTS], c.joints))
        PHX_SNAP_FAIL("snapshot blob: %s", bad);
    // the columns' ranges
    if (c.columns & SNAP_HAS_FILTERS)
        for (int i = 0; i < c.bodies; ++i)
            if (snap_get32(h + l.offset[SNAP_FILTERS] + 16 * (uint64_t)i + 12)) PHX_SNAP_FAIL("snapshot blob: filter of body %d: the fourth word is not zero", i);
    if (c.columns & SNAP_HAS_MATERIALS)
        for (int i = 0; i < c.bodies; ++i) {
            const phx_material m = snap_load<phx_material>(h + l.offset[SNAP_MATERIALS], (uint64_t)i);
            if (!snap_material_ok(m)) PHX_SNAP_FAIL("snapshot blob: material of body %d: friction %g not in [0, 1e6] or restitution %g not in [0, 1]", i, (double)m.friction, (double)m.restitution);
        }
    if (c.columns & SNAP_HAS_FLAGS)
        for (int i = 0; i < c.bodies; ++i) {
            const uint32_t f = snap_get32(h + l.offset[SNAP_FLAGS] + 4 * (uint64_t)i);
            if (!snap_flags_ok(f)) PHX_SNAP_FAIL("snapshot blob: flags 0x%x of body %d hold an unknown bit", f, i);
        }
    if (c.columns & SNAP_HAS_SWEEP)
        for (int i = 0; i < c.bodies; ++i) {
            float v[4];
            std::memcpy(v, h + l.sweep_offset + 16 * (uint64_t)i, sizeof v);
            if (!(v[0] >= 0.f && v[0] <= 3.0e38f)) PHX_SNAP_FAIL("snapshot blob: core radius %g of body %d is not finite and >= 0", (double)v[0], i);
            if (!(v[1] >= -3.0e38f && v[1] <= 3.0e38f && v[2] >= -3.0e38f && v[2] <= 3.0e38f)) PHX_SNAP_FAIL("snapshot blob: start of body %d is not finite", i);
            if (snap_get32(h + l.sweep_offset + 16 * (uint64_t)i + 12)) PHX_SNAP_FAIL("snapshot blob: continuous body %d: the fourth word is not zero", i);
        }
    // the baseline: strictly increasing keys of pairs of bodies
    uint64_t before = 0;
    for (int k = 0; k < c.baseline; ++k) {
        const uint64_t key = snap_get64(h + l.offset[SNAP_BASELINE] + 8 * (uint64_t)k);
        if ((key >> 32) >= (uint64_t)c.bodies || (key & 0xFFFFFFFFu) >= (uint64_t)c.bodies) PHX_SNAP_FAIL("snapshot blob: baseline pair %d: body index out of range", k);
        if (k && key <= before) PHX_SNAP_FAIL("snapshot blob: baseline pair %d is not above the one before it (sorted, no pair twice)", k);
        before = key;
    }
    if (accelerations) {
        *accelerations = false;
        for (int i = 0; i < c.bodies && !*accelerations; ++i) {
            const phx_rigid_body b = snap_load<phx_rigid_body>(h + l.offset[SNAP_BODIES], (uint64_t)i);
            *accelerations = b.acceleration.x != 0.f || b.acceleration.y != 0.f || b.angular_acceleration != 0.f;
        }
    }
    if (counts) *counts = c;
    if (layout) *layout = l;
    return PHX_OK;
#undef PHX_SNAP_FAIL
}

// A blob from host arrays (phx_snapshot_blob_pack).  A null column: every body has the default.  A null baseline: T(state), the
// touching pairs of the manifolds, as phx_world_set_state makes it.  *bytes always receives the blob's size; PHX_ERR_CAPACITY when
// `cap` is smaller.  What was written is then checked like any other blob.
inline int snap_blob_pack(const phx_rigid_body* bodies, int32_t body_count, const phx_manifold* manifolds, int32_t manifold_count,
                          const phx_contact_point* cps, int32_t cp_count, const phx_contact_joint* joints, int32_t joint_count,
                          const phx_collision_filter* filters, const phx_material* materials, const uint32_t* flags,
                          const int32_t* baseline_pairs, int32_t baseline_count, void* blob, size_t cap, size_t* bytes, char* msg, size_t msg_cap)
{
#define PHX_SNAP_FAIL(code, ...) do { if (msg && msg_cap) std::snprintf(msg, msg_cap, __VA_ARGS__); return code; } while (0)
    if (body_count < 0 || manifold_count < 0 || joint_count < 0 || baseline_count < 0 || (int64_t)cp_count != 2 * (int64_t)manifold_count)
        PHX_SNAP_FAIL(PHX_ERR_INVALID, "phx_snapshot_blob_pack: bad counts (two contact-point slots per manifold)");
    if ((body_count && !bodies) || (manifold_count && (!manifolds || !cps)) || (joint_count && !joints))
        PHX_SNAP_FAIL(PHX_ERR_INVALID, "phx_snapshot_blob_pack: null array");
    std::vector<uint64_t> keys;
    if (baseline_pairs) {
        keys.resize((size_t)baseline_count);
        for (int32_t k = 0; k < baseline_count; ++k) keys[(size_t)k] = ((uint64_t)(uint32_t)baseline_pairs[2 * (size_t)k] << 32) | (uint32_t)baseline_pairs[2 * (size_t)k + 1];
    } else {
        for (int32_t i = 0; i < manifold_count; ++i)
            if (manifolds[i].point_count > 0) keys.push_back(((uint64_t)(uint32_t)manifolds[i].body1 << 32) | (uint32_t)manifolds[i].body2);
        std::sort(keys.begin(), keys.end());
        keys.erase(std::unique(keys.begin(), keys.end()), keys.end());
    }
    if (keys.size() > (size_t)INT32_MAX) PHX_SNAP_FAIL(PHX_ERR_INVALID, "phx_snapshot_blob_pack: the baseline exceeds the int32 range");
    SnapCounts c;
    c.bodies = body_count; c.manifolds = manifold_count; c.joints = joint_count; c.baseline = (int32_t)keys.size();
    c.columns = (filters ? SNAP_HAS_FILTERS : 0) | (materials ? SNAP_HAS_MATERIALS : 0) | (flags ? SNAP_HAS_FLAGS : 0);
    const SnapLayout l = snap_layout(c);
    if (l.total > (uint64_t)SIZE_MAX) PHX_SNAP_FAIL(PHX_ERR_INVALID, "phx_snapshot_blob_pack: the blob does not fit the address space");
    if (bytes) *bytes = (size_t)l.total;
    if (!blob || (uint64_t)cap < l.total) PHX_SNAP_FAIL(PHX_ERR_CAPACITY, "phx_snapshot_blob_pack: the blob needs %llu bytes, room for %zu", (unsigned long long)l.total, blob ? cap : (size_t)0);
    unsigned char* out = static_cast<unsigned char*>(blob);
    std::memset(out, 0, (size_t)l.total);
    snap_write_header(out, c, l);
    auto put = [&](int section, const void* src) { if (l.bytes[section]) std::memcpy(out + l.offset[section], src, (size_t)l.bytes[section]); };
    put(SNAP_BODIES, bodies); put(SNAP_MANIFOLDS, manifolds); put(SNAP_CPS, cps); put(SNAP_JOINTS, joints);
    if (filters)
        for (int32_t i = 0; i < body_count; ++i) {
            unsigned char* f = out + l.offset[SNAP_FILTERS] + 16 * (uint64_t)i;
            snap_put32(f, filters[i].category); snap_put32(f + 4, filters[i].mask); snap_put32(f + 8, (uint32_t)filters[i].group);
        }
    if (materials) put(SNAP_MATERIALS, materials);
    if (flags) put(SNAP_FLAGS, flags);
    for (size_t k = 0; k < keys.size(); ++k) snap_put64(out + l.offset[SNAP_BASELINE] + 8 * k, keys[k]);
    return snap_blob_check(out, (size_t)l.total, msg, msg_cap);
#undef PHX_SNAP_FAIL
}

} // namespace phx
