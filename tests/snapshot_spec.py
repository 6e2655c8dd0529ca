"""The snapshot blob (include/phyx_amd.h SNAPSHOTS), restated from the header's description with struct and numpy: pack() builds a
blob from host arrays and check() names the first rule a blob violates (None if it is valid).  Tests compare the library's packer
and validator with these."""
import struct

import numpy as np

from phyx_amd import (rigid_body_dtype, manifold_dtype, contact_point_dtype, contact_joint_dtype, collision_filter_dtype, material_dtype)

MAGIC = b"PHXSNAP\0"
VERSION = 1
HEADER = 128
HAS_FILTERS, HAS_MATERIALS, HAS_FLAGS = 1, 2, 4
SECTIONS = ("bodies", "manifolds", "contact points", "joints", "filters", "materials", "flags", "baseline")
ELEMENT = (128, 16, 32, 20, 16, 8, 4, 8)
OFF_COUNTS, OFF_COLUMNS, OFF_BASELINE, OFF_TOTAL, OFF_OFFSETS = 16, 32, 36, 40, 48
BODY_SENSOR = 1


def up16(x):
    return (x + 15) // 16 * 16


def layout(n, m, j, columns, t):
    """(offsets, sizes, total): the first section at 128, each next one at the end of the one before rounded up to 16."""
    elements = (n, m, 2 * m, j, n if columns & HAS_FILTERS else 0, n if columns & HAS_MATERIALS else 0, n if columns & HAS_FLAGS else 0, t)
    offsets, sizes, at = [], [], HEADER
    for count, size in zip(elements, ELEMENT):
        offsets.append(at)
        sizes.append(count * size)
        at = up16(at + count * size)
    return offsets, sizes, at


def touching(manifolds):
    """T(state): the pairs of the manifolds with a live point, sorted, each once."""
    m = manifolds[manifolds["point_count"] > 0]
    pairs = sorted(set(zip(m["body1"].tolist(), m["body2"].tolist())))
    return np.array(pairs, dtype=np.int32).reshape(-1, 2)


def pack(bodies, manifolds, cps, joints, filters=None, materials=None, flags=None, baseline=None):
    bodies = np.ascontiguousarray(bodies, dtype=rigid_body_dtype); manifolds = np.ascontiguousarray(manifolds, dtype=manifold_dtype)
    cps = np.ascontiguousarray(cps, dtype=contact_point_dtype); joints = np.ascontiguousarray(joints, dtype=contact_joint_dtype)
    n, m, j = len(bodies), len(manifolds), len(joints)
    base = touching(manifolds) if baseline is None else np.asarray(baseline, dtype=np.int32).reshape(-1, 2)
    columns = (HAS_FILTERS if filters is not None else 0) | (HAS_MATERIALS if materials is not None else 0) | (HAS_FLAGS if flags is not None else 0)
    offsets, sizes, total = layout(n, m, j, columns, len(base))
    blob = bytearray(total)
    struct.pack_into("<8sII4iIiQ8Q", blob, 0, MAGIC, VERSION, HEADER, n, m, 2 * m, j, columns, len(base), total, *offsets)
    parts = [bodies.tobytes(), manifolds.tobytes(), cps.tobytes(), joints.tobytes(), b"", b"", b"", b""]
    if filters is not None:
        f = np.ascontiguousarray(filters, dtype=collision_filter_dtype)
        wide = np.zeros((n, 4), dtype="<u4")
        wide[:, 0], wide[:, 1], wide[:, 2] = f["category"], f["mask"], f["group"].astype("<u4")
        parts[4] = wide.tobytes()
    if materials is not None:
        parts[5] = np.ascontiguousarray(materials, dtype=material_dtype).tobytes()
    if flags is not None:
        parts[6] = np.ascontiguousarray(flags, dtype="<u4").tobytes()
    parts[7] = ((base[:, 0].astype(np.uint64) << np.uint64(32)) | base[:, 1].astype(np.uint32).astype(np.uint64)).astype("<u8").tobytes()
    for off, size, part in zip(offsets, sizes, parts):
        assert len(part) == size
        blob[off:off + size] = part
    return bytes(blob)


def check(blob):
    """The first violated rule as a short string, or None."""
    if len(blob) < HEADER:
        return "shorter than the header"
    magic, version, header, n, m, c, j, columns, t, total = struct.unpack_from("<8sII4iIiQ", blob, 0)
    offsets = struct.unpack_from("<8Q", blob, OFF_OFFSETS)
    if magic != MAGIC:
        return "magic"
    if version != VERSION:
        return "version"
    if header != HEADER:
        return "header size"
    if min(n, m, c, j, t) < 0:
        return "negative count"
    if c != 2 * m:
        return "two slots per manifold"
    if columns & ~7:
        return "unknown column bit"
    if any(blob[112:128]):
        return "reserved bytes"
    if total != len(blob):
        return "total size"
    want, sizes, want_total = layout(n, m, j, columns, t)
    for off, size, w in zip(offsets, sizes, want):
        if off > len(blob) or size > len(blob) - off:
            return "section beyond the end"
        if off != w:
            return "section offset"
    if want_total != len(blob):
        return "total size"
    for off, size, nxt in zip(want, sizes, want[1:] + [want_total]):
        if any(blob[off + size:nxt]):
            return "padding not zero"
    man = np.frombuffer(blob, dtype=manifold_dtype, count=m, offset=want[1])
    cps = np.frombuffer(blob, dtype=contact_point_dtype, count=c, offset=want[2])
    jts = np.frombuffer(blob, dtype=contact_joint_dtype, count=j, offset=want[3])
    for i in range(m):
        if not (0 <= man["body1"][i] < n and 0 <= man["body2"][i] < n):
            return "manifold body index"
        if man["point_index"][i] != 2 * i or not 0 <= man["point_count"][i] <= 2:
            return "manifold slots"
    for k in range(j):
        cp = int(jts["contact_point_index"][k])
        if not 0 <= cp < c:
            return "joint contact point"
        if jts["body1"][k] != man["body1"][cp // 2] or jts["body2"][k] != man["body2"][cp // 2]:
            return "joint bodies"
        if cps["solver_index"][cp] != k:
            return "joint back link"
    if columns & HAS_FILTERS and np.frombuffer(blob, dtype="<u4", count=4 * n, offset=want[4])[3::4].any():
        return "filter fourth word"
    if columns & HAS_MATERIALS:
        mt = np.frombuffer(blob, dtype=material_dtype, count=n, offset=want[5])
        ok = (mt["friction"] >= 0) & (mt["friction"] <= np.float32(1e6)) & (mt["restitution"] >= 0) & (mt["restitution"] <= 1)      # (NaN fails)
        if not ok.all():
            return "material range"
    if columns & HAS_FLAGS and (np.frombuffer(blob, dtype="<u4", count=n, offset=want[6]) & ~np.uint32(BODY_SENSOR)).any():
        return "unknown flag bit"
    keys = np.frombuffer(blob, dtype="<u8", count=t, offset=want[7])
    if ((keys >> np.uint64(32)) >= n).any() or ((keys & np.uint64(0xFFFFFFFF)) >= n).any():
        return "baseline body index"
    if t > 1 and not (keys[1:] > keys[:-1]).all():
        return "baseline order"
    return None
