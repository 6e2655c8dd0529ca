"""Host-side mirror of the reference's interface for the hot path, over the C ABI.

Names and argument meaning follow the reference (ref = /root/reference/src):
  Configuration  <- Configuration.h:3-23      (solveMode, islandMode, contactIterationsCount, penetrationIterationsCount)
  Solver         <- Solver.h:47-128           (SolveJoints, islandCount, islandMaxSize)
  Collider       <- Collider.h:24-66          (UpdateBroadphase + UpdatePairs, broadphase[], broadphaseSort[1])
  World          <- World.h:9-36              (AddBody, Update, bodies, gravity)
Arrays are numpy structured arrays with the reference's exact POD layouts, so the same buffers can be
handed to the oracle in tests/.  All compute happens inside libphyx_amd.so (HIP); nothing here
falls back to numpy or the CPU.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import Config, SolveStats, BroadphaseStats, BenchResult, check

SOLVE_SCALAR, SOLVE_SSE2, SOLVE_AVX2 = 0, 1, 2
ISLAND_SINGLE, ISLAND_MULTIPLE, ISLAND_SINGLE_SLOPPY, ISLAND_MULTIPLE_SLOPPY = 0, 1, 2, 3

_vec2 = np.dtype([("x", "<f4"), ("y", "<f4")])
rigid_body_dtype = np.dtype([
    ("index", "<u4"), ("geom_size", _vec2), ("geom_xv", _vec2), ("geom_yv", _vec2), ("geom_pos", _vec2),
    ("aabb_min", _vec2), ("aabb_max", _vec2), ("velocity", _vec2), ("acceleration", _vec2),
    ("displacing_velocity", _vec2), ("angular_velocity", "<f4"), ("angular_acceleration", "<f4"),
    ("displacing_angular_velocity", "<f4"), ("inv_mass", "<f4"), ("inv_inertia", "<f4"),
    ("xv", _vec2), ("yv", _vec2), ("pos", _vec2), ("last_iteration", "<i4"), ("last_displacement_iteration", "<i4"),
])
contact_point_dtype = np.dtype([
    ("delta1", _vec2), ("delta2", _vec2), ("normal", _vec2), ("is_merged", "u1"), ("is_newly_created", "u1"),
    ("pad", "u1", (2,)), ("solver_index", "<i4"),
])
manifold_dtype = np.dtype([("body1", "<i4"), ("body2", "<i4"), ("point_count", "<i4"), ("point_index", "<i4")])
contact_joint_dtype = np.dtype([("contact_point_index", "<i4"), ("body1", "<i4"), ("body2", "<i4"),
                                ("normal_acc", "<f4"), ("friction_acc", "<f4")])
broadphase_entry_dtype = np.dtype([("minx", "<f4"), ("maxx", "<f4"), ("centery", "<f4"), ("extenty", "<f4"), ("index", "<u4")])
sort_entry_dtype = np.dtype([("value", "<u4"), ("index", "<u4")])
assert rigid_body_dtype.itemsize == 128 and contact_point_dtype.itemsize == 32
ray_hit_dtype = np.dtype([("body", "<i4"), ("t", "<f4"), ("normal", "<f4", (2,)), ("point", "<f4", (2,))])      # phx_ray_hit
assert ray_hit_dtype.itemsize == 24
shape_hit_dtype = np.dtype([("body", "<i4"), ("t", "<f4"), ("normal", "<f4", (2,))])      # phx_shape_hit
assert shape_hit_dtype.itemsize == 16
near_hit_dtype = np.dtype([("body", "<i4"), ("distance", "<f4"), ("normal", "<f4", (2,)), ("point", "<f4", (2,))])      # phx_near_hit
assert near_hit_dtype.itemsize == 24
contact_dtype = np.dtype([("other", "<i4"), ("manifold", "<i4"), ("slot", "<i4"), ("flags", "<i4"), ("point", "<f4", (2,)), ("normal", "<f4", (2,)),
                          ("normal_impulse", "<f4"), ("friction_impulse", "<f4")])                                     # phx_contact
collision_filter_dtype = np.dtype([("category", "<u4"), ("mask", "<u4"), ("group", "<i4")])      # phx_collision_filter
material_dtype = np.dtype([("friction", "<f4"), ("restitution", "<f4")])      # phx_material
assert material_dtype.itemsize == 8
shape_dtype = np.dtype([("kind", "<i4"), ("hx", "<f4"), ("hy", "<f4")])      # phx_shape
assert shape_dtype.itemsize == 12
polygon_dtype = np.dtype([("count", "<i4"), ("v", "<f4", (8, 2))])      # phx_polygon
assert polygon_dtype.itemsize == 68
sweep_hit_dtype = np.dtype([("body", "<i4"), ("target", "<i4"), ("t", "<f4"), ("normal", "<f4", (2,))])      # phx_sweep_hit
assert sweep_hit_dtype.itemsize == 20
contact_marker_dtype = np.dtype([("point1", "<f4", (2,)), ("point2", "<f4", (2,)), ("live", "<i4"), ("newly_created", "<i4")])     # phx_contact_marker
assert contact_dtype.itemsize == 40 and contact_marker_dtype.itemsize == 24
pin_dtype = np.dtype([("body1", "<i4"), ("body2", "<i4"), ("anchor1", "<f4", (2,)), ("anchor2", "<f4", (2,)), ("impulse", "<f4", (2,))])      # phx_pin
assert pin_dtype.itemsize == 32
link_dtype = np.dtype([("body1", "<i4"), ("body2", "<i4"), ("anchor1", "<f4", (2,)), ("anchor2", "<f4", (2,)), ("min_length", "<f4"), ("max_length", "<f4"),
                       ("hertz", "<f4"), ("damping_ratio", "<f4"), ("impulse", "<f4"), ("reserved", "<u4")])      # phx_link
assert link_dtype.itemsize == 48
angle_dtype = np.dtype([("body1", "<i4"), ("body2", "<i4"), ("lower", "<f4"), ("upper", "<f4"), ("hertz", "<f4"), ("damping_ratio", "<f4"),
                        ("motor_speed", "<f4"), ("max_torque", "<f4"), ("impulse", "<f4"), ("motor_impulse", "<f4")])      # phx_angle
assert angle_dtype.itemsize == 40
slider_dtype = np.dtype([("body1", "<i4"), ("body2", "<i4"), ("anchor1", "<f4", (2,)), ("anchor2", "<f4", (2,)), ("axis", "<f4", (2,)), ("lower", "<f4"), ("upper", "<f4"),
                         ("hertz", "<f4"), ("damping_ratio", "<f4"), ("motor_speed", "<f4"), ("max_force", "<f4"), ("impulse", "<f4"), ("axis_impulse", "<f4"),
                         ("motor_impulse", "<f4"), ("reserved", "<u4")])      # phx_slider
assert slider_dtype.itemsize == 72
break_event_dtype = np.dtype([("kind", "<i4"), ("index", "<i4"), ("body1", "<i4"), ("body2", "<i4"), ("step", "<i4"), ("reaction", "<f4"), ("threshold", "<f4"),
                              ("reserved", "<u4")])      # phx_break_event
assert break_event_dtype.itemsize == 32
sleep_state_dtype = np.dtype([("asleep", "<i4"), ("timer", "<f4"), ("inv_mass", "<f4"), ("inv_inertia", "<f4")])      # phx_sleep_state
assert sleep_state_dtype.itemsize == 16
field_dtype = np.dtype([("kind", "<i4"), ("shape", "<i4"), ("mask", "<u4"), ("flags", "<u4"), ("region", "<f4", (4,)), ("value", "<f4", (4,))])      # phx_field
assert field_dtype.itemsize == 48 == C.sizeof(_lib.Field)
MAX_FIELDS = 256                                               # PHX_MAX_FIELDS
FIELD_UNIFORM, FIELD_RADIAL, FIELD_DRAG = 0, 1, 2              # phx_field.kind
REGION_ALL, REGION_BOX, REGION_DISC = 0, 1, 2                  # phx_field.shape
FIELD_FORCE = 1                                                # PHX_FIELD_FORCE (phx_field.flags)
UNIT_KINDS = ("pin", "link", "angle", "slider")      # PHX_UNIT_PIN ... PHX_UNIT_SLIDER
CONTACT_NEW, CONTACT_NO_JOINT = 1, 2      # phx_contact.flags
BODY_SENSOR = 1                           # PHX_BODY_SENSOR (phx_world_set_body_flags)
SHAPE_BOX, SHAPE_CIRCLE, SHAPE_CAPSULE = 0, 1, 2            # PHX_SHAPE_BOX, PHX_SHAPE_CIRCLE, PHX_SHAPE_CAPSULE (phx_shape.kind)
SHAPE_POLYGON, POLYGON_MAX_VERTICES = 3, 8                  # PHX_SHAPE_POLYGON, PHX_POLYGON_MAX_VERTICES
assert manifold_dtype.itemsize == 16 and contact_joint_dtype.itemsize == 20 and broadphase_entry_dtype.itemsize == 20


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _dev_ptr(p):
    """A device address given as an int (a torch tensor's data_ptr()) or a ctypes pointer (DeviceBuffer.address())."""
    return p if isinstance(p, C.c_void_p) else C.c_void_p(int(p))


def frame_from_angle(px, py, angle):
    """{pos.x, pos.y, xv.x, xv.y, yv.x, yv.y} of a body at `angle`, rounded as AddBody rounds it (ref: RigidBody.h:15-36, Coords2.h:10-17:
    the float angle and angle + pi / 2 go through the double cos / sin, then narrow to float)."""
    a = np.float32(angle)
    quarter = np.float32(a + np.float32(np.float32(3.141592) / np.float32(2.0)))
    return np.array([px, py, math.cos(float(a)), math.sin(float(a)), math.cos(float(quarter)), math.sin(float(quarter))], dtype=np.float32)


def box_from_angle(px, py, angle, hx, hy):
    """The query box {pos.x, pos.y, xv.x, xv.y, yv.x, yv.y, h.x, h.y} of World.query_boxes / cast_boxes, with the frame add_body builds
    for `angle` (frame_from_angle)."""
    return np.concatenate([frame_from_angle(px, py, angle), np.array([hx, hy], dtype=np.float32)])


def pinned_inv_inertia(sx, sy):
    """invInertia of a box pinned by invMass = 0 only (ref: main.cpp:176-177): AddBody's float formula (RigidBody.h:15-36)."""
    sx, sy = float(sx), float(sy)
    mass = np.float32(1e-5) * (np.float32(sx) * np.float32(sy))
    inertia = mass * (np.float32(sx) * np.float32(sx) + np.float32(sy) * np.float32(sy))
    return float(np.float32(1.0) / inertia)


def circle_inverse_masses(r):
    """(K, 2) float32 {invMass, invInertia} of circles of radii r on AddBody's scale (include/phyx_amd.h SHAPES): mass = 1e-5f *
    0.785398f * r * r, inertia = mass * 1.5f * r * r, every operation a float32 one, left to right."""
    r = np.atleast_1d(np.asarray(r, dtype=np.float32))
    f = np.float32
    with np.errstate(over="ignore", divide="ignore"):
        mass = f(1e-5) * f(0.785398) * r * r
        inertia = mass * f(1.5) * r * r
        return np.stack([f(1.0) / mass, f(1.0) / inertia], axis=1).astype(np.float32)


def capsule_inverse_masses(hx, hy):
    """(K, 2) float32 {invMass, invInertia} of capsules of frame half extents hx > hy on AddBody's scale (include/phyx_amd.h SHAPES), with
    a = hx - hy and r = hy: mb = 1e-5f*a*r, mc = 1e-5f*0.785398f*r*r, mass = mb + mc, inertia = mb*(a*a + r*r) + mc*(1.5f*r*r + 3.0f*a*a +
    2.546479f*a*r), every operation a float32 one, left to right.  The rectangle's term is the box formula; a -> 0 gives the circle's."""
    f = np.float32
    hx, hy = np.broadcast_arrays(np.atleast_1d(np.asarray(hx, dtype=f)), np.atleast_1d(np.asarray(hy, dtype=f)))
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        a, r = hx - hy, hy
        mb = f(1e-5) * a * r
        mc = f(1e-5) * f(0.785398) * r * r
        mass = mb + mc
        inertia = mb * (a * a + r * r) + mc * (f(1.5) * r * r + f(3.0) * a * a + f(2.546479) * a * r)
        return np.stack([f(1.0) / mass, f(1.0) / inertia], axis=1).astype(np.float32)


def polygon_inverse_masses(vertices):
    """(2,) float32 {invMass, invInertia} of the convex polygon with the given (N, 2) body-local vertices, counter-clockwise, on AddBody's
    scale (include/phyx_amd.h POLYGONS): with the float64 shoelace area A and the second moment J about the origin,
    mass = 1e-5 * A / 4 and inertia = 3 * mass * J / A, both rounded to float32.  A rectangle's corners give the box formula."""
    v = np.asarray(vertices, dtype=np.float64).reshape(-1, 2)
    w = np.roll(v, -1, axis=0)
    c = v[:, 0] * w[:, 1] - w[:, 0] * v[:, 1]
    area = 0.5 * c.sum()
    second = (c * ((v * v).sum(axis=1) + (v * w).sum(axis=1) + (w * w).sum(axis=1))).sum() / 12.0
    mass = 1e-5 * area / 4.0
    inertia = 3.0 * mass * second / area
    f = np.float32
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        return np.array([f(1.0) / f(mass), f(1.0) / f(inertia)], dtype=np.float32)


def continuous_check(body, kind, hx, hy, rc, polygon=None, what="continuous_check"):
    """phx_continuous_check: raises PhxError unless rc is finite, >= 0 and (where above 0) strictly below the inradius of the shape
    {kind, hx, hy} (with `polygon`, an (N, 2) vertex list, for SHAPE_POLYGON); no device needed."""
    s = np.zeros(1, dtype=shape_dtype)
    s["kind"], s["hx"], s["hy"] = kind, hx, hy
    p = None if polygon is None else _polygons(polygon, 1, what)
    check(_lib.load().phx_continuous_check(what.encode(), int(body), _ptr(s), None if p is None else _ptr(p), float(np.float32(rc))))


def _polygons(polygons, count, what):
    """`count` phx_polygon records from an array of polygon_dtype, one (N, 2) vertex list for all bodies, or one vertex list per body."""
    if isinstance(polygons, np.ndarray) and polygons.dtype == polygon_dtype:
        p = np.ascontiguousarray(polygons).reshape(-1)
        if len(p) == 1 and count != 1:
            p = np.repeat(p, count)
        if len(p) != count:
            raise ValueError("%s: %d polygons for %d bodies" % (what, len(p), count))
        return p
    try:
        one = np.asarray(polygons, dtype=np.float32)
    except (ValueError, TypeError):
        one = None
    lists = [one] * count if one is not None and one.ndim == 2 else list(polygons)
    if len(lists) != count:
        raise ValueError("%s: %d polygons for %d bodies" % (what, len(lists), count))
    p = np.zeros(count, dtype=polygon_dtype)
    for k, v in enumerate(lists):
        if getattr(v, "dtype", None) == polygon_dtype:
            p[k] = v
            continue
        v = np.asarray(v, dtype=np.float32)
        if v.ndim != 2 or v.shape[1] != 2:
            raise ValueError("%s: polygon %d must have shape (N, 2), got %s" % (what, k, v.shape))
        p["count"][k] = len(v)                                              # (the library rejects a count outside 3 .. 8)
        p["v"][k][:min(len(v), POLYGON_MAX_VERTICES)] = v[:POLYGON_MAX_VERTICES]
    return p


def _or_empty(a, shape, dtype):
    """An empty list or tuple as the empty array it stands for ([] alone reads as float64)."""
    return np.zeros(shape, dtype=dtype) if isinstance(a, (list, tuple)) and not len(a) else a


def _contig(a, dtype):
    a = np.asarray(a)
    if a.dtype != dtype or not a.flags["C_CONTIGUOUS"]:
        raise TypeError("expected a C-contiguous array of dtype %s" % (dtype,))
    return a


def _field(kind, value, box, disc, mask, force):
    """One field_dtype row; the region is ALL unless `box` = (min.x, min.y, max.x, max.y) or `disc` = (c.x, c.y, r) is given."""
    if box is not None and disc is not None:
        raise ValueError("a field's region is a box or a disc, not both")
    f = np.zeros((), dtype=field_dtype)
    f["kind"], f["mask"], f["flags"] = kind, mask, FIELD_FORCE if force else 0
    f["value"][:len(value)] = value
    if box is not None:
        f["shape"], f["region"] = REGION_BOX, box
    elif disc is not None:
        f["shape"] = REGION_DISC
        f["region"][:3] = disc
    return f


def uniform_field(ax, ay, angular=0.0, box=None, disc=None, mask=0xFFFFFFFF, force=False):
    """A wind, a current, a zero-gravity room (ay = -gravity): the same acceleration {ax, ay, angular} for every body in the region
    (a force / torque with force=True: scaled by the body's inverse mass / inverse inertia)."""
    return _field(FIELD_UNIFORM, (ax, ay, angular), box, disc, mask, force)


def radial_field(cx, cy, strength, falloff_radius=0.0, box=None, disc=None, mask=0xFFFFFFFF, force=False):
    """A magnet, a planet, a blast: `strength` along the direction from (cx, cy) to the body (negative: toward the centre), fading
    linearly to nothing at falloff_radius where that is > 0."""
    return _field(FIELD_RADIAL, (cx, cy, strength, falloff_radius), box, disc, mask, force)


def drag_field(k_lin, k_ang=0.0, flow=(0.0, 0.0), box=None, disc=None, mask=0xFFFFFFFF, force=False):
    """A water volume, a conveyor current: the velocity is drawn toward `flow` at rate k_lin per second and the angular velocity
    toward 0 at k_ang, never past them in one step."""
    return _field(FIELD_DRAG, (flow[0], flow[1], k_lin, k_ang), box, disc, mask, force)


def _fields(fields, what):
    """A list of field_dtype rows (or one array of them) as one contiguous field_dtype array."""
    if isinstance(fields, np.ndarray):
        a = fields.reshape(-1) if fields.dtype == field_dtype else None
    else:
        rows = list(fields)
        a = np.zeros(len(rows), dtype=field_dtype)
        for k, r in enumerate(rows):
            r = np.asarray(r)
            if r.dtype != field_dtype or r.size != 1:
                a = None
                break
            a[k] = r.reshape(())
    if a is None:
        raise TypeError("%s: fields must be field_dtype rows (uniform_field, radial_field, drag_field)" % what)
    return np.ascontiguousarray(a)


def field_check(fields):
    """phx_field_check: raises PhxError naming the first rule a field of the list breaks (no device needed)."""
    f = _fields(fields, "field_check")
    check(_lib.load().phx_field_check(_ptr(f), len(f)))


def device_count():
    return check(_lib.load().phx_device_count())


def device_info(device=0):
    L = _lib.load()
    name = C.create_string_buffer(256)
    cu, lds, hbm = C.c_int(), C.c_int(), C.c_int64()
    check(L.phx_device_info(device, name, 256, C.byref(cu), C.byref(lds), C.byref(hbm)))
    return {"name": name.value.decode(), "compute_units": cu.value, "lds_bytes": lds.value, "hbm_bytes": hbm.value}


XCH_PEER_ERROR, XCH_SERIAL_MISMATCH, XCH_TOPOLOGY_MISMATCH, XCH_BAD_SEGMENT = 1, 2, 4, 8
XCH_HEADER_BYTES = 32


def exchange_layout(group_bodies, group_slots, shard_count):
    """Host-only: the deal of the groups to the ranks (longest processing time first by joint count) and the segment layout
    of the island-sharded exchange (include/phyx_amd.h: phx_exchange_layout) -> (group_offset_words, rank_words, segment_words,
    group_owner)."""
    L = _lib.load()
    gb = np.ascontiguousarray(group_bodies, dtype=np.int32)
    gs = np.ascontiguousarray(group_slots, dtype=np.int32)
    off = np.zeros(max(len(gb), 1), dtype=np.int64)
    own = np.zeros(max(len(gb), 1), dtype=np.int32)
    rw = np.zeros(max(shard_count, 1), dtype=np.int64)
    seg = C.c_int64(0)
    check(L.phx_exchange_layout(_ptr(gb), _ptr(gs), len(gb), shard_count, _ptr(own), _ptr(off), _ptr(rw), C.byref(seg)))
    return off[:len(gb)], rw, seg.value, own[:len(gb)]


def schedule_priority(priority_id, joint_index, lower_body=0):
    """Colouring priority of a joint (higher = coloured earlier); see include/phyx_amd.h."""
    return int(_lib.load().phx_schedule_priority(int(priority_id), int(joint_index), int(lower_body)))


def schedule_colours(body1, body2, is_static, priority_ids=None):
    """Host-only: colour classes of body-disjoint joints (this backend's PrepareIndices, ref: Solver.cpp:217-273).
    priority_ids: per-joint priority id (the solver uses contactPointIndex); the joint index if None."""
    L = _lib.load()
    pid = None if priority_ids is None else np.ascontiguousarray(priority_ids, dtype=np.int32)
    b1 = np.ascontiguousarray(body1, dtype=np.int32)
    b2 = np.ascontiguousarray(body2, dtype=np.int32)
    st = np.ascontiguousarray(is_static, dtype=np.uint8)
    order = np.zeros(max(len(b1), 1), dtype=np.int32)
    offs = np.zeros(len(b1) + 2, dtype=np.int32)
    nc = C.c_int32(0)
    check(L.phx_schedule_colours(_ptr(b1), _ptr(b2), len(b1), _ptr(st), len(st), None if pid is None else _ptr(pid), _ptr(order), _ptr(offs), len(offs), C.byref(nc)))
    return order[:len(b1)], offs[:nc.value + 1]


def schedule_groups(body1, body2, is_static, priority_ids=None, lanes=256, body_cap=768):
    """Host-only: the island-mode schedule as workgroup-sized LDS groups (include/phyx_amd.h phx_schedule_groups) -> dict with
    order, colour_offsets, group_offsets, group_first_colour, lds_groups, unit_lane, unit_leader_slot."""
    L = _lib.load()
    pid = None if priority_ids is None else np.ascontiguousarray(priority_ids, dtype=np.int32)
    b1 = np.ascontiguousarray(body1, dtype=np.int32)
    b2 = np.ascontiguousarray(body2, dtype=np.int32)
    st = np.ascontiguousarray(is_static, dtype=np.uint8)
    n = len(b1)
    order = np.zeros(max(n, 1), dtype=np.int32)
    offs = np.zeros(n + 2, dtype=np.int32)
    goff = np.zeros(n + 3, dtype=np.int32); gfc = np.zeros(n + 3, dtype=np.int32)
    ulane = np.zeros(max(n, 1), dtype=np.int32); uslot = np.zeros(max(n, 1), dtype=np.int32)
    nc = C.c_int32(0); lg = C.c_int32(0)
    nu = check(L.phx_schedule_groups(_ptr(b1), _ptr(b2), n, _ptr(st), len(st), None if pid is None else _ptr(pid), int(lanes), int(body_cap), _ptr(order), _ptr(offs),
                                     len(offs), C.byref(nc), _ptr(goff), _ptr(gfc), len(goff), C.byref(lg), _ptr(ulane), _ptr(uslot)))
    ng = lg.value + (1 if lg.value == 0 or goff[lg.value] < n else 0)
    return dict(order=order[:n], colour_offsets=offs[:nc.value + 1], lds_groups=lg.value, group_offsets=goff[:ng + 1], group_first_colour=gfc[:ng + 1],
                unit_lane=ulane[:nu], unit_leader_slot=uslot[:nu])


def pin_schedule(body1, body2, is_static, group_pins=256):
    """Host-only: the schedule of the pin pass (include/phyx_amd.h phx_pin_schedule; body2 = -1: the world) -> dict with order,
    class_offsets, group_offsets, lds_groups."""
    L = _lib.load()
    b1 = np.ascontiguousarray(body1, dtype=np.int32)
    b2 = np.ascontiguousarray(body2, dtype=np.int32)
    st = np.ascontiguousarray(is_static, dtype=np.uint8)
    n = len(b1)
    order = np.zeros(max(n, 1), dtype=np.int32)
    coff = np.zeros(n + 2, dtype=np.int32); goff = np.zeros(n + 2, dtype=np.int32)
    nc = C.c_int32(0); ng = C.c_int32(0); lg = C.c_int32(0)
    check(L.phx_pin_schedule(_ptr(b1), _ptr(b2), n, _ptr(st), len(st), int(group_pins), _ptr(order), _ptr(coff), len(coff), C.byref(nc),
                             _ptr(goff), len(goff), C.byref(ng), C.byref(lg)))
    return dict(order=order[:n], class_offsets=coff[:nc.value + 1], group_offsets=goff[:ng.value + 1], lds_groups=lg.value)


def schedule_islands(body1, body2, is_static):
    """Host-only: GatherIslands semantics (ref: Solver.cpp:285-454) -> (joint_island, island_size)."""
    L = _lib.load()
    b1 = np.ascontiguousarray(body1, dtype=np.int32)
    b2 = np.ascontiguousarray(body2, dtype=np.int32)
    st = np.ascontiguousarray(is_static, dtype=np.uint8)
    ji = np.zeros(max(len(b1), 1), dtype=np.int32)
    sz = np.zeros(len(b1) + 1, dtype=np.int32)
    n = check(L.phx_schedule_islands(_ptr(b1), _ptr(b2), len(b1), _ptr(st), len(st), _ptr(ji), _ptr(sz), len(sz)))
    return ji[:len(b1)], sz[:n]


class Configuration:
    """ref: Configuration.h:20-23; defaults are the demo's (main.cpp:262-263,348) with the scalar mode."""

    def __init__(self, solveMode=SOLVE_SCALAR, islandMode=ISLAND_SINGLE, contactIterationsCount=15, penetrationIterationsCount=15):
        self.solveMode = solveMode
        self.islandMode = islandMode
        self.contactIterationsCount = contactIterationsCount
        self.penetrationIterationsCount = penetrationIterationsCount

    def _c(self):
        return Config(self.solveMode, self.islandMode, self.contactIterationsCount, self.penetrationIterationsCount)


class DeviceBuffer:
    """A raw HBM allocation of `nbytes` (exchange buffers of a sharded solve when the caller has no torch tensors)."""

    def __init__(self, nbytes, device=0):
        self.L = _lib.load()
        self.device = device
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        check(self.L.phx_device_malloc(device, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p

    def address(self, offset=0):
        return C.c_void_p(self.ptr.value + int(offset))

    def to_host(self, nbytes=None, offset=0):
        n = self.nbytes - offset if nbytes is None else int(nbytes)
        out = np.zeros(n, dtype=np.uint8)
        if n:
            check(self.L.phx_memcpy_d2h(self.device, _ptr(out), self.address(offset), n))
        return out

    def from_host(self, data, offset=0):
        a = np.ascontiguousarray(data).view(np.uint8).reshape(-1)
        if len(a):
            check(self.L.phx_memcpy_h2d(self.device, self.address(offset), _ptr(a), len(a)))

    def copy_from(self, other, nbytes, dst_offset=0, src_offset=0, stream=None):
        """Device-to-device copy; with `stream` (a hipStream_t address) it is queued on that stream instead of blocking."""
        if not nbytes:
            return
        if stream is None:
            check(self.L.phx_memcpy_d2d(self.device, self.address(dst_offset), other.address(src_offset), int(nbytes)))
        else:
            check(self.L.phx_memcpy_d2d_on(self.device, self.address(dst_offset), other.address(src_offset), int(nbytes), C.c_void_p(int(stream))))

    def free(self):
        if self.ptr:
            self.L.phx_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceArray:
    """A raw HBM allocation holding a copy of a host array (inputs resident before a timed region)."""

    def __init__(self, host_array, device=0):
        self.L = _lib.load()
        self.device = device
        self.dtype = host_array.dtype
        self.count = len(host_array)
        self.nbytes = int(host_array.nbytes)
        p = C.c_void_p()
        check(self.L.phx_device_malloc(device, max(self.nbytes, 1), C.byref(p)))
        self.ptr = p
        if self.nbytes:
            check(self.L.phx_memcpy_h2d(device, self.ptr, _ptr(np.ascontiguousarray(host_array)), self.nbytes))

    def to_host(self):
        out = np.zeros(self.count, dtype=self.dtype)
        if self.nbytes:
            check(self.L.phx_memcpy_d2h(self.device, _ptr(out), self.ptr, self.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.L.phx_device_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Solver:
    """Device replacement of Solver (ref: Solver.h:47-128)."""

    def __init__(self, device=0, _handle=None):
        self.L = _lib.load()
        self.device = device
        self._owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            check(self.L.phx_solver_create(C.byref(h), device))
            self.h = h
        else:
            self.h = C.c_void_p(_handle)
        self.islandCount = 0
        self.islandMaxSize = 0

    def __del__(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            self.L.phx_solver_destroy(self.h)
            self.h = None

    def SolveJoints(self, bodies, contactPoints, contactJoints, configuration):
        """ref: Solver.h:54 — solves in place on the host arrays (velocities + accumulated impulses)."""
        b = _contig(bodies, rigid_body_dtype)
        cp = _contig(contactPoints, contact_point_dtype)
        j = _contig(contactJoints, contact_joint_dtype)
        cfg = configuration._c()
        check(self.L.phx_solver_solve(self.h, _ptr(b), len(b), _ptr(cp), len(cp), _ptr(j), len(j), C.byref(cfg)))
        st = self.stats()
        self.islandCount, self.islandMaxSize = st.island_count, st.island_max_size
        return st

    def SolveJointsDevice(self, d_bodies, d_contact_points, d_joints, configuration):
        cfg = configuration._c()
        check(self.L.phx_solver_solve_device(self.h, d_bodies.ptr, d_bodies.count, d_contact_points.ptr, d_contact_points.count,
                                             d_joints.ptr, d_joints.count, C.byref(cfg)))

    def synchronize(self):
        check(self.L.phx_solver_synchronize(self.h))

    def set_body_state_bits(self, bits):
        """32 = fp32 solver-side body state (default, the reference's); 16 = the fp16 ablation of BASELINE config 5."""
        check(self.L.phx_solver_set_body_state_bits(self.h, bits))

    def set_schedule_reuse(self, on):
        """False: rebuild the schedule on every solve (the reference rebuilds its grouping every call)."""
        check(self.L.phx_solver_set_schedule_reuse(self.h, 1 if on else 0))

    def set_trace(self, on=True, waves=True):
        """Phase stamps of the island kernel's workgroups (island_trace); waves=True also counts every wave's class-step cycles
        (wave_trace), which slows the sweeps by ~15 %."""
        check(self.L.phx_solver_set_trace(self.h, (2 if waves else 1) if on else 0))

    def island_trace(self):
        """(groups, 8) uint64: phase stamps of the island kernel's workgroups in the last solve (set_trace first)."""
        n = C.c_int32(0)
        check(self.L.phx_solver_get_island_trace(self.h, None, 0, C.byref(n)))
        out = np.zeros((max(n.value, 1), 8), dtype=np.uint64)
        check(self.L.phx_solver_get_island_trace(self.h, _ptr(out), n.value, C.byref(n)))
        return out[:n.value]

    def wave_trace(self):
        """(groups, waves, 8) uint64: per-wave colour-step cycles of the last traced solve."""
        n, w = C.c_int32(0), C.c_int32(0)
        check(self.L.phx_solver_get_island_trace(self.h, None, 0, C.byref(n)))
        check(self.L.phx_solver_get_wave_trace(self.h, None, 0, C.byref(w)))
        out = np.zeros((max(n.value, 1), w.value, 8), dtype=np.uint64)
        check(self.L.phx_solver_get_wave_trace(self.h, _ptr(out), out.size, C.byref(w)))
        return out[:n.value]

    def phase_trace(self):
        """(groups, words) uint64: the island kernel's finer phase stamps and, with waves=True, where a working wave's class step goes
        (include/phyx_amd.h phx_solver_get_phase_trace)."""
        n, w = C.c_int32(0), C.c_int32(0)
        check(self.L.phx_solver_get_island_trace(self.h, None, 0, C.byref(n)))
        check(self.L.phx_solver_get_phase_trace(self.h, None, 0, C.byref(w)))
        out = np.zeros((max(n.value, 1), w.value), dtype=np.uint64)
        check(self.L.phx_solver_get_phase_trace(self.h, _ptr(out), out.size, C.byref(w)))
        return out[:n.value]

    def set_shard(self, shard, shard_count):
        """Sweep only the schedule groups g with g % shard_count == shard (multi-GPU island sharding)."""
        check(self.L.phx_solver_set_shard(self.h, shard, shard_count))

    # ---- island-sharded solves: the post-solve exchange (include/phyx_amd.h: phx_solver_exchange_pack) ----
    def set_comm(self, comm):
        """bench(): the all-gather between pack and unpack runs natively on the solver's stream (no step hook needed)."""
        self._comm = comm
        check(self.L.phx_solver_set_comm(self.h, comm.h if comm is not None else None))

    def set_exchange_buffers(self, send_ptr, recv_ptr, segment_capacity_bytes):
        """Caller-owned device buffers (raw addresses): one segment to send, shard_count segments to receive."""
        check(self.L.phx_solver_set_exchange_buffers(self.h, C.c_void_p(int(send_ptr)), C.c_void_p(int(recv_ptr)), int(segment_capacity_bytes)))

    def exchange_pack(self, d_bodies, d_joints, status_word=0):
        seg = C.c_size_t(0)
        check(self.L.phx_solver_exchange_pack(self.h, d_bodies.ptr, d_joints.ptr, int(status_word), C.byref(seg)))
        return seg.value

    def exchange_unpack(self, d_bodies, d_joints):
        check(self.L.phx_solver_exchange_unpack(self.h, d_bodies.ptr, d_joints.ptr))

    def exchange_status(self):
        v = C.c_int32(0)
        check(self.L.phx_solver_exchange_status(self.h, C.byref(v)))
        return v.value

    def exchange_segment_bytes(self):
        return int(self.L.phx_solver_exchange_segment_bytes(self.h))

    def stats(self):
        st = SolveStats()
        check(self.L.phx_solver_get_stats(self.h, C.byref(st)))
        return st

    def schedule(self):
        """(order, colour_offsets) of the last solve: order[k] = joint in slot k."""
        nc = C.c_int32(0)
        check(self.L.phx_solver_get_schedule(self.h, None, 0, None, 0, C.byref(nc)))
        offs = np.zeros(nc.value + 1, dtype=np.int32)
        check(self.L.phx_solver_get_schedule(self.h, None, 0, _ptr(offs), len(offs), C.byref(nc)))
        order = np.zeros(max(int(offs[-1]), 1), dtype=np.int32)
        check(self.L.phx_solver_get_schedule(self.h, _ptr(order), len(order), _ptr(offs), len(offs), C.byref(nc)))
        return order[:int(offs[-1])], offs

    def groups(self):
        """(group_offsets, lds_group_count) of the last solve's schedule."""
        n, lds = C.c_int32(0), C.c_int32(0)
        check(self.L.phx_solver_get_groups(self.h, None, 0, C.byref(n), C.byref(lds)))
        offs = np.zeros(n.value + 1, dtype=np.int32)
        check(self.L.phx_solver_get_groups(self.h, _ptr(offs), len(offs), C.byref(n), C.byref(lds)))
        return offs, lds.value

    def lanes(self):
        """(leader_slot, lane) per unit of the last solve's LDS groups (phx_solver_get_lanes)."""
        n = C.c_int32(0)
        check(self.L.phx_solver_get_lanes(self.h, None, None, 0, C.byref(n)))
        slot = np.zeros(max(n.value, 1), dtype=np.int32); lane = np.zeros(max(n.value, 1), dtype=np.int32)
        check(self.L.phx_solver_get_lanes(self.h, _ptr(slot), _ptr(lane), len(slot), C.byref(n)))
        return slot[:n.value], lane[:n.value]

    def partition(self):
        """(interior_classes, parts, sweep_launches) of the last solve: the partitioned-component path (phx_solver_get_partition)."""
        ki, parts, launches = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        check(self.L.phx_solver_get_partition(self.h, C.byref(ki), C.byref(parts), C.byref(launches)))
        return ki.value, parts.value, launches.value

    def refreshed(self, joint_index):
        out = np.zeros(30, dtype=np.float32)
        check(self.L.phx_solver_get_refreshed(self.h, joint_index, _ptr(out)))
        return out

    def bench_stage(self, d_bodies, d_joints, steps):
        """Make `steps` private copies of the input in HBM NOW (before the caller starts its clock): the next bench() call on the same
        arrays solves copy k in step k instead of restoring a working copy in front of every step."""
        check(self.L.phx_solver_bench_stage(self.h, d_bodies.ptr, d_bodies.count, d_joints.ptr, d_joints.count, steps))

    def bench_checksum(self):
        """64-bit checksum of the results of the last bench() step (velocities, displacing velocities, impulses)."""
        out = C.c_uint64(0)
        check(self.L.phx_solver_bench_checksum(self.h, C.byref(out)))
        return int(out.value)

    def bench(self, d_bodies, d_contact_points, d_joints, configuration, warmup, steps, hook=None):
        """`steps` solves of the same resident input, queued back to back.  hook(step, phase) (optional) runs on the host:
        phase 0 after step `step` has been queued (start the per-step exchange on stream_ptr()), phase 1 when the local
        preparation of step `step` is queued and its sweeps are not (make the stream wait for the previous exchange)."""
        cfg = configuration._c()
        res = BenchResult()
        if hook is None:
            check(self.L.phx_solver_bench(self.h, d_bodies.ptr, d_bodies.count, d_contact_points.ptr, d_contact_points.count,
                                          d_joints.ptr, d_joints.count, C.byref(cfg), warmup, steps, C.byref(res)))
            return res
        failure = []

        def _trampoline(_user, step, phase):
            try:
                hook(int(step), int(phase))
                return 0
            except BaseException as e:          # an exception must not unwind through the C frames
                failure.append(e)
                return 1
        cb = _lib.STEP_HOOK(_trampoline)
        st = self.L.phx_solver_bench_hooked(self.h, d_bodies.ptr, d_bodies.count, d_contact_points.ptr, d_contact_points.count,
                                            d_joints.ptr, d_joints.count, C.byref(cfg), warmup, steps, cb, None, C.byref(res))
        if failure:
            raise failure[0]
        check(st)
        return res

    def stream_ptr(self):
        """The hipStream_t (as an int) all of this handle's work is queued on."""
        return int(self.L.phx_solver_stream(self.h) or 0)


class Comm:
    """Native RCCL communicator (csrc/comm.hip): one per process / GPU.  `unique_id()` on rank 0, hand the 128 bytes to every
    rank out of band, then every rank constructs Comm(id, rank, nranks, device) — a collective call."""

    ID_BYTES = 128

    @staticmethod
    def unique_id():
        L = _lib.load()
        buf = C.create_string_buffer(Comm.ID_BYTES)
        check(L.phx_comm_unique_id(buf))
        return buf.raw

    @staticmethod
    def rccl_version():
        """ncclGetVersion of the RCCL the library resolved (0: none)"""
        return int(_lib.load().phx_comm_rccl_version())

    def __init__(self, unique_id, rank, nranks, device=0):
        self.L = _lib.load()
        assert len(unique_id) == Comm.ID_BYTES
        h = C.c_void_p()
        check(self.L.phx_comm_create(C.byref(h), C.c_char_p(bytes(unique_id)), rank, nranks, device))
        self.h = h
        self.rank, self.size, self.device = rank, nranks, device

    def __del__(self):
        h = getattr(self, "h", None)
        if h is not None and h.value:
            self.L.phx_comm_destroy(h)
            self.h = C.c_void_p()

    def all_gather(self, send_ptr, recv_ptr, bytes_per_rank, stream_ptr):
        check(self.L.phx_comm_all_gather(self.h, C.c_void_p(send_ptr), C.c_void_p(recv_ptr), bytes_per_rank, C.c_void_p(stream_ptr)))

    def barrier(self, stream_ptr=0):
        check(self.L.phx_comm_barrier(self.h, C.c_void_p(stream_ptr)))

    def barrier_async(self, stream_ptr):
        check(self.L.phx_comm_barrier_async(self.h, C.c_void_p(stream_ptr)))

    def async_error(self):
        e = C.c_int32(0)
        check(self.L.phx_comm_async_error(self.h, C.byref(e)))
        return e.value


class Collider:
    """Device replacement of the broadphase half of Collider (ref: Collider.h:28-29, 58-66)."""

    def __init__(self, device=0, _handle=None):
        self.L = _lib.load()
        self._owned = _handle is None
        if _handle is None:
            h = C.c_void_p()
            check(self.L.phx_broadphase_create(C.byref(h), device))
            self.h = h
        else:
            self.h = C.c_void_p(_handle)

    def __del__(self):
        if getattr(self, "_owned", False) and getattr(self, "h", None):
            self.L.phx_broadphase_destroy(self.h)
            self.h = None

    def clear(self):
        check(self.L.phx_broadphase_clear(self.h))

    def UpdateBroadphaseAndPairs(self, bodies):
        """UpdateBroadphase + UpdatePairs; returns the pairs that were new this step, (n,2) uint32 in the
        reference's serial emission order; they are now part of the persistent set."""
        b = _contig(bodies, rigid_body_dtype)
        n = C.c_int32(0)
        check(self.L.phx_broadphase_update(self.h, _ptr(b), len(b), None, 0, C.byref(n)))
        pairs = np.zeros((max(n.value, 1), 2), dtype=np.uint32)
        check(self.L.phx_broadphase_get_new_pairs(self.h, _ptr(pairs), n.value, C.byref(n)))
        return pairs[:n.value]

    def sorted(self, n):
        srt = np.zeros(n, dtype=sort_entry_dtype)
        ent = np.zeros(n, dtype=broadphase_entry_dtype)
        check(self.L.phx_broadphase_get_sorted(self.h, _ptr(srt), _ptr(ent), n))
        return srt, ent

    def erase(self, pairs):
        p = np.ascontiguousarray(pairs, dtype=np.uint32).reshape(-1, 2)
        check(self.L.phx_broadphase_erase_pairs(self.h, _ptr(p), len(p)))

    def stats(self):
        st = BroadphaseStats()
        check(self.L.phx_broadphase_get_stats(self.h, C.byref(st)))
        return st


class Snapshot:
    """A saved world in device memory (phx_snapshot): filled by World.save or from_bytes, emptied into any world of its device by
    World.load, as often as wanted.  Its memory grows geometrically and is reused by every save."""

    def __init__(self, device=0):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.phx_snapshot_create(C.byref(h), device))
        self.h = h
        self.device = device

    def __del__(self):
        if getattr(self, "h", None):
            self.L.phx_snapshot_destroy(self.h)
            self.h = None

    @property
    def counts(self):
        """(bodies, manifolds, contact points, joints) of the saved world."""
        v = [C.c_int32() for _ in range(4)]
        check(self.L.phx_snapshot_counts(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def to_bytes(self):
        """The snapshot as one versioned blob (phx_snapshot_export): the form for disk or another machine."""
        n = C.c_size_t(0)
        check(self.L.phx_snapshot_blob_bytes(self.h, C.byref(n)))
        buf = C.create_string_buffer(n.value)
        check(self.L.phx_snapshot_export(self.h, buf, n.value))
        return buf.raw

    @classmethod
    def from_bytes(cls, blob, device=0):
        """A snapshot filled from a blob (phx_snapshot_import); the blob is checked completely first (PhxError if it is not valid)."""
        snap = cls(device)
        blob = bytes(blob)
        check(snap.L.phx_snapshot_import(snap.h, blob, len(blob)))
        return snap

    @staticmethod
    def check_bytes(blob):
        """phx_snapshot_blob_check on the host: raises PhxError naming the first violated rule."""
        blob = bytes(blob)
        check(_lib.load().phx_snapshot_blob_check(blob, len(blob)))

    @staticmethod
    def pack(bodies, manifolds, contact_points, joints, filters=None, materials=None, flags=None, baseline=None):
        """phx_snapshot_blob_pack on the host: a blob from what the getters return.  A column left None is the default for every body;
        baseline: (T, 2) int32 pairs sorted by (body1, body2), or None for the touching pairs of the manifolds."""
        L = _lib.load()
        b = np.ascontiguousarray(bodies, dtype=rigid_body_dtype); m = np.ascontiguousarray(manifolds, dtype=manifold_dtype)
        c = np.ascontiguousarray(contact_points, dtype=contact_point_dtype); j = np.ascontiguousarray(joints, dtype=contact_joint_dtype)
        f = None if filters is None else np.ascontiguousarray(filters, dtype=collision_filter_dtype)
        mt = None if materials is None else np.ascontiguousarray(materials, dtype=material_dtype)
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32)
        for name, col in (("filters", f), ("materials", mt), ("flags", fl)):
            if col is not None and col.shape != (len(b),):
                raise ValueError("Snapshot.pack: %s must have one entry per body" % name)
        base = None if baseline is None else np.ascontiguousarray(baseline, dtype=np.int32).reshape(-1, 2)
        args = (_ptr(b), len(b), _ptr(m), len(m), _ptr(c), len(c), _ptr(j), len(j), _ptr(f), _ptr(mt), _ptr(fl),
                _ptr(base), 0 if base is None else len(base))
        n = C.c_size_t(0)
        st = L.phx_snapshot_blob_pack(*args, None, 0, C.byref(n))
        if st != _lib.PHX_ERR_CAPACITY:
            check(st)
        buf = C.create_string_buffer(max(n.value, 1))
        check(L.phx_snapshot_blob_pack(*args, buf, n.value, C.byref(n)))
        return buf.raw[:n.value]


class World:
    """Device-backed World (ref: World.h:9-36)."""

    PHASES = ("IntegrateVelocity", "UpdateBroadphase", "UpdatePairs", "UpdateManifolds", "PackManifolds",
              "RefreshContactJoints", "SolveJoints", "IntegratePosition")

    def __init__(self, device=0, gravity=0.0):
        self.L = _lib.load()
        h = C.c_void_p()
        check(self.L.phx_world_create(C.byref(h), device))
        self.h = h
        self.device = device
        self.gravity = gravity
        self.solver = Solver(device, _handle=self.L.phx_world_solver(self.h))
        self.collider = Collider(device, _handle=self.L.phx_world_broadphase(self.h))

    def __del__(self):
        if getattr(self, "h", None):
            self.L.phx_world_destroy(self.h)
            self.h = None

    @property
    def gravity(self):
        return self._gravity

    @gravity.setter
    def gravity(self, g):
        self._gravity = float(g)
        check(self.L.phx_world_set_gravity(self.h, self._gravity))

    def AddBody(self, pos, angle, size, static=False):
        """ref: World.cpp:11-17 — pos=(x,y), size = half extents; returns the body index."""
        i = check(self.L.phx_world_add_body(self.h, pos[0], pos[1], angle, size[0], size[1]))
        if static:
            check(self.L.phx_world_set_body_static(self.h, i))
        return i

    def set_inverse_mass(self, body, inv_mass, inv_inertia):
        """body->invMass / invInertia (the demo pins shelves with invMass = 0 only, ref: main.cpp:176-177)."""
        check(self.L.phx_world_set_body_inverse_mass(self.h, int(body), float(inv_mass), float(inv_inertia)))

    def add_scene(self, scene):
        pinned = scene.get("pinned")                 # invMass = 0 only: infinitely heavy but free to rotate
        for k in range(len(scene["px"])):
            i = self.AddBody((float(scene["px"][k]), float(scene["py"][k])), float(scene["angle"][k]),
                             (float(scene["sx"][k]), float(scene["sy"][k])), bool(scene["static"][k]))
            if pinned is not None and pinned[k]:
                self.set_inverse_mass(i, 0.0, pinned_inv_inertia(scene["sx"][k], scene["sy"][k]))

    def set_shard(self, shard, shard_count):
        check(self.L.phx_world_set_shard(self.h, shard, shard_count))

    def Update(self, dt, configuration):
        cfg = configuration._c()
        check(self.L.phx_world_update(self.h, dt, C.byref(cfg)))

    def StepBegin(self, dt, configuration):
        """First half of a SHARDED world's step: everything up to and including SolveJoints of this rank's groups, then
        the pack.  Returns the segment size in bytes every rank must all-gather (send buffer -> recv buffer)."""
        cfg = configuration._c()
        seg = C.c_size_t(0)
        check(self.L.phx_world_step_begin(self.h, dt, C.byref(cfg), C.byref(seg)))
        return seg.value

    def StepEnd(self, dt):
        """Second half: scatter the other ranks' results, IntegratePosition."""
        check(self.L.phx_world_step_end(self.h, dt))

    def set_comm(self, comm):
        """Attach a native communicator (Comm): this world becomes rank comm.rank of comm.size and owns its exchange buffers."""
        self._comm = comm
        check(self.L.phx_world_set_comm(self.h, comm.h if comm is not None else None))

    def StepSharded(self, dt, configuration):
        """World::Update of a sharded world in one library call: step_begin, ncclAllGather on the world's stream, step_end."""
        cfg = configuration._c()
        check(self.L.phx_world_step_sharded(self.h, dt, C.byref(cfg)))

    def check_exchange(self):
        check(self.L.phx_world_check_exchange(self.h))

    def stream_ptr(self):
        return int(self.L.phx_world_stream(self.h) or 0)

    def PreSolve(self, dt):
        """Everything of World::Update that precedes Solver::SolveJoints (ref: World.cpp:25-32)."""
        check(self.L.phx_world_pre_solve(self.h, dt))

    def FinishStep(self, dt, configuration):
        """Solver::SolveJoints + IntegratePosition (ref: World.cpp:34-36)."""
        cfg = configuration._c()
        check(self.L.phx_world_finish_step(self.h, dt, C.byref(cfg)))

    def counts(self):
        v = [C.c_int32() for _ in range(4)]
        check(self.L.phx_world_counts(self.h, *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def _get(self, fn, dtype, n):
        out = np.zeros(n, dtype=dtype)
        check(fn(self.h, _ptr(out), n))
        return out

    @property
    def bodies(self):
        return self._get(self.L.phx_world_get_bodies, rigid_body_dtype, self.counts()[0])

    @property
    def manifolds(self):
        return self._get(self.L.phx_world_get_manifolds, manifold_dtype, self.counts()[1])

    @property
    def contactPoints(self):
        return self._get(self.L.phx_world_get_contact_points, contact_point_dtype, self.counts()[2])

    @property
    def contactJoints(self):
        return self._get(self.L.phx_world_get_joints, contact_joint_dtype, self.counts()[3])

    def state(self):
        """(bodies, manifolds, contact points, joints): everything a world carries from one step to the next."""
        return self.bodies, self.manifolds, self.contactPoints, self.contactJoints

    def set_state(self, bodies, manifolds, contact_points, joints):
        """Restore a saved state() (phx_world_set_state): the world then steps exactly like the one the state was taken from."""
        b = np.ascontiguousarray(bodies, dtype=rigid_body_dtype); m = np.ascontiguousarray(manifolds, dtype=manifold_dtype)
        c = np.ascontiguousarray(contact_points, dtype=contact_point_dtype); j = np.ascontiguousarray(joints, dtype=contact_joint_dtype)
        check(self.L.phx_world_set_state(self.h, _ptr(b), len(b), _ptr(m), len(m), _ptr(c), len(c), _ptr(j), len(j)))

    # ---- snapshots (include/phyx_amd.h SNAPSHOTS; the blob's specification: tests/snapshot_spec.py) ----
    def save(self, snap=None):
        """snap := this world (phx_world_save), queued on the world's stream; a new Snapshot on the world's device when none is given.
        Returns the snapshot.  It holds the state and the per-body columns (the shapes' kinds among them), not settings such as gravity."""
        if snap is None:
            snap = Snapshot(self.device)
        check(self.L.phx_world_save(self.h, snap.h))
        return snap

    def load(self, snap):
        """This world := snap (phx_world_load): exactly what set_state of the saved arrays, the three column setters and the saved
        touch-event baseline would have made of it.  snap is unchanged; gravity and every other setting of this world stay."""
        check(self.L.phx_world_load(self.h, snap.h))

    def fork(self):
        """A new world on the same device with the same gravity, loaded from a fresh save of this one: both step identically from here."""
        other = World(self.device, self.gravity)
        other.load(self.save())
        return other

    # ---- edits and gathers between steps (include/phyx_amd.h: phx_world_add_accelerations ...) ----
    def _indices(self, bodies, what):
        idx = np.asarray(_or_empty(bodies, 0, np.int32))
        if idx.ndim != 1 or idx.dtype.kind not in "iu":
            raise TypeError("%s: body indices must be a 1-D integer array, got %s of shape %s" % (what, idx.dtype, idx.shape))
        if idx.size and (idx.min() < np.iinfo(np.int32).min or idx.max() > np.iinfo(np.int32).max):
            raise ValueError("%s: body index out of the int32 range" % what)
        return np.ascontiguousarray(idx, dtype=np.int32)

    def _values(self, values, count, width, what):
        v = np.asarray(values)
        if v.dtype.kind != "f":
            raise TypeError("%s: values must be a float array, got %s" % (what, v.dtype))
        if v.shape != (count, width):
            raise ValueError("%s: values must have shape (%d, %d), got %s" % (what, count, width, v.shape))
        return np.ascontiguousarray(v, dtype=np.float32)

    def _edit(self, fn, bodies, values, width, what):
        idx = self._indices(bodies, what)
        v = self._values(values, len(idx), width, what)
        check(getattr(self.L, fn)(self.h, _ptr(idx), _ptr(v), len(idx)))

    def add_accelerations(self, bodies, accel):
        """acceleration += accel[k] on body bodies[k]: accel is (K, 3) {ax, ay, angular} (ref: main.cpp:343-346).  The next Update's
        IntegrateVelocity consumes them; until then they show in the records."""
        self._edit("phx_world_add_accelerations", bodies, accel, 3, "add_accelerations")

    def set_velocities(self, bodies, vel):
        """velocity, angularVelocity = vel[k] {vx, vy, angular} on body bodies[k]."""
        self._edit("phx_world_set_velocities", bodies, vel, 3, "set_velocities")

    def set_poses(self, bodies, poses):
        """Move bodies (ref: RigidBody.h:38-42: coords, then UpdateGeom).  poses: (K, 6) frames {pos.x, pos.y, xv.x, xv.y, yv.x, yv.y},
        or (K, 3) {pos.x, pos.y, angle}, turned into a frame by the float formula of AddBody (ref: RigidBody.h:15-36, Coords2.h:10-17)."""
        p = np.asarray(poses)
        if p.ndim == 2 and p.shape[1] == 3:
            p = self._values(p, p.shape[0], 3, "set_poses")
            p = np.stack([frame_from_angle(x, y, a) for x, y, a in p]) if len(p) else np.zeros((0, 6), dtype=np.float32)
        self._edit("phx_world_set_poses", bodies, p, 6, "set_poses")

    def body_states(self, bodies):
        """The 128-byte records of the listed bodies, equal to bodies[bodies] byte for byte, at O(len(bodies)) cost."""
        idx = self._indices(bodies, "body_states")
        out = np.zeros(len(idx), dtype=rigid_body_dtype)
        check(self.L.phx_world_get_body_states(self.h, _ptr(idx), len(idx), _ptr(out)))
        return out

    def poses(self, out=None):
        """(N, 4) float32 {pos.x, pos.y, xv.x, xv.y} of every body (16 B per body instead of the 128-byte record)."""
        n = self.counts()[0]
        if out is None:
            out = np.zeros((n, 4), dtype=np.float32)
        elif not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.shape != (n, 4) or not out.flags.c_contiguous:
            raise ValueError("poses: out must be a C-contiguous float32 array of shape (%d, 4)" % n)
        check(self.L.phx_world_get_poses(self.h, _ptr(out), n))
        return out

    def poses_device(self, ptr, cap=None):
        """The same into device memory at `ptr` (16-byte aligned, room for `cap` bodies, default all of them), queued on the world's
        stream (stream_ptr()); e.g. a torch tensor's data_ptr()."""
        n = self.counts()[0]
        check(self.L.phx_world_get_poses_device(self.h, C.c_void_p(int(ptr)), n if cap is None else int(cap)))

    # ---- removal between steps (include/phyx_amd.h: phx_world_remove_bodies / phx_world_remove_outside) ----
    def remove_bodies(self, bodies):
        """Remove the listed bodies (each at most once) and compact the world on the device; exactly what set_state of the filtered
        state() would make (tests/removal_spec.py).  Returns remap: int32 of the old body count, remap[i] = body i's new index or -1.
        Indices held elsewhere shift (the drag's body 1 becomes remap[1])."""
        idx = self._indices(bodies, "remove_bodies")
        remap = np.zeros(self.counts()[0], dtype=np.int32)
        check(self.L.phx_world_remove_bodies(self.h, _ptr(idx), len(idx), _ptr(remap)))
        return remap

    def remove_outside(self, box):
        """Remove every body whose AABB does not overlap the closed box (min.x, min.y, max.x, max.y), tested on the device.
        Returns (removed, remap) as remove_bodies."""
        b = np.asarray(box)
        if b.shape != (4,) or b.dtype.kind not in "iuf":
            raise TypeError("remove_outside: box must be 4 numbers (min.x, min.y, max.x, max.y), got %s of shape %s" % (b.dtype, b.shape))
        with np.errstate(over="ignore"):
            b = np.ascontiguousarray(b, dtype=np.float32)      # (a box beyond the float range becomes infinite: refused below)
        if not np.isfinite(b).all() or b[0] > b[2] or b[1] > b[3]:
            raise ValueError("remove_outside: the box must be finite with min <= max, got %s" % (b.tolist(),))
        remap = np.zeros(self.counts()[0], dtype=np.int32)
        removed = C.c_int32(0)
        check(self.L.phx_world_remove_outside(self.h, _ptr(b), C.byref(removed), _ptr(remap)))
        return removed.value, remap

    # ---- spawn between steps (include/phyx_amd.h: phx_world_add_bodies / phx_world_set_inverse_masses) ----
    def add_bodies(self, spawn):
        """Append bodies, each exactly the record AddBody would make, on the device without a state round trip.  spawn: a (K, 5) float
        array {px, py, angle, half_x, half_y}, or a scenes.py dict (px, py, angle, sx, sy; optional static, pinned — applied through
        set_inverse_masses as add_scene applies them).  Returns the new bodies' indices, np.arange(first, first + K)."""
        flags = None
        if isinstance(spawn, dict):
            try:
                cols = [np.asarray(spawn[k]) for k in ("px", "py", "angle", "sx", "sy")]
            except KeyError as e:
                raise ValueError("add_bodies: the scene dict has no %s" % (e,))
            if any(c.ndim != 1 or c.dtype.kind not in "iuf" for c in cols):
                raise TypeError("add_bodies: the scene's px, py, angle, sx, sy must be 1-D numeric arrays")
            if len({len(c) for c in cols}) != 1:
                raise ValueError("add_bodies: the scene's px, py, angle, sx, sy differ in length")
            k = len(cols[0])
            static = np.asarray(spawn.get("static", np.zeros(k, dtype=bool)), dtype=bool)
            pinned = np.asarray(spawn.get("pinned", np.zeros(k, dtype=bool)), dtype=bool)
            if static.shape != (k,) or pinned.shape != (k,):
                raise ValueError("add_bodies: static / pinned must have one entry per body")
            s = np.ascontiguousarray(np.stack(cols, axis=1), dtype=np.float32) if k else np.zeros((0, 5), dtype=np.float32)
            flags = (static, pinned)
        else:
            a = np.asarray(spawn)
            if a.dtype.kind != "f":
                raise TypeError("add_bodies: spawn must be a float array, got %s" % (a.dtype,))
            if a.ndim != 2 or a.shape[1] != 5:
                raise ValueError("add_bodies: spawn must have shape (K, 5) {px, py, angle, half_x, half_y}, got %s" % (a.shape,))
            s = np.ascontiguousarray(a, dtype=np.float32)
        first = C.c_int32(0)
        check(self.L.phx_world_add_bodies(self.h, _ptr(s), len(s), C.byref(first)))
        idx = np.arange(first.value, first.value + len(s), dtype=np.int64)
        if flags is not None and (flags[0].any() or flags[1].any()):
            static, pinned = flags
            sel = np.flatnonzero(static | pinned)
            vals = np.zeros((len(sel), 2), dtype=np.float32)
            for r, k in enumerate(sel):              # (pinned after static, as add_scene applies them)
                if pinned[k]:
                    vals[r, 1] = pinned_inv_inertia(s[k, 3], s[k, 4])
            self.set_inverse_masses(idx[sel], vals)
        return idx

    def set_inverse_masses(self, bodies, values):
        """invMass, invInertia = values[k] on body bodies[k], values (K, 2) ((0, 0): static).  Like set_inverse_mass, a topology change:
        the next step rebuilds the solver's schedule."""
        self._edit("phx_world_set_inverse_masses", bodies, values, 2, "set_inverse_masses")

    # ---- units: pins, links, angles and sliders (include/phyx_amd.h PINS, LINKS, ANGLES, SLIDERS; the specifications: tests/pin_spec.py, link_spec.py, angle_spec.py, slider_spec.py) ----
    def _add_units(self, fn, recs, dtype, extra=(), required=0, anchors=True):
        """recs: an array of `dtype`, or rows (body1, body2, anchor1, anchor2 (unless the record has no `anchors`), then the fields
        `extra`, the first `required` of them always); the rest of a record is zero."""
        if isinstance(recs, np.ndarray) and recs.dtype == dtype:
            p = np.ascontiguousarray(recs)
        else:
            rows = list(recs)
            p = np.zeros(len(rows), dtype=dtype)
            for k, r in enumerate(rows):
                p["body1"][k], p["body2"][k] = int(r[0]), int(r[1])
                if anchors:
                    p["anchor1"][k], p["anchor2"][k] = r[2], r[3]
                at = 4 if anchors else 2
                for i, name in enumerate(extra):
                    if i < required or len(r) > at + i:
                        p[name][k] = r[at + i]
        first = C.c_int32(0)
        check(getattr(self.L, fn)(self.h, _ptr(p), len(p), C.byref(first)))
        return np.arange(first.value, first.value + len(p), dtype=np.int64)

    def _remove_units(self, fn, which, what):
        idx = self._indices(which, what)
        check(getattr(self.L, fn)(self.h, _ptr(idx), len(idx)))

    def _int32(self, fn):
        n = C.c_int32(0)
        check(getattr(self.L, fn)(self.h, C.byref(n)))
        return n.value

    def add_pins(self, pins):
        """Append pins: a pin_dtype array, or rows (body1, body2, (a1x, a1y), (a2x, a2y)) with impulse 0.  body2 = -1 pins body1 to the
        world point anchor2.  Returns the new pins' indices."""
        return self._add_units("phx_world_add_pins", pins, pin_dtype)

    def remove_pins(self, pins):
        """Remove the listed pins (each at most once); the others keep their order, so their indices shift."""
        self._remove_units("phx_world_remove_pins", pins, "remove_pins")

    def set_pin_anchors(self, pins, anchors):
        """anchor1, anchor2 = anchors[k] {a1.x, a1.y, a2.x, a2.y} of pin pins[k]; the schedule stays (a dragged body's world pin
        follows the cursor this way)."""
        self._edit("phx_world_set_pin_anchors", pins, anchors, 4, "set_pin_anchors")

    def pin_count(self):
        return self._int32("phx_world_pin_count")

    def pins(self):
        """Every pin as a pin_dtype array, with the impulses the last step accumulated."""
        return self._get(self.L.phx_world_get_pins, pin_dtype, self.pin_count())

    @property
    def pin_iterations(self):
        return self._int32("phx_world_get_pin_iterations")

    @pin_iterations.setter
    def pin_iterations(self, n):
        check(self.L.phx_world_set_pin_iterations(self.h, int(n)))

    def pin_schedule(self):
        """The schedule the next step's pin pass uses (built now unless current) -> dict with order, class_offsets, group_offsets,
        lds_groups, as api.pin_schedule.  The slots hold units: the pins, then the links, then the angles, then the sliders."""
        nc = C.c_int32(0); ng = C.c_int32(0); lg = C.c_int32(0)
        check(self.L.phx_world_get_pin_schedule(self.h, None, 0, None, 0, C.byref(nc), None, 0, C.byref(ng), C.byref(lg)))
        n = self.pin_count() + self.link_count() + self.angle_count() + self.slider_count()
        order = np.zeros(max(n, 1), dtype=np.int32)
        coff = np.zeros(nc.value + 1, dtype=np.int32); goff = np.zeros(ng.value + 1, dtype=np.int32)
        check(self.L.phx_world_get_pin_schedule(self.h, _ptr(order), n, _ptr(coff), len(coff), C.byref(nc), _ptr(goff), len(goff), C.byref(ng), C.byref(lg)))
        return dict(order=order[:n], class_offsets=coff, group_offsets=goff, lds_groups=lg.value)

    def pin_schedule_builds(self):
        n = C.c_int64(0)
        check(self.L.phx_world_pin_schedule_builds(self.h, C.byref(n)))
        return n.value

    def add_links(self, links):
        """Append links: a link_dtype array, or rows (body1, body2, (a1x, a1y), (a2x, a2y), min_length, max_length[, hertz[, damping_ratio]])
        with impulse 0.  min == max: a rod, with hertz > 0 a spring; min < max: limits (a rope: min = 0).  Returns the new links' indices."""
        return self._add_units("phx_world_add_links", links, link_dtype, ("min_length", "max_length", "hertz", "damping_ratio"), required=2)

    def remove_links(self, links):
        """Remove the listed links (each at most once); the others keep their order, so their indices shift."""
        self._remove_units("phx_world_remove_links", links, "remove_links")

    def set_link_anchors(self, links, anchors):
        """anchor1, anchor2 = anchors[k] {a1.x, a1.y, a2.x, a2.y} of link links[k]; the schedule stays (a spring to the cursor)."""
        self._edit("phx_world_set_link_anchors", links, anchors, 4, "set_link_anchors")

    def set_link_lengths(self, links, lengths):
        """min_length, max_length = lengths[k] of link links[k]; the schedule stays (a rope reeled in)."""
        self._edit("phx_world_set_link_lengths", links, lengths, 2, "set_link_lengths")

    def link_count(self):
        return self._int32("phx_world_link_count")

    def links(self):
        """Every link as a link_dtype array, with the impulses the last step accumulated."""
        return self._get(self.L.phx_world_get_links, link_dtype, self.link_count())

    def add_angles(self, angles):
        """Append angles: an angle_dtype array, or rows (body1, body2, lower, upper[, hertz[, damping_ratio[, motor_speed[, max_torque]]]])
        with both impulses 0.  lower == upper: a lock, with hertz > 0 a torsion spring; lower < upper: limits (wider than a full turn:
        none); max_torque > 0: a motor.  Returns the new angles' indices."""
        return self._add_units("phx_world_add_angles", angles, angle_dtype, ("lower", "upper", "hertz", "damping_ratio", "motor_speed", "max_torque"),
                               required=2, anchors=False)

    def remove_angles(self, angles):
        """Remove the listed angles (each at most once); the others keep their order, so their indices shift."""
        self._remove_units("phx_world_remove_angles", angles, "remove_angles")

    def set_angle_limits(self, angles, limits):
        """lower, upper = limits[k] of angle angles[k]; the schedule stays."""
        self._edit("phx_world_set_angle_limits", angles, limits, 2, "set_angle_limits")

    def set_angle_motors(self, angles, motors):
        """motor_speed, max_torque = motors[k] of angle angles[k]; the schedule stays (a throttle, a brake)."""
        self._edit("phx_world_set_angle_motors", angles, motors, 2, "set_angle_motors")

    def angle_count(self):
        return self._int32("phx_world_angle_count")

    def angles(self):
        """Every angle as an angle_dtype array, with the impulses the last step accumulated."""
        return self._get(self.L.phx_world_get_angles, angle_dtype, self.angle_count())

    def add_sliders(self, sliders):
        """Append sliders: a slider_dtype array, or rows (body1, body2, anchor1, anchor2, axis, lower, upper[, hertz[, damping_ratio[,
        motor_speed[, max_force]]]]) with the three impulses 0.  body1 is the carriage, body2 the rail (-1: the world); lower == upper: a
        lock, with hertz > 0 a spring towards s = lower; lower < upper: limits; max_force > 0: a motor.  Returns the new sliders' indices."""
        return self._add_units("phx_world_add_sliders", sliders, slider_dtype, ("axis", "lower", "upper", "hertz", "damping_ratio", "motor_speed", "max_force"), required=3)

    def remove_sliders(self, sliders):
        """Remove the listed sliders (each at most once); the others keep their order, so their indices shift."""
        self._remove_units("phx_world_remove_sliders", sliders, "remove_sliders")

    def set_slider_anchors(self, sliders, anchors):
        """anchor1, anchor2 = anchors[k] (4 floats) of slider sliders[k]; the schedule stays."""
        self._edit("phx_world_set_slider_anchors", sliders, anchors, 4, "set_slider_anchors")

    def set_slider_limits(self, sliders, limits):
        """lower, upper = limits[k] of slider sliders[k]; the schedule stays."""
        self._edit("phx_world_set_slider_limits", sliders, limits, 2, "set_slider_limits")

    def set_slider_motors(self, sliders, motors):
        """motor_speed, max_force = motors[k] of slider sliders[k]; the schedule stays (an elevator's reversal)."""
        self._edit("phx_world_set_slider_motors", sliders, motors, 2, "set_slider_motors")

    def slider_count(self):
        return self._int32("phx_world_slider_count")

    def sliders(self):
        """Every slider as a slider_dtype array, with the impulses the last step accumulated."""
        return self._get(self.L.phx_world_get_sliders, slider_dtype, self.slider_count())

    # ---- breaks (include/phyx_amd.h BREAKS; the specification: tests/break_spec.py) ----
    @staticmethod
    def _unit_kind(kind, what):
        if isinstance(kind, str):
            if kind not in UNIT_KINDS:
                raise ValueError("%s: kind %r is none of %s" % (what, kind, ", ".join(UNIT_KINDS)))
            return UNIT_KINDS.index(kind)
        return int(kind)

    def set_break_limits(self, kind, units, limits):
        """The break limit limits[k] (> 0; inf: unbreakable, a new unit's) of unit units[k] of `kind` (0..3 or "pin", "link", "angle",
        "slider"): a unit whose reaction impulse exceeds limit * dt after a step's pin pass is removed behind that step and reported by
        break_events().  The schedule stays."""
        idx = self._indices(units, "set_break_limits")
        v = self._values(np.asarray(limits, dtype=np.float32).reshape(-1, 1), len(idx), 1, "set_break_limits")
        check(self.L.phx_world_set_break_limits(self.h, self._unit_kind(kind, "set_break_limits"), _ptr(idx), _ptr(v), len(idx)))

    def break_limits(self, kind):
        """Every unit's break limit of `kind`, in index order: a float32 array (inf where none was set)."""
        k = self._unit_kind(kind, "break_limits")
        n = C.c_int32(0)
        if 0 <= k < 4:
            check(getattr(self.L, "phx_world_%s_count" % UNIT_KINDS[k])(self.h, C.byref(n)))
        out = np.zeros(n.value, dtype=np.float32)
        check(self.L.phx_world_get_break_limits(self.h, k, _ptr(out), len(out)))
        return out

    def break_events(self):
        """The breaks since the last call: a break_event_dtype array in step order, then by (kind, index); index and the bodies in the
        numbering of the step the unit broke in.  Call it once per step (then every `step` is 0)."""
        total = C.c_int64(0)
        cap = 64
        while True:
            out = np.zeros(cap, dtype=break_event_dtype)
            st = self.L.phx_world_break_events(self.h, _ptr(out), cap, C.byref(total))
            if st != _lib.PHX_ERR_CAPACITY or total.value <= cap:
                break
            cap = int(total.value)                                 # (grown to what the call reported; the queue was kept)
        check(st)
        return out[:total.value].copy()

    # ---- sleeping (include/phyx_amd.h SLEEPING; the specification: tests/sleep_spec.py) ----
    def set_sleeping(self, linear_tolerance=None, angular_tolerance=None, time_to_sleep=None):
        """Enable sleeping with the three parameters (all finite and >= 0; no defaults: the scene's units are the caller's), or, with
        no argument, wake everything and turn it off.  A component whose bodies all stayed below both tolerances for time_to_sleep
        rests as static bodies until something awake touches it or a call names one of its bodies."""
        given = [v is not None for v in (linear_tolerance, angular_tolerance, time_to_sleep)]
        if not any(given):
            check(self.L.phx_world_set_sleeping(self.h, None))
            return
        if not all(given):
            raise ValueError("set_sleeping: linear_tolerance, angular_tolerance and time_to_sleep go together (none of them: sleeping off)")
        p = np.array([linear_tolerance, angular_tolerance, time_to_sleep], dtype=np.float32)
        check(self.L.phx_world_set_sleeping(self.h, _ptr(p)))

    def sleeping(self):
        """(linear_tolerance, angular_tolerance, time_to_sleep) while sleeping is enabled, else None."""
        p = np.zeros(3, dtype=np.float32)
        on = C.c_int32(0)
        check(self.L.phx_world_get_sleeping(self.h, _ptr(p), C.byref(on)))
        return tuple(float(x) for x in p) if on.value else None

    def sleep_states(self):
        """Every body's sleep_state_dtype record: asleep, timer, and its own inverse masses whether it sleeps or not (bodies shows a
        sleeper as the step sees it: inverse masses and velocities 0)."""
        return self._get(self.L.phx_world_get_sleep_states, sleep_state_dtype, self.counts()[0])

    def wake_bodies(self, bodies):
        """Wake the sleeping component of each listed body (a body that is awake is left alone)."""
        idx = self._indices(bodies, "wake_bodies")
        check(self.L.phx_world_wake_bodies(self.h, _ptr(idx), len(idx)))

    def sleep_counts(self):
        """(asleep now, bodies put to sleep in total, bodies woken in total)."""
        asleep, slept, woken = C.c_int32(0), C.c_int64(0), C.c_int64(0)
        check(self.L.phx_world_sleep_counts(self.h, C.byref(asleep), C.byref(slept), C.byref(woken)))
        return asleep.value, slept.value, woken.value

    # ---- force fields (include/phyx_amd.h FORCE FIELDS; the specification: tests/field_spec.py) ----
    def set_fields(self, fields):
        """Replace the world's field list (rows of uniform_field / radial_field / drag_field, at most MAX_FIELDS; []: none).  From the
        next Update on, every step first adds the fields' accelerations, in list order, to what IntegrateVelocity consumes."""
        f = _fields(fields, "set_fields")
        check(self.L.phx_world_set_fields(self.h, _ptr(f), len(f)))

    def fields(self):
        """The field list as a field_dtype array."""
        n = C.c_int32(0)
        out = np.zeros(MAX_FIELDS, dtype=field_dtype)
        check(self.L.phx_world_get_fields(self.h, _ptr(out), len(out), C.byref(n)))
        return out[:n.value].copy()

    def pulse_fields(self, fields):
        """One shot, between steps: velocity += what the listed fields would add in a step of dt = 1 (a blast: a radial_field with a
        falloff radius).  Sleepers are not affected; wake_bodies(query_aabb(...)) first for a blast that wakes a pile."""
        f = _fields(fields, "pulse_fields")
        check(self.L.phx_world_pulse_fields(self.h, _ptr(f), len(f)))

    def apply_impulses(self, bodies, impulses):
        """The impulse (J.x, J.y) at the world point (point.x, point.y) on body bodies[k]: impulses is (K, 4) {J.x, J.y, point.x, point.y};
        v += inv_mass J, w -= inv_inertia (r x J) with r = point - pos (the engine's angular velocity is clockwise-positive)."""
        self._edit("phx_world_apply_impulses", bodies, impulses, 4, "apply_impulses")

    def field_passes(self):
        """How many field passes the steps have launched so far: one per step while the list is not empty, none otherwise."""
        n = C.c_int64(0)
        check(self.L.phx_world_field_passes(self.h, C.byref(n)))
        return n.value

    # ---- the per-body columns: collision filters, materials, body flags ----
    @staticmethod
    def _per_body(what, name, v, count, kinds, lo=None, hi=None, range_text=None):
        """A setter's value `name`: a scalar for all `count` bodies or one value per body, of the dtype kinds `kinds` ("iu": integers,
        "fiu": numbers) and within [lo, hi] where given."""
        a = np.asarray(v)
        if a.dtype.kind not in kinds:
            raise TypeError("%s: %s must be %s, got %s" % (what, name, "integers" if kinds == "iu" else "numbers", a.dtype))
        if a.ndim > 1 or (a.ndim == 1 and a.shape != (count,)):
            raise ValueError("%s: %s must be a scalar or have shape (%d,), got %s" % (what, name, count, a.shape))
        if lo is not None and a.size and (int(a.min()) < lo or int(a.max()) > hi):
            raise ValueError("%s: %s out of the range %s" % (what, name, range_text or "[%d, %d]" % (lo, hi)))
        return a

    # ---- collision filters (include/phyx_amd.h COLLISION FILTERS; the specification: tests/filter_spec.py) ----
    def set_collision_filters(self, bodies, category=1, mask=0xFFFFFFFF, group=0):
        """Give the listed bodies (each at most once) the filter {category, mask, group}: each a scalar for all of them or one value per
        body.  A pair (a, b) collides iff a shared non-zero group is positive, or else each mask meets the other's category.  Manifolds
        whose pair now fails are dropped as set_state of filter_spec.drop(state()) would; returns how many were."""
        idx = self._indices(bodies, "set_collision_filters")
        f = np.zeros(len(idx), dtype=collision_filter_dtype)
        for name, v, lo, hi in (("category", category, 0, 2 ** 32 - 1), ("mask", mask, 0, 2 ** 32 - 1),
                                ("group", group, -2 ** 31, 2 ** 31 - 1)):
            f[name] = self._per_body("set_collision_filters", name, v, len(idx), "iu", lo, hi)
        dropped = C.c_int32(0)
        check(self.L.phx_world_set_collision_filters(self.h, _ptr(idx), _ptr(f), len(idx), C.byref(dropped)))
        return dropped.value

    def collision_filters(self):
        """Every body's filter, in index order: an array of collision_filter_dtype."""
        return self._get(self.L.phx_world_get_collision_filters, collision_filter_dtype, self.counts()[0])

    # ---- collision exclusions (include/phyx_amd.h COLLISION EXCLUSIONS; the specification: tests/exclusion_spec.py) ----
    @staticmethod
    def _pairs(pairs, what):
        p = np.asarray(pairs)
        if p.size == 0:
            return np.zeros((0, 2), dtype=np.int32)
        if p.dtype.kind not in "iu":
            raise TypeError("%s: the pairs must be integers, got %s" % (what, p.dtype))
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError("%s: the pairs must have shape (n, 2), got %s" % (what, p.shape))
        if int(p.min()) < -2 ** 31 or int(p.max()) > 2 ** 31 - 1:
            raise ValueError("%s: a body index is outside the int32 range" % what)
        return np.ascontiguousarray(p, dtype=np.int32)

    def add_collision_exclusions(self, pairs):
        """The body pairs (a, b) of `pairs`, shape (n, 2), never collide from now on: set union with the world's exclusion set (a != b;
        (a, b) and (b, a) are one pair, at most once per call).  Manifolds of pairs that are now excluded are dropped as set_state of
        exclusion_spec.drop(state(), pairs) would; returns how many were."""
        p = self._pairs(pairs, "add_collision_exclusions")
        dropped = C.c_int32(0)
        check(self.L.phx_world_add_collision_exclusions(self.h, _ptr(p), len(p), C.byref(dropped)))
        return dropped.value

    def remove_collision_exclusions(self, pairs):
        """Set difference: the listed pairs may collide again (absent ones are ignored).  No manifold changes; a pair that overlaps is
        new to the next step."""
        p = self._pairs(pairs, "remove_collision_exclusions")
        check(self.L.phx_world_remove_collision_exclusions(self.h, _ptr(p), len(p)))

    def clear_collision_exclusions(self):
        """Empty the exclusion set."""
        check(self.L.phx_world_clear_collision_exclusions(self.h))

    def collision_exclusions(self):
        """The exclusion set: an (n, 2) int32 array of {lo, hi} pairs, ascending by (lo, hi)."""
        n = C.c_int32(0)
        st = self.L.phx_world_get_collision_exclusions(self.h, None, 0, C.byref(n))
        if st != _lib.PHX_ERR_CAPACITY:
            check(st)
        out = np.zeros((n.value, 2), dtype=np.int32)
        check(self.L.phx_world_get_collision_exclusions(self.h, _ptr(out), n.value, C.byref(n)))
        return out

    def exclude_joined(self, kinds=None):
        """collideConnected = false: exclude the body pair of every current unit of `kinds` (any of "pin", "link", "angle", "slider" or
        0..3; None: all four) that joins two bodies (body2 >= 0).  Units added later are not covered.  Returns what
        add_collision_exclusions returns."""
        chosen = range(len(UNIT_KINDS)) if kinds is None else [self._unit_kind(k, "exclude_joined") for k in kinds]
        pairs = set()
        for k in chosen:
            if not 0 <= k < len(UNIT_KINDS):
                raise ValueError("exclude_joined: kind %r is none of %s" % (k, ", ".join(UNIT_KINDS)))
            units = getattr(self, UNIT_KINDS[k] + "s")()
            for a, b in zip(units["body1"].tolist(), units["body2"].tolist()):
                if b >= 0 and a != b:
                    pairs.add((min(a, b), max(a, b)))
        return self.add_collision_exclusions(np.array(sorted(pairs), dtype=np.int32).reshape(-1, 2))

    # ---- materials (include/phyx_amd.h MATERIALS; the specification: tests/material_spec.py) ----
    def set_materials(self, bodies, friction=0.3, restitution=0.0):
        """Give the listed bodies (each at most once) the material {friction, restitution}: each a scalar for all of them or one value per
        body.  A contact uses mu = (fa + fb) * 0.5 and e = max(ea, eb) from the next step on; the library rejects friction outside
        [0, 1e6], restitution outside [0, 1] and non-finite values (PhxError), the world unchanged."""
        idx = self._indices(bodies, "set_materials")
        m = np.zeros(len(idx), dtype=material_dtype)
        for name, v in (("friction", friction), ("restitution", restitution)):
            m[name] = self._per_body("set_materials", name, v, len(idx), "fiu")
        check(self.L.phx_world_set_materials(self.h, _ptr(idx), _ptr(m), len(idx)))

    def materials(self):
        """Every body's material, in index order: an array of material_dtype."""
        return self._get(self.L.phx_world_get_materials, material_dtype, self.counts()[0])

    # ---- body flags / sensors (include/phyx_amd.h BODY FLAGS / SENSORS; the specification: tests/sensor_spec.py) ----
    def set_body_flags(self, bodies, flags):
        """Give the listed bodies (each at most once) the flag word `flags`: a scalar for all of them or one value per body.  BODY_SENSOR
        makes a body a trigger volume: its pairs keep their manifolds and contact points (touch events, contact reports with
        CONTACT_NO_JOINT) and get no joints, from the next step on.  The library rejects any other bit (PhxError), the world unchanged."""
        idx = self._indices(bodies, "set_body_flags")
        f = np.zeros(len(idx), dtype=np.uint32)
        f[:] = self._per_body("set_body_flags", "flags", flags, len(idx), "iu", 0, 2 ** 32 - 1, "[0, 2^32)")
        check(self.L.phx_world_set_body_flags(self.h, _ptr(idx), _ptr(f), len(idx)))

    def body_flags(self):
        """Every body's flag word, in index order: a uint32 array."""
        return self._get(self.L.phx_world_get_body_flags, np.uint32, self.counts()[0])

    # ---- shapes (include/phyx_amd.h SHAPES; the specification: tests/circle_spec.py) ----
    def set_shapes(self, bodies, kind=SHAPE_BOX, hx=None, hy=None):
        """Give the listed bodies (each at most once) the shape {kind, hx, hy}: each a scalar for all of them or one value per body.
        kind is SHAPE_BOX (hx, hy: half extents), SHAPE_CIRCLE (hx: the radius; hy may be left out and must equal hx otherwise) or
        SHAPE_CAPSULE (hx > hy: the half extents of its frame box; the radius is hy, the core segment runs hx - hy either way along x).
        The body's geom_size becomes (hx, hy) and its AABB is recomputed as set_poses recomputes it; the inverse masses stay
        (set_inverse_masses; circle_inverse_masses has the circle formula).  The library rejects any other kind, sizes that are not
        finite and positive, a circle whose hy differs from hx and a capsule whose hx is not above hy (PhxError), the world unchanged."""
        idx = self._indices(bodies, "set_shapes")
        if hx is None:
            raise ValueError("set_shapes: hx (the half extent on x, or the radius) is required")
        s = np.zeros(len(idx), dtype=shape_dtype)
        s["kind"] = self._per_body("set_shapes", "kind", kind, len(idx), "iu", -2 ** 31, 2 ** 31 - 1)
        s["hx"] = self._per_body("set_shapes", "hx", hx, len(idx), "fiu")
        s["hy"] = s["hx"] if hy is None else self._per_body("set_shapes", "hy", hy, len(idx), "fiu")
        check(self.L.phx_world_set_shapes(self.h, _ptr(idx), _ptr(s), len(idx)))

    def shapes(self):
        """Every body's shape {kind, hx, hy}, in index order: an array of shape_dtype (boxes in a world that never set a shape)."""
        return self._get(self.L.phx_world_get_shapes, shape_dtype, self.counts()[0])

    def add_circles(self, spawn):
        """Append circles: spawn is a (K, 4) float array {px, py, angle, r}.  add_bodies with half extents (r, r), then set_shapes of
        the new bodies to SHAPE_CIRCLE, then set_inverse_masses with circle_inverse_masses(r).  Returns the first new index."""
        a = np.asarray(spawn)
        if a.dtype.kind != "f":
            raise TypeError("add_circles: spawn must be a float array, got %s" % (a.dtype,))
        if a.ndim != 2 or a.shape[1] != 4:
            raise ValueError("add_circles: spawn must have shape (K, 4) {px, py, angle, r}, got %s" % (a.shape,))
        s = np.ascontiguousarray(a, dtype=np.float32)
        idx = self.add_bodies(np.ascontiguousarray(s[:, [0, 1, 2, 3, 3]]))
        first = int(idx[0]) if len(idx) else self.counts()[0]
        if len(idx):
            self.set_shapes(idx, SHAPE_CIRCLE, s[:, 3])
            self.set_inverse_masses(idx, circle_inverse_masses(s[:, 3]))
        return first

    def add_capsules(self, spawn):
        """Append capsules: spawn is a (K, 5) float array {px, py, angle, hx, hy}, hx > hy (the frame box's half extents; the radius is
        hy).  add_bodies with those half extents, then set_shapes of the new bodies to SHAPE_CAPSULE, then set_inverse_masses with
        capsule_inverse_masses(hx, hy).  Returns the first new index."""
        a = np.asarray(spawn)
        if a.dtype.kind != "f":
            raise TypeError("add_capsules: spawn must be a float array, got %s" % (a.dtype,))
        if a.ndim != 2 or a.shape[1] != 5:
            raise ValueError("add_capsules: spawn must have shape (K, 5) {px, py, angle, hx, hy}, got %s" % (a.shape,))
        s = np.ascontiguousarray(a, dtype=np.float32)
        if not (s[:, 3] > s[:, 4]).all():
            raise ValueError("add_capsules: hx must be above hy (a capsule with hx == hy is a circle: add_circles)")
        idx = self.add_bodies(s)
        first = int(idx[0]) if len(idx) else self.counts()[0]
        if len(idx):
            self.set_shapes(idx, SHAPE_CAPSULE, s[:, 3], s[:, 4])
            self.set_inverse_masses(idx, capsule_inverse_masses(s[:, 3], s[:, 4]))
        return first

    # ---- polygons (include/phyx_amd.h POLYGONS; the specification: tests/polygon_spec.py) ----
    def set_polygons(self, bodies, polygons):
        """Make the listed bodies (each at most once) convex polygons: `polygons` is one (N, 2) list of body-local vertices for all of
        them, one such list per body, or an array of polygon_dtype.  The vertices are counter-clockwise, 3 to 8 of them, strictly convex,
        with the body's origin strictly inside.  The body's kind becomes SHAPE_POLYGON, its geom_size the frame box
        (max |x|, max |y|) and its AABB is recomputed; the inverse masses stay (set_inverse_masses; polygon_inverse_masses has the
        formula).  The library rejects anything else (PhxError), the world unchanged.  set_shapes turns a polygon back into a box, a
        circle or a capsule."""
        idx = self._indices(bodies, "set_polygons")
        p = _polygons(polygons, len(idx), "set_polygons")
        check(self.L.phx_world_set_polygons(self.h, _ptr(idx), _ptr(p), len(idx)))

    def polygons(self, bodies=None):
        """The polygons of the listed bodies (all of them if None), in that order: an array of polygon_dtype; count 0 and zeros for a
        body that is not a polygon."""
        idx = np.arange(self.counts()[0], dtype=np.int32) if bodies is None else np.ascontiguousarray(np.asarray(bodies).reshape(-1), dtype=np.int32)
        out = np.zeros(len(idx), dtype=polygon_dtype)
        check(self.L.phx_world_get_polygons(self.h, _ptr(idx), _ptr(out), len(idx)))
        return out

    def add_polygons(self, spawn, polygons):
        """Append polygons: spawn is a (K, 3) float array {px, py, angle}, `polygons` as in set_polygons.  add_bodies with each polygon's
        frame box as half extents, then set_polygons of the new bodies, then set_inverse_masses with polygon_inverse_masses.  Returns
        the first new index."""
        a = np.asarray(spawn)
        if a.dtype.kind != "f":
            raise TypeError("add_polygons: spawn must be a float array, got %s" % (a.dtype,))
        if a.ndim != 2 or a.shape[1] != 3:
            raise ValueError("add_polygons: spawn must have shape (K, 3) {px, py, angle}, got %s" % (a.shape,))
        s = np.ascontiguousarray(a, dtype=np.float32)
        p = _polygons(polygons, len(s), "add_polygons")
        if ((p["count"] < 3) | (p["count"] > POLYGON_MAX_VERTICES)).any():
            raise ValueError("add_polygons: a polygon has 3 to %d vertices" % POLYGON_MAX_VERTICES)
        half = np.array([np.abs(q["v"][:q["count"]]).max(axis=0) for q in p], dtype=np.float32).reshape(-1, 2)
        idx = self.add_bodies(np.ascontiguousarray(np.column_stack([s, half])))
        first = int(idx[0]) if len(idx) else self.counts()[0]
        if len(idx):
            self.set_polygons(idx, p)
            self.set_inverse_masses(idx, np.array([polygon_inverse_masses(q["v"][:q["count"]]) for q in p], dtype=np.float32))
        return first

    # ---- continuous bodies (include/phyx_amd.h CONTINUOUS BODIES; the specification: tests/sweep_spec.py) ----
    def inradii(self, bodies=None):
        """The inradius about its origin of the listed bodies (all of them if None), computed on the host from shapes() and polygons():
        min(hx, hy) of a box, r of a circle, hy of a capsule, min_k dot(n_k, v_k) of a polygon (float32)."""
        idx = np.arange(self.counts()[0], dtype=np.int32) if bodies is None else self._indices(bodies, "inradii")
        s = self.shapes()[idx]
        out = np.minimum(s["hx"], s["hy"]).astype(np.float32)
        out = np.where(s["kind"] == SHAPE_CIRCLE, s["hx"], out).astype(np.float32)
        which = np.flatnonzero(s["kind"] == SHAPE_POLYGON)
        if len(which):
            f = np.float32
            for k, p in zip(which, self.polygons(idx[which])):
                v = p["v"][:p["count"]].astype(f)
                e = (np.roll(v, -1, axis=0) - v).astype(f)
                l = np.sqrt((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]).astype(f)).astype(f)
                nx, ny = (e[:, 1] / l).astype(f), (-e[:, 0] / l).astype(f)
                out[k] = ((nx * v[:, 0]).astype(f) + (ny * v[:, 1]).astype(f)).astype(f).min()
        return out

    def set_continuous(self, bodies, radii=None, factor=0.8):
        """Make the listed bodies (each at most once) continuous: after every step's IntegratePosition the core disc of radius radii[k]
        about the body's origin is cast along the translation the step gave the body, against every static body it collides with, and
        the body is put back to the point of first touch.  radii: a scalar for all of them or one value per body, each below the body's
        inradius; 0 makes a body discrete again; None takes factor x inradii(bodies).  The library rejects anything else (PhxError),
        the world unchanged."""
        idx = self._indices(bodies, "set_continuous")
        r = np.zeros(len(idx), dtype=np.float32)
        if radii is None:
            if len(idx):
                r[:] = (np.float32(factor) * self.inradii(idx)).astype(np.float32)
        else:
            r[:] = self._per_body("set_continuous", "radii", radii, len(idx), "fiu")
        check(self.L.phx_world_set_continuous(self.h, _ptr(idx), _ptr(r), len(idx)))

    def continuous(self):
        """Every body's core radius, in index order: a float32 array, 0 for a discrete body."""
        return self._get(self.L.phx_world_get_continuous, np.float32, self.counts()[0])

    def sweep_hits(self):
        """The clamps of the last step's pass, ascending by body: an array of sweep_hit_dtype {body, target, t, normal}."""
        total = C.c_int64(0)
        st = self.L.phx_world_sweep_hits(self.h, None, 0, C.byref(total))
        if st == 0 and total.value == 0:
            return np.zeros(0, dtype=sweep_hit_dtype)
        out = np.zeros(max(int(total.value), 1), dtype=sweep_hit_dtype)
        check(self.L.phx_world_sweep_hits(self.h, _ptr(out), len(out), C.byref(total)))
        return out[:total.value]

    def sweep_counts(self):
        """(passes launched, clamps made) since the world was created; passes stays 0 in a world without a continuous body."""
        passes, clamps = C.c_int64(0), C.c_int64(0)
        check(self.L.phx_world_sweep_counts(self.h, C.byref(passes), C.byref(clamps)))
        return passes.value, clamps.value

    def sweep_timing(self, enable=True):
        """The device time in ms of the last pass's kernel that was timed (0.0 if none was); then every later pass is timed by two HIP
        events while `enable` holds (tools/sweep_cost.py)."""
        ms = C.c_double(0.0)
        check(self.L.phx_world_sweep_timing(self.h, 1 if enable else 0, C.byref(ms)))
        return ms.value

    # ---- queries (include/phyx_amd.h: phx_world_query_aabb / _points / raycast; the specification: tests/query_spec.py) ----
    @staticmethod
    def _queries(q, width, what, names):
        a = np.asarray(_or_empty(q, (0, width), np.float32))
        if a.dtype.kind not in "iuf":
            raise TypeError("%s: queries must be a numeric array, got %s" % (what, a.dtype))
        if a.ndim != 2 or a.shape[1] != width:
            raise ValueError("%s: queries must have shape (K, %d) %s, got %s" % (what, width, names, a.shape))
        if len(a) > np.iinfo(np.int32).max:
            raise ValueError("%s: more than 2^31 - 1 queries" % what)
        with np.errstate(over="ignore"):
            a = np.ascontiguousarray(a, dtype=np.float32)          # (a value beyond the float range becomes infinite: refused below)
        if not np.isfinite(a).all():
            raise ValueError("%s: every value must be finite" % what)
        return a

    def query_aabb(self, boxes, skip_static=False):
        """Bodies whose AABB overlaps each closed box; boxes (K, 4) {min.x, min.y, max.x, max.y}.  Returns (offsets, hits): int32 arrays,
        the hits of box q are hits[offsets[q]:offsets[q + 1]], ascending."""
        b = self._queries(boxes, 4, "query_aabb", "{min.x, min.y, max.x, max.y}")
        if ((b[:, 0] > b[:, 2]) | (b[:, 1] > b[:, 3])).any():
            raise ValueError("query_aabb: every box must have min <= max")
        return self._overlaps(self.L.phx_world_query_aabb, b, skip_static)

    def _listing(self, fn, rows, skip_static, dtype, cap):
        """The lists of phx_world_query_aabb / _boxes / _contacts: a call with room for `cap` records and, if it reports
        PHX_ERR_CAPACITY with a total that fits int32, one more with room for exactly that total.  Returns (offsets, records)."""
        flags = 1 if skip_static else 0
        offsets = np.zeros(len(rows) + 1, dtype=np.int32)
        total = C.c_int64(0)
        for _ in range(2):
            out = np.zeros(cap, dtype=dtype)
            st = fn(self.h, _ptr(rows), len(rows), flags, _ptr(offsets), _ptr(out), cap, C.byref(total))
            if st != _lib.PHX_ERR_CAPACITY or total.value > np.iinfo(np.int32).max:
                break
            cap = int(total.value)
        check(st)
        return offsets, out[:total.value].copy() if total.value < cap else out

    def _overlaps(self, fn, b, skip_static):
        return self._listing(fn, b, skip_static, np.int32, max(1024, 4 * len(b)))

    def query_points(self, points, skip_static=False):
        """For each point (K, 2), the lowest index of a body whose box contains it, -1 if none (int32)."""
        p = self._queries(points, 2, "query_points", "{x, y}")
        out = np.zeros(len(p), dtype=np.int32)
        check(self.L.phx_world_query_points(self.h, _ptr(p), len(p), 1 if skip_static else 0, _ptr(out)))
        return out

    def raycast(self, rays, skip_static=False):
        """The closest hit of each ray (K, 5) {ox, oy, dx, dy, max_t}: a ray_hit_dtype array (body -1 and zeros: no hit)."""
        r = self._queries(rays, 5, "raycast", "{ox, oy, dx, dy, max_t}")
        if (r[:, 4] < 0).any():
            raise ValueError("raycast: max_t must be >= 0")
        if ((r[:, 2] == 0) & (r[:, 3] == 0)).any():
            raise ValueError("raycast: a ray's direction must not be zero")
        out = np.zeros(len(r), dtype=ray_hit_dtype)
        check(self.L.phx_world_raycast(self.h, _ptr(r), len(r), 1 if skip_static else 0, _ptr(out)))
        return out

    def query_points_device(self, points_ptr, count, body_ptr, skip_static=False):
        """query_points on device memory (2 floats per point in, int32 per point out), queued on the world's stream (stream_ptr())."""
        check(self.L.phx_world_query_points_device(self.h, _dev_ptr(points_ptr), int(count), 1 if skip_static else 0, _dev_ptr(body_ptr)))

    def raycast_device(self, rays_ptr, count, out_ptr, skip_static=False):
        """raycast on device memory (5 floats per ray in, a 24-byte ray_hit_dtype record per ray out), queued on the world's stream."""
        check(self.L.phx_world_raycast_device(self.h, _dev_ptr(rays_ptr), int(count), 1 if skip_static else 0, _dev_ptr(out_ptr)))

    def query_boxes(self, boxes, skip_static=False):
        """Bodies whose box overlaps each oriented query box (closed); boxes (K, 8) {pos.x, pos.y, xv.x, xv.y, yv.x, yv.y, h.x, h.y}
        (box_from_angle builds one).  Returns (offsets, hits) as query_aabb."""
        b = self._queries(boxes, 8, "query_boxes", "{pos.x, pos.y, xv.x, xv.y, yv.x, yv.y, h.x, h.y}")
        if (b[:, 6:8] <= 0).any():
            raise ValueError("query_boxes: half extents must be positive")
        return self._overlaps(self.L.phx_world_query_boxes, b, skip_static)

    @staticmethod
    def _casts(casts, what):
        c = World._queries(casts, 11, what, "{box[8], dx, dy, max_t}")
        if (c[:, 6:8] <= 0).any():
            raise ValueError("%s: half extents must be positive" % what)
        if (c[:, 10] < 0).any():
            raise ValueError("%s: max_t must be >= 0" % what)
        if ((c[:, 8] == 0) & (c[:, 9] == 0)).any():
            raise ValueError("%s: a cast's direction must not be zero" % what)
        return c

    def cast_boxes(self, casts, skip_static=False):
        """The first body each box touches moving pos + t * d, t in [0, max_t]; casts (K, 11) {box[8], dx, dy, max_t}: a shape_hit_dtype
        array (body -1 and zeros: no hit)."""
        c = self._casts(casts, "cast_boxes")
        out = np.zeros(len(c), dtype=shape_hit_dtype)
        check(self.L.phx_world_cast_boxes(self.h, _ptr(c), len(c), 1 if skip_static else 0, _ptr(out)))
        return out

    def cast_boxes_device(self, casts_ptr, count, out_ptr, skip_static=False):
        """cast_boxes on device memory (11 floats per cast in, a 16-byte shape_hit_dtype record per cast out), queued on the world's stream."""
        check(self.L.phx_world_cast_boxes_device(self.h, _dev_ptr(casts_ptr), int(count), 1 if skip_static else 0, _dev_ptr(out_ptr)))

    def query_circles(self, circles, skip_static=False):
        """Bodies whose box or disc overlaps each query circle (closed); circles (K, 3) {c.x, c.y, r}.  Returns (offsets, hits) as
        query_aabb."""
        c = self._queries(circles, 3, "query_circles", "{c.x, c.y, r}")
        if (c[:, 2] <= 0).any():
            raise ValueError("query_circles: the radius must be positive")
        return self._overlaps(self.L.phx_world_query_circles, c, skip_static)

    def cast_circles(self, casts, skip_static=False):
        """The first body each circle touches moving c + t * d, t in [0, max_t]; casts (K, 6) {c.x, c.y, r, dx, dy, max_t}: a
        shape_hit_dtype array (body -1 and zeros: no hit)."""
        c = self._queries(casts, 6, "cast_circles", "{c.x, c.y, r, dx, dy, max_t}")
        if (c[:, 2] <= 0).any():
            raise ValueError("cast_circles: the radius must be positive")
        if (c[:, 5] < 0).any():
            raise ValueError("cast_circles: max_t must be >= 0")
        if ((c[:, 3] == 0) & (c[:, 4] == 0)).any():
            raise ValueError("cast_circles: a cast's direction must not be zero")
        out = np.zeros(len(c), dtype=shape_hit_dtype)
        check(self.L.phx_world_cast_circles(self.h, _ptr(c), len(c), 1 if skip_static else 0, _ptr(out)))
        return out

    def cast_circles_device(self, casts_ptr, count, out_ptr, skip_static=False):
        """cast_circles on device memory (6 floats per cast in, a 16-byte shape_hit_dtype record per cast out), queued on the world's stream."""
        check(self.L.phx_world_cast_circles_device(self.h, _dev_ptr(casts_ptr), int(count), 1 if skip_static else 0, _dev_ptr(out_ptr)))

    def query_nearest(self, queries, skip_static=False):
        """The body nearest to each point within max_dist; queries (K, 3) {p.x, p.y, max_dist} (np.finfo(np.float32).max: anywhere): a
        near_hit_dtype array of the signed distance (negative inside), the outward normal and the surface point (body -1 and zeros: none)."""
        q = self._queries(queries, 3, "query_nearest", "{p.x, p.y, max_dist}")
        if (q[:, 2] < 0).any():
            raise ValueError("query_nearest: max_dist must be >= 0")
        out = np.zeros(len(q), dtype=near_hit_dtype)
        check(self.L.phx_world_query_nearest(self.h, _ptr(q), len(q), 1 if skip_static else 0, _ptr(out)))
        return out

    def query_nearest_device(self, queries_ptr, count, out_ptr, skip_static=False):
        """query_nearest on device memory (3 floats per query in, a 24-byte near_hit_dtype record per query out), queued on the world's stream."""
        check(self.L.phx_world_query_nearest_device(self.h, _dev_ptr(queries_ptr), int(count), 1 if skip_static else 0, _dev_ptr(out_ptr)))

    def query_index(self):
        """Queue the build of the query index unless it is current; returns how many times this world has built it."""
        n = C.c_int64(0)
        check(self.L.phx_world_query_index(self.h, C.byref(n)))
        return n.value

    # ---- contact reports (include/phyx_amd.h: CONTACTS; the specification: tests/contact_spec.py) ----
    def contacts(self, bodies, skip_static=False):
        """The contacts of each listed body (repeats allowed): one contact_dtype record per live contact-point slot of every manifold the
        body is in, ordered by (other, manifold, slot).  Returns (offsets, records): body q's records are records[offsets[q]:offsets[q + 1]]."""
        idx = self._indices(bodies, "contacts")
        if idx.size and idx.min() < 0:
            raise ValueError("contacts: negative body index")
        return self._listing(self.L.phx_world_query_contacts, idx, skip_static, contact_dtype, max(256, 8 * len(idx)))

    def contact_events(self):
        """Touch events since the last call: (begin, end), (K, 2) int32 arrays of {body1, body2} pairs sorted ascending; the pairs that
        started / stopped touching (a manifold with point_count > 0).  The baseline advances only when the call succeeds."""
        caps = [max(64, self.counts()[1]), 64]
        bt, et = C.c_int64(0), C.c_int64(0)
        for _ in range(2):
            begin = np.zeros((caps[0], 2), dtype=np.int32)
            end = np.zeros((caps[1], 2), dtype=np.int32)
            st = self.L.phx_world_contact_events(self.h, _ptr(begin), caps[0], C.byref(bt), _ptr(end), caps[1], C.byref(et))
            if st != _lib.PHX_ERR_CAPACITY:
                break
            caps = [max(caps[0], int(bt.value)), max(caps[1], int(et.value))]
        check(st)
        return begin[:bt.value].copy(), end[:et.value].copy()

    def contact_markers_device(self, out, cap=None):
        """The demo's contact markers (contact_marker_dtype, 24 B each, 2 per manifold) into device memory, queued on the world's stream:
        `out` is a torch tensor (its data_ptr()) or a device address (int or ctypes pointer, 8-byte aligned); cap in markers (default:
        2 * the manifold count)."""
        if hasattr(out, "data_ptr"):
            if cap is None:
                cap = out.numel() * out.element_size() // contact_marker_dtype.itemsize
            out = out.data_ptr()
        if isinstance(out, bool) or not isinstance(out, (int, np.integer, C.c_void_p)):
            raise TypeError("contact_markers_device: expected a tensor or a device address, got %s" % type(out).__name__)
        if cap is None:
            cap = 2 * self.counts()[1]
        if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or cap < 0 or cap > np.iinfo(np.int32).max:
            raise ValueError("contact_markers_device: cap must be an int32 >= 0")
        check(self.L.phx_world_get_contact_markers_device(self.h, _dev_ptr(out), int(cap)))

    def contact_index(self):
        """Queue the build of the contact index unless it is current; returns how many times this world has built it."""
        n = C.c_int64(0)
        check(self.L.phx_world_contact_index(self.h, C.byref(n)))
        return n.value

    def sync(self):
        """Wait for the queued step (Update returns once the step is queued; getters synchronise on their own)."""
        check(self.L.phx_world_synchronize(self.h))

    def x_extent(self):
        """(min x, max x) over the dynamic bodies' AABBs, reduced on the device (phx_world_x_extent)."""
        out = np.zeros(2, dtype=np.float32)
        check(self.L.phx_world_x_extent(self.h, _ptr(out)))
        return float(out[0]), float(out[1])

    def reslab(self, global_index, scene_size, bounds, margin=1.0, rank=0, size=1, comm=None, all_gather=None, all_reduce_max=None):
        """phx_world_reslab: the collective hand-over of an ownership-sharded world's bodies (every rank calls it at the same step).
        global_index: scene index of every body of this world.  comm: a phyx_amd.Comm (collectives on device buffers through RCCL), or
        the two host callables all_gather(send: uint8 array) -> uint8 array of size * len(send) and all_reduce_max(int) -> int.
        Returns (moved, global_index, (lo, hi)): moved = somebody changed owner and this world was rebuilt for its new slab."""
        from ._lib import SlabTransport, SLAB_ALL_GATHER, SLAB_ALL_REDUCE_MAX
        gi = np.zeros(int(scene_size), dtype=np.int64)
        gi[:len(global_index)] = np.asarray(global_index, dtype=np.int64)
        count = C.c_int32(len(global_index))
        b = np.asarray([bounds[0], bounds[1]], dtype=np.float64)
        moved = C.c_int32(0)
        errors = []

        def gather_cb(user, send, recv, nbytes):
            try:
                mine = np.ctypeslib.as_array(C.cast(send, C.POINTER(C.c_uint8)), shape=(nbytes,)).copy()
                out = np.ascontiguousarray(all_gather(mine), dtype=np.uint8).reshape(-1)
                if out.size != nbytes * size:
                    raise RuntimeError("all_gather returned %d bytes, expected %d" % (out.size, nbytes * size))
                C.memmove(recv, out.ctypes.data, out.size)
                return 0
            except Exception as e:          # (an exception must not unwind through the C frames)
                errors.append(e)
                return 1

        def max_cb(user, value):
            try:
                value[0] = int(all_reduce_max(int(value[0])))
                return 0
            except Exception as e:
                errors.append(e)
                return 1
        tp = SlabTransport()
        tp.rank, tp.size = int(rank), int(size)
        tp.comm = comm.h if comm is not None else None
        g_cb = SLAB_ALL_GATHER(gather_cb) if all_gather is not None else SLAB_ALL_GATHER()
        m_cb = SLAB_ALL_REDUCE_MAX(max_cb) if all_reduce_max is not None else SLAB_ALL_REDUCE_MAX()
        tp.all_gather, tp.all_reduce_max, tp.user = g_cb, m_cb, None
        st = self.L.phx_world_reslab(self.h, C.byref(tp), _ptr(gi), len(gi), C.byref(count), int(scene_size), float(margin), _ptr(b), C.byref(moved))
        if errors:
            raise errors[0]
        check(st)
        return bool(moved.value), gi[:count.value].copy(), (float(b[0]), float(b[1]))

    def build_counts(self):
        """(rebuilds whose components and bins came from the manifolds, rebuilds from the joints) so far (phx_world_build_counts)."""
        out = np.zeros(2, dtype=np.int64)
        check(self.L.phx_world_build_counts(self.h, _ptr(out)))
        return int(out[0]), int(out[1])

    def debug_counters(self):
        """{deferred_packs, deferred_pack_retries, solve_replays, dropped_points} (phx_world_debug_counters)."""
        out = np.zeros(4, dtype=np.int64)
        check(self.L.phx_world_debug_counters(self.h, _ptr(out)))
        return dict(zip(("deferred_packs", "deferred_pack_retries", "solve_replays", "dropped_points"), (int(x) for x in out)))

    def set_phase_timing(self, on=True):
        """Per-phase host timers (phase_ms) cost one stream synchronisation per phase; off by default."""
        check(self.L.phx_world_set_phase_timing(self.h, 1 if on else 0))

    def phase_ms(self):
        out = np.zeros(8, dtype=np.float64)
        check(self.L.phx_world_get_phase_ms(self.h, _ptr(out)))
        return dict(zip(self.PHASES, out.tolist()))
