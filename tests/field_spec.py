"""The definition of the force fields (include/phyx_amd.h FORCE FIELDS): scalar float32, every operation rounded on its own, no fused
multiply-add, IEEE division and square root.  The device kernels (phyx_amd/csrc/field_kernels.h) follow this file operation for
operation, and the GPU tests compare bytes.

`fields` is a field_dtype array (phyx_amd.uniform_field / radial_field / drag_field rows), `bodies` a rigid_body_dtype array (the
oracle World's own, or a copy), `categories` the bodies' collision-filter categories (None: no filter was ever set, every body has 1).
"""
import numpy as np

F = np.float32
UNIFORM, RADIAL, DRAG = 0, 1, 2
ALL, BOX, DISC = 0, 1, 2
FORCE = 1
D_MIN = F(2.0 ** -10)      # a RADIAL field has no direction closer to its centre than this


def inside(f, x, y):
    """Membership of the centre (x, y), closed; every test is written so that a NaN coordinate is outside (ALL has no test)."""
    r = [F(v) for v in f["region"]]
    shape = int(f["shape"])
    if shape == BOX:
        return bool(x >= r[0] and x <= r[2] and y >= r[1] and y <= r[3])
    if shape == DISC:
        dx, dy = x - r[0], y - r[1]
        return bool(dx * dx + dy * dy <= r[2] * r[2])
    return True


def acceleration(f, dt, x, y, vx, vy, w, inv_mass, inv_inertia):
    """The {ax, ay, angular} field `f` gives a body that passed the who-rule, or None: no contribution (nothing is added, not + 0)."""
    dt = F(dt)
    if not inside(f, x, y):
        return None
    v = [F(u) for u in f["value"]]
    kind = int(f["kind"])
    with np.errstate(all="ignore"):
        if kind == UNIFORM:
            a = [v[0], v[1], v[2]]
        elif kind == RADIAL:
            dx, dy = x - v[0], y - v[1]
            d = np.sqrt(dx * dx + dy * dy)
            if not d > D_MIN:
                return None
            mag = v[2]
            if v[3] > F(0):
                t = F(1) - d / v[3]
                if not t > F(0):
                    return None
                mag = v[2] * t
            a = [(dx / d) * mag, (dy / d) * mag, F(0)]
        else:
            kl, ka = v[2] * dt, v[3] * dt
            c = (kl if kl < F(1) else F(1)) / dt
            ca = (ka if ka < F(1) else F(1)) / dt
            a = [(v[0] - vx) * c, (v[1] - vy) * c, (F(0) - w) * ca]
        if int(f["flags"]) & FORCE:
            a = [a[0] * inv_mass, a[1] * inv_mass, a[2] * inv_inertia]
    return a


def sums(fields, dt, bodies, start, categories=None):
    """start[i] + a(field 0) + a(field 1) + ... per body, in list order, each + rounded: (N, 3) float32.  A body with inv_mass <= 0
    (a static body, a sleeper) or whose category misses a field's mask keeps its start."""
    out = np.array(start, dtype=np.float32).reshape(len(bodies), 3).copy()
    for i in range(len(bodies)):
        b = bodies[i]
        m, ii = F(b["inv_mass"]), F(b["inv_inertia"])
        if not m > F(0):
            continue
        cat = 1 if categories is None else int(categories[i])
        x, y = F(b["pos"]["x"]), F(b["pos"]["y"])
        vx, vy, w = F(b["velocity"]["x"]), F(b["velocity"]["y"]), F(b["angular_velocity"])
        s = [F(out[i, 0]), F(out[i, 1]), F(out[i, 2])]
        for f in fields:
            if not (cat & int(f["mask"])):
                continue
            a = acceleration(f, dt, x, y, vx, vy, w, m, ii)
            if a is None:
                continue
            with np.errstate(all="ignore"):
                s = [s[0] + a[0], s[1] + a[1], s[2] + a[2]]
        out[i] = s
    return out


def pending_of(bodies):
    return np.stack([bodies["acceleration"]["x"], bodies["acceleration"]["y"], bodies["angular_acceleration"]], axis=1).astype(np.float32)


def velocities_of(bodies):
    return np.stack([bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"]], axis=1).astype(np.float32)


def step_accelerations(fields, dt, bodies, categories=None):
    """What the pass at the head of a step leaves for IntegrateVelocity: pending + the fields, from the records' own pending
    accelerations (zero where nothing is pending)."""
    return sums(fields, dt, bodies, pending_of(bodies), categories)


def pulse(fields, bodies, categories=None):
    """phx_world_pulse_fields: the velocities after it, vel + a(field 0) + a(field 1) + ... with dt = 1 (a DRAG reads the velocity
    the call found)."""
    return sums(fields, 1.0, bodies, velocities_of(bodies), categories)


def impulse(body, jx, jy, px, py):
    """phx_world_apply_impulses on one record: its {vx, vy, w} after the impulse (jx, jy) at the world point (px, py).  A body with
    inv_mass <= 0 is skipped.  The angular sign is the engine's clockwise-positive one (pin_spec.apply)."""
    m, ii = F(body["inv_mass"]), F(body["inv_inertia"])
    vx, vy, w = F(body["velocity"]["x"]), F(body["velocity"]["y"]), F(body["angular_velocity"])
    if not m > F(0):
        return vx, vy, w
    jx, jy = F(jx), F(jy)
    rx, ry = F(px) - F(body["pos"]["x"]), F(py) - F(body["pos"]["y"])
    with np.errstate(all="ignore"):
        return vx + m * jx, vy + m * jy, w - ii * (rx * jy - ry * jx)
