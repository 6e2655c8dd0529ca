"""An independent reference for the pin pass (include/phyx_amd.h PINS), written from the mechanics and not from tests/pin_spec.py:
generalised velocities, Jacobians and matrix products, numpy.linalg.solve for the 2 x 2 block — no scalar formula of the spec appears.

A body's generalised velocity is q = (vx, vy, w) and its inverse mass matrix W = diag(inv_mass, inv_mass, inv_inertia).  A pin holds
the point ra of body A on the point rb of body B (r: the anchor rotated into the world, relative to the body's centre).  The velocity
of a body's point is J(r) q with the 2 x 3 Jacobian of point_jacobian below — the ONE place where the engine's clockwise-positive
angular velocity enters; tests/test_pin_corpus_cpu.py pins that row to the integrators (a point carried through IntegratePosition
moves by J q dt).  Everything else follows from J:

    K  = J_a W_a J_a^T + J_b W_b J_b^T                       (the world has W = 0)
    dP = solve(K, -(J_b q_b - J_a q_a + beta C)),  beta = 0.2 / dt,  C = (pos_b + rb) - (pos_a + ra)
    q_a -= W_a J_a^T P,   q_b += W_b J_b^T P

unit_reference.solve runs the pass as the header defines it: every pin's K and C from the poses, the warm start P = the stored impulse
in slot order, then `iterations` sweeps in slot order.  A static body has W = 0 and is left alone by the algebra itself; a pin is inactive
where K is singular (its smallest eigenvalue is not above SINGULAR x the largest, decided in float64 whatever `dtype` is: whether a
pin is well posed is a property of the problem, not of the precision it is solved in).

`dtype` is the precision of every array and of the linear solve.  Run at float32 the same algorithm measures its own rounding noise;
deviation() is the metric in which the suite compares runs."""
import numpy as np

BETA = 0.2
SINGULAR = 1e-6          # relative eigenvalue gap below which K is treated as singular (float32 cannot resolve less than ~1e-7)


def point_jacobian(r, dtype=np.float64):
    """d(velocity of the body's point at r) / d(vx, vy, w) for the engine's clockwise-positive w: a clockwise turn carries the point
    r = (x, y) towards (y, -x)."""
    return np.array([[1.0, 0.0, r[1]], [0.0, 1.0, -r[0]]], dtype=dtype)


class State:
    """The generalised coordinates of a rigid_body_dtype array in `dtype`."""

    def __init__(self, bodies, dtype=np.float64):
        n = len(bodies)
        self.dtype = dtype
        self.pos = np.stack([bodies["pos"]["x"], bodies["pos"]["y"]], axis=1).astype(dtype)
        # the frame as a rotation matrix: columns xVector, yVector
        self.rot = np.zeros((n, 2, 2), dtype=dtype)
        self.rot[:, 0, 0], self.rot[:, 1, 0] = bodies["xv"]["x"], bodies["xv"]["y"]
        self.rot[:, 0, 1], self.rot[:, 1, 1] = bodies["yv"]["x"], bodies["yv"]["y"]
        self.q = np.stack([bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"]], axis=1).astype(dtype)
        self.w = np.stack([bodies["inv_mass"], bodies["inv_mass"], bodies["inv_inertia"]], axis=1).astype(dtype)


def _constraint(st, pin):
    """-> (a, b, J_a, J_b, K, C) of one pin in st.dtype; b = -1 and J_b = 0 for the world"""
    dt_ = st.dtype
    a, b = int(pin["body1"]), int(pin["body2"])
    ra = st.rot[a] @ np.asarray(pin["anchor1"], dtype=dt_)
    ja = point_jacobian(ra, dt_)
    k = ja @ np.diag(st.w[a]) @ ja.T
    pa = st.pos[a] + ra
    if b >= 0:
        rb = st.rot[b] @ np.asarray(pin["anchor2"], dtype=dt_)
        jb = point_jacobian(rb, dt_)
        k = k + jb @ np.diag(st.w[b]) @ jb.T
        pb = st.pos[b] + rb
    else:
        jb = np.zeros((2, 3), dtype=dt_)
        pb = np.asarray(pin["anchor2"], dtype=dt_)
    return a, b, ja, jb, k, pb - pa


def well_posed(k):
    lam = np.linalg.eigvalsh(np.asarray(k, dtype=np.float64))
    return bool(lam[0] > SINGULAR * lam[1])


def velocities(bodies):
    """(n, 3) float64 {vx, vy, w} of a rigid_body_dtype array"""
    return np.stack([bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"]], axis=1).astype(np.float64)


def deviation(q, q_ref):
    """The suite's metric: per velocity component the largest difference over the bodies, divided by that component's largest
    magnitude over the bodies in q_ref; the largest of the three.  A component that is zero on every body must agree exactly.
    (Also used on the pins' impulses, (pins, 2), in the same way.)"""
    q, q_ref = np.asarray(q, dtype=np.float64), np.asarray(q_ref, dtype=np.float64)
    worst = 0.0
    for c in range(q.shape[1]):
        diff, scale = np.abs(q[:, c] - q_ref[:, c]).max(), np.abs(q_ref[:, c]).max()
        if not np.isfinite(diff):
            return np.inf
        if diff > 0:
            worst = max(worst, diff / scale if scale > 0 else np.inf)
    return worst


def residual(bodies_before, bodies_after, pin, dt):
    """J_b q_b - J_a q_a + beta C of one pin in float64: C from the poses of bodies_before (the pass does not move them), q from
    bodies_after.  -> (the residual, K, the sum of the magnitudes of the terms it is made of)"""
    pre = State(bodies_before, np.float64)
    a, b, ja, jb, k, c = _constraint(pre, pin)
    q = velocities(bodies_after)
    cdot = -(ja @ q[a])
    terms = np.abs(ja) @ np.abs(q[a])
    if b >= 0:
        cdot = cdot + jb @ q[b]
        terms = terms + np.abs(jb) @ np.abs(q[b])
    bias = (BETA / float(dt)) * c
    return cdot + bias, k, float((terms + np.abs(bias)).sum())


def momenta(bodies):
    """(sum m v, sum (m x cross v - I w)) in float64 over bodies that all have mass and inertia: the linear momentum and the
    counter-clockwise angular momentum about the origin (w is clockwise-positive, hence the minus)."""
    m, i = 1.0 / bodies["inv_mass"].astype(np.float64), 1.0 / bodies["inv_inertia"].astype(np.float64)
    x = np.stack([bodies["pos"]["x"], bodies["pos"]["y"]], axis=1).astype(np.float64)
    q = velocities(bodies)
    lin = (m[:, None] * q[:, :2]).sum(axis=0)
    ang = (m * (x[:, 0] * q[:, 1] - x[:, 1] * q[:, 0]) - i * q[:, 2]).sum()
    return lin, ang


def momentum_scale(bodies):
    """sum m |v|, sum (m |x| |v| + I |w|): what a relative rounding error of the velocities is relative to"""
    m, i = 1.0 / bodies["inv_mass"].astype(np.float64), 1.0 / bodies["inv_inertia"].astype(np.float64)
    x = np.hypot(bodies["pos"]["x"].astype(np.float64), bodies["pos"]["y"].astype(np.float64))
    q = velocities(bodies)
    speed = np.hypot(q[:, 0], q[:, 1])
    return (m * speed).sum(), (m * x * speed + i * np.abs(q[:, 2])).sum()


# ---- a float64 free-body stepper (no contacts), for the pendulum's release height ----
def step_free(bodies, pins, order, dt, gravity, iterations=8):
    """IntegrateVelocity, the pins, IntegratePosition on a float64 state kept in `bodies` (a dict pos, angle, q, w made by free_state);
    the pins' impulses are carried in pins["impulse"] (a float64 copy made by free_state)."""
    n = len(bodies["angle"])
    q = bodies["q"]
    q[bodies["w"][:, 0] > 0, 1] += gravity * dt
    rec = np.zeros(n, dtype=_record_dtype())
    c, s = np.cos(bodies["angle"]), np.sin(bodies["angle"])
    rec["pos"]["x"], rec["pos"]["y"] = bodies["pos"][:, 0], bodies["pos"][:, 1]
    rec["xv"]["x"], rec["xv"]["y"], rec["yv"]["x"], rec["yv"]["y"] = c, s, -s, c
    rec["velocity"]["x"], rec["velocity"]["y"], rec["angular_velocity"] = q[:, 0], q[:, 1], q[:, 2]
    rec["inv_mass"], rec["inv_inertia"] = bodies["w"][:, 0], bodies["w"][:, 2]
    import unit_reference
    r = unit_reference.solve(rec, [pins], order, dt, iterations, np.float64)
    pins["impulse"][:] = r.pin_impulse
    bodies["q"] = r.q
    bodies["pos"] = bodies["pos"] + r.q[:, :2] * dt
    bodies["angle"] = bodies["angle"] - r.q[:, 2] * dt          # clockwise-positive w turns the frame by -w dt
    return float(np.hypot(r.pin_c[:, 0], r.pin_c[:, 1])[r.pin_active].max(initial=0.0))


def _record_dtype():
    v = np.dtype([("x", np.float64), ("y", np.float64)])
    return np.dtype([("pos", v), ("xv", v), ("yv", v), ("velocity", v), ("angular_velocity", np.float64), ("inv_mass", np.float64),
                     ("inv_inertia", np.float64)])


def free_state(bodies, pins):
    """float64 copies of a rigid_body_dtype array and a pin_dtype array for step_free"""
    st = State(bodies, np.float64)
    state = dict(pos=st.pos, angle=np.arctan2(st.rot[:, 1, 0], st.rot[:, 0, 0]), q=st.q, w=st.w)
    p = np.zeros(len(pins), dtype=[("body1", np.int32), ("body2", np.int32), ("anchor1", np.float64, 2), ("anchor2", np.float64, 2),
                                   ("impulse", np.float64, 2)])
    for f in ("body1", "body2", "anchor1", "anchor2", "impulse"):
        p[f] = pins[f]
    return state, p
