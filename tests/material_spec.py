"""The specification of materials (include/phyx_amd.h, MATERIALS): the pair rule, what the state-changing calls do to the per-body table,
and the solve with per-joint friction coefficients mu and restitutions e.  Plain numpy; the device is held to it byte for byte
(tests/test_materials_gpu.py), and at mu = 0.3, e = 0 it is the oracle's solve byte for byte (tests/test_materials_cpu.py).

solve_grouped restates phxo_solver_solve_grouped under STAG_COLOUR_SYNC (oracle/phx_oracle.c): groups one after the other; in a group
RefreshJoints, PreStepJoints slot by slot, the impulse sweeps and the displacement sweeps, each sweep slot by slot with the reference's
skip test and the class-synchronous static tags.  Slots that touch no common body (static ones included) commute, so a run of such
slots inside one class is evaluated as one vector operation; the order of the runs is the slot order.  Every operation is float32,
rounded on its own, in the oracle's source order; the sweeps' multiply-add pairs are one correctly rounded fmaf in the fused form."""
import numpy as np

from phyx_amd.api import material_dtype

DEFAULT_FRICTION, DEFAULT_RESTITUTION = np.float32(0.3), np.float32(0.0)
F32 = np.float32


def materials(n, friction=0.3, restitution=0.0):
    """n materials of material_dtype, each field a scalar or one value per body."""
    m = np.zeros(n, dtype=material_dtype)
    m["friction"], m["restitution"] = friction, restitution
    return m


def defaults(n):
    return materials(n)


def pair_values(ma, mb):
    """(mu, e) of contacts between bodies with materials ma, mb (records or arrays of them): mu = (fa + fb) * 0.5 (one rounded float32
    sum, an exact halving), e = the larger restitution (a > b ? a : b)."""
    fa, fb = np.asarray(ma["friction"], dtype=F32), np.asarray(mb["friction"], dtype=F32)
    ea, eb = np.asarray(ma["restitution"], dtype=F32), np.asarray(mb["restitution"], dtype=F32)
    mu = (fa + fb) * F32(0.5)
    e = np.where(ea > eb, ea, eb)
    return mu.astype(F32), e.astype(F32)


def joint_values(mat, joints):
    """Per joint (mu, e) of a joint array under the per-body materials `mat`."""
    return pair_values(mat[joints["body1"].astype(np.int64)], mat[joints["body2"].astype(np.int64)])


# ---- the state transforms -----------------------------------------------------------------------------------------------------------
def spawn(mat, count):
    """add_body / add_bodies: new bodies get the default material."""
    return np.concatenate([mat, defaults(count)])


def remove(mat, keep):
    """remove_bodies / remove_outside: the kept bodies' materials move with them, through new[] (kept order)."""
    return mat[np.asarray(keep, dtype=bool)].copy()


def set_state(n):
    """phx_world_set_state: every material is the default again."""
    return defaults(n)


def valid(friction, restitution):
    """The values phx_world_set_materials accepts: friction finite in [0, 1e6], restitution finite in [0, 1]."""
    f, e = np.asarray(friction, dtype=F32), np.asarray(restitution, dtype=F32)
    return (f >= 0) & (f <= F32(1e6)) & (e >= 0) & (e <= 1)


# ---- float32 arithmetic --------------------------------------------------------------------------------------------------------------
def fmaf(a, b, c):
    """Correctly rounded float32 fma, elementwise: the product of two float32 is exact in float64; the sum p + c rounded to odd in
    float64 (TwoSum gives the rounding error) and then rounded to float32 is the correctly rounded result (53 >= 2 * 24 + 2)."""
    a64, b64, c64 = (np.asarray(x, dtype=F32).astype(np.float64) for x in (a, b, c))
    with np.errstate(invalid="ignore", over="ignore"):
        p = a64 * b64
        s = p + c64
        bp = s - c64
        err = (p - bp) + (c64 - (s - bp))
        fin = np.isfinite(s) & np.isfinite(err)
        even = (s.view(np.int64) & 1) == 0
        bump = fin & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(bump, np.nextafter(s, toward), s)
        return s.astype(F32)


def maxf(l, r):
    """ref: base/SIMD_Scalar.h:275-278 (l > r ? l : r; a NaN on either side gives r)."""
    return np.where(l > r, l, r).astype(F32)


class _Arith:
    def __init__(self, fused):
        self.fused = bool(fused)

    def mul_add(self, a, b, acc):          # acc + a * b
        if self.fused:
            return fmaf(a, b, acc)
        with np.errstate(all="ignore"):
            return (acc + a * b).astype(F32)

    def mul_sub(self, a, b, acc):          # acc - a * b
        if self.fused:
            return fmaf(-a, b, acc)
        with np.errstate(all="ignore"):
            return (acc - a * b).astype(F32)


def _limiter(n1x, n1y, n2x, n2y, w1x, w1y, w2x, w2y, im1, ii1, im2, ii2):
    """RefreshLimiter (ref: Solver.cpp:549-590): projectors, angular projectors, compMass, 1 / (normal mass)."""
    a1 = n1x * w1y - n1y * w1x
    a2 = n2x * w2y - n2y * w2x
    c1x, c1y, c1a = n1x * im1, n1y * im1, a1 * ii1
    c2x, c2y, c2a = n2x * im2, n2y * im2, a2 * ii2
    m1 = n1x * c1x + n1y * c1y + a1 * c1a
    m2 = n2x * c2x + n2y * c2y + a2 * c2a
    m = m1 + m2
    nz = np.abs(m) > 0
    cim = np.where(nz, F32(1) / np.where(nz, m, F32(1)), F32(0)).astype(F32)
    return dict(p1x=n1x, p1y=n1y, p2x=n2x, p2y=n2y, a1=a1, a2=a2, c1x=c1x, c1y=c1y, c2x=c2x, c2y=c2y, c1a=c1a, c2a=c2a, cim=cim)


def refresh(v1, v2, q1, q2, d1, d2, n, e):
    """RefreshJoints (ref: Solver.cpp:642-693) of a vector of joints.  v = {vx, vy, w} of the solve's velocities, q = {im, ii, px, py},
    d1 / d2 = contact offsets, n = normal, e = restitution.  Returns (normal limiter, friction limiter, dstVelocity, dstDisplacing)."""
    with np.errstate(all="ignore"):
        p1x, p1y = d1[0] + q1[2], d1[1] + q1[3]
        p2x, p2y = d2[0] + q2[2], d2[1] + q2[3]
        w1x, w1y = d1[0], d1[1]
        w2x, w2y = p1x - q2[2], p1y - q2[3]
        nx, ny = n
        N = _limiter(nx, ny, -nx, -ny, w1x, w1y, w2x, w2y, q1[0], q1[1], q2[0], q2[1])
        pv1x = (q1[3] - p1y) * v1[2] + v1[0]
        pv1y = (p1x - q1[2]) * v1[2] + v1[1]
        pv2x = (q2[3] - p2y) * v2[2] + v2[0]
        pv2y = (p2x - q2[2]) * v2[2] + v2[1]
        rvx, rvy = pv1x - pv2x, pv1y - pv2y
        dv = (-e) * (rvx * nx + rvy * ny)
        depth = (p2x - p1x) * nx + (p2y - p1y) * ny
        dst = maxf(dv - F32(1), F32(0))
        n_dst = np.where(depth < F32(1), dst - F32(0.1), dst).astype(F32)
        n_dst_disp = (F32(0.1) * maxf(F32(0), depth - F32(2) * F32(1))).astype(F32)
        tx, ty = -ny, nx
        Fl = _limiter(tx, ty, -tx, -ty, w1x, w1y, w2x, w2y, q1[0], q1[1], q2[0], q2[1])
    return N, Fl, n_dst, n_dst_disp


def dst_velocity(v1, v2, q1, q2, d1, d2, n, e):
    """dstVelocity of RefreshJoints alone (hand checks)."""
    f = lambda x: tuple(np.atleast_1d(np.asarray(c, dtype=F32)) for c in x)
    return refresh(f(v1), f(v2), f(q1), f(q2), f(d1), f(d2), f(n), np.atleast_1d(F32(e)))[2]


def max_dst_velocity(bodies, cps, joints, e):
    """The largest dstVelocity RefreshJoints gives the joints (restitutions e per joint) on the solver's input `bodies` (-inf if none)."""
    if not len(joints):
        return -np.inf
    b1, b2 = joints["body1"].astype(np.int64), joints["body2"].astype(np.int64)
    cp = cps[joints["contact_point_index"].astype(np.int64)]
    f = lambda x: x.astype(F32)      # noqa: E731
    v = lambda b: (f(bodies["velocity"]["x"][b]), f(bodies["velocity"]["y"][b]), f(bodies["angular_velocity"][b]))      # noqa: E731
    q = lambda b: (f(bodies["inv_mass"][b]), f(bodies["inv_inertia"][b]), f(bodies["pos"]["x"][b]), f(bodies["pos"]["y"][b]))      # noqa: E731
    nd = refresh(v(b1), v(b2), q(b1), q(b2), (f(cp["delta1"]["x"]), f(cp["delta1"]["y"])), (f(cp["delta2"]["x"]), f(cp["delta2"]["y"])),
                 (f(cp["normal"]["x"]), f(cp["normal"]["y"])), np.asarray(e, dtype=F32))[2]
    return float(nd.max())


# ---- the grouped solve ---------------------------------------------------------------------------------------------------------------
def _runs(b1, b2, colour, begin, end):
    """[begin, end) cut into runs of slots of one class in which no body occurs twice (slot order kept)."""
    runs, start, seen = [], begin, set()
    for s in range(begin, end):
        x, y = int(b1[s]), int(b2[s])
        if s > start and (colour[s] != colour[start] or x in seen or y in seen):
            runs.append((start, s))
            start, seen = s, set()
        seen.add(x)
        seen.add(y)
    if end > start:
        runs.append((start, end))
    return runs


def solve_grouped(bodies, cps, joints, order, colour_offsets, groups, iters, pen_iters, mu, e, fused=True):
    """phxo_solver_solve_grouped(..., STAG_COLOUR_SYNC) with per-joint friction coefficients mu[j] and restitutions e[j] (indexed by the
    joint, like the joints array): updates bodies' velocities / displacing velocities and the joints' accumulated impulses in place."""
    A = _Arith(fused)
    nb, nj = len(bodies), len(joints)
    order = np.asarray(order, dtype=np.int64)
    co = np.asarray(colour_offsets, dtype=np.int64)
    go = np.asarray(groups, dtype=np.int64)
    mu = np.asarray(mu, dtype=F32)
    e = np.asarray(e, dtype=F32)
    assert len(order) == nj and len(mu) == nj and len(e) == nj
    # PrepareBodies
    im, ii = bodies["inv_mass"].astype(F32), bodies["inv_inertia"].astype(F32)
    px, py = bodies["pos"]["x"].astype(F32), bodies["pos"]["y"].astype(F32)
    imp = [bodies["velocity"]["x"].astype(F32), bodies["velocity"]["y"].astype(F32), bodies["angular_velocity"].astype(F32)]
    disp = [bodies["displacing_velocity"]["x"].astype(F32), bodies["displacing_velocity"]["y"].astype(F32),
            bodies["displacing_angular_velocity"].astype(F32)]
    tag_i, tag_d = np.full(nb, -1, np.int64), np.full(nb, -1, np.int64)
    static = (im == 0) & (ii == 0)
    colour = np.zeros(nj, dtype=np.int64)
    for k in range(len(co) - 1):
        colour[co[k]:co[k + 1]] = k
    # CopyJoints, in slot order
    jb1, jb2 = joints["body1"].astype(np.int64)[order], joints["body2"].astype(np.int64)[order]
    jcp = joints["contact_point_index"].astype(np.int64)[order]
    n_acc, f_acc = joints["normal_acc"].astype(F32)[order], joints["friction_acc"].astype(F32)[order]
    n_acc_d = np.zeros(nj, dtype=F32)
    smu, se = mu[order], e[order]
    L = {}
    n_dst, n_dst_disp = np.zeros(nj, F32), np.zeros(nj, F32)
    sw_iter = np.full((2, nb), -100, np.int64)
    sw_col = np.zeros((2, nb), np.int64)

    def productive(arr_tag, b, s, it):
        sync = static[b]
        p = arr_tag[b] > it - 2
        if it == 0:
            ps = np.ones(len(b), bool)
        else:
            ps = (sw_iter[(it - 1) & 1, b] == it - 1) | ((sw_iter[it & 1, b] == it) & (sw_col[it & 1, b] < colour[s]))
        return np.where(sync, ps, p)

    def mark(arr_tag, b, s, it):
        p = it & 1
        st = static[b]
        bs, ss = b[st], s[st]
        new = sw_iter[p, bs] != it
        lower = ~new & (colour[ss] < sw_col[p, bs])
        sw_col[p, bs] = np.where(new | lower, colour[ss], sw_col[p, bs])
        sw_iter[p, bs] = it
        arr_tag[b] = it

    def visit(s, it, which):
        b1, b2 = jb1[s], jb2[s]
        tags = tag_d if which else tag_i
        go_ = productive(tags, b1, s, it) | productive(tags, b2, s, it)
        s, b1, b2 = s[go_], b1[go_], b2[go_]
        if not len(s):
            return False
        arr = disp if which else imp
        N = {k: v[s] for k, v in L["n"].items()}
        v1x, v1y, w1 = arr[0][b1], arr[1][b1], arr[2][b1]
        v2x, v2y, w2 = arr[0][b2], arr[1][b2], arr[2][b2]
        with np.errstate(all="ignore"):
            dv = n_dst_disp[s] if which else n_dst[s]
            dv = A.mul_sub(N["p1x"], v1x, dv); dv = A.mul_sub(N["p1y"], v1y, dv); dv = A.mul_sub(N["a1"], w1, dv)
            dv = A.mul_sub(N["p2x"], v2x, dv); dv = A.mul_sub(N["p2y"], v2y, dv); dv = A.mul_sub(N["a2"], w2, dv)
            acc = n_acc_d if which else n_acc
            dn = (dv * N["cim"]).astype(F32)
            dn = maxf(dn, -acc[s])
            v1x = A.mul_add(N["c1x"], dn, v1x); v1y = A.mul_add(N["c1y"], dn, v1y); w1 = A.mul_add(N["c1a"], dn, w1)
            v2x = A.mul_add(N["c2x"], dn, v2x); v2y = A.mul_add(N["c2y"], dn, v2y); w2 = A.mul_add(N["c2a"], dn, w2)
            acc[s] = (acc[s] + dn).astype(F32)
            if which:
                prod = np.abs(dn) > F32(1e-4)
            else:
                Fl = {k: v[s] for k, v in L["f"].items()}
                fv = np.zeros(len(s), F32)
                fv = A.mul_sub(Fl["p1x"], v1x, fv); fv = A.mul_sub(Fl["p1y"], v1y, fv); fv = A.mul_sub(Fl["a1"], w1, fv)
                fv = A.mul_sub(Fl["p2x"], v2x, fv); fv = A.mul_sub(Fl["p2y"], v2y, fv); fv = A.mul_sub(Fl["a2"], w2, fv)
                df = (fv * Fl["cim"]).astype(F32)
                reaction, facc = n_acc[s], f_acc[s]
                force = (facc + df).astype(F32)
                limit = (reaction * smu[s]).astype(F32)
                signed_limit = np.where(force < 0, -limit, limit).astype(F32)
                adjusted = (signed_limit - facc).astype(F32)
                df = np.where(np.abs(force) > limit, adjusted, df).astype(F32)
                f_acc[s] = (facc + df).astype(F32)
                v1x = A.mul_add(Fl["c1x"], df, v1x); v1y = A.mul_add(Fl["c1y"], df, v1y); w1 = A.mul_add(Fl["c1a"], df, w1)
                v2x = A.mul_add(Fl["c2x"], df, v2x); v2y = A.mul_add(Fl["c2y"], df, v2y); w2 = A.mul_add(Fl["c2a"], df, w2)
                prod = maxf(np.abs(dn), np.abs(df)) > F32(1e-4)
        arr[0][b1], arr[1][b1], arr[2][b1] = v1x, v1y, w1
        arr[0][b2], arr[1][b2], arr[2][b2] = v2x, v2y, w2
        if prod.any():
            mark(tags, b1[prod], s[prod], it)
            mark(tags, b2[prod], s[prod], it)
        return bool(prod.any())

    for g in range(len(go) - 1):
        b, en = int(go[g]), int(go[g + 1])
        if en <= b:
            continue
        tag_i[static], tag_d[static] = -1, -1
        s = np.arange(b, en)
        # RefreshJoints of the group
        b1, b2 = jb1[s], jb2[s]
        cp = cps[jcp[s]]
        f = lambda x: x.astype(F32)
        N, Fl, nd, ndd = refresh((imp[0][b1], imp[1][b1], imp[2][b1]), (imp[0][b2], imp[1][b2], imp[2][b2]),
                                 (im[b1], ii[b1], px[b1], py[b1]), (im[b2], ii[b2], px[b2], py[b2]),
                                 (f(cp["delta1"]["x"]), f(cp["delta1"]["y"])), (f(cp["delta2"]["x"]), f(cp["delta2"]["y"])),
                                 (f(cp["normal"]["x"]), f(cp["normal"]["y"])), se[s])
        if not L:
            L["n"] = {k: np.zeros(nj, F32) for k in N}
            L["f"] = {k: np.zeros(nj, F32) for k in Fl}
        for k in N:
            L["n"][k][s] = N[k]
            L["f"][k][s] = Fl[k]
        n_dst[s], n_dst_disp[s], n_acc_d[s] = nd, ndd, 0
        runs = [np.arange(r0, r1) for r0, r1 in _runs(jb1, jb2, colour, b, en)]
        # PreStepJoints, slot by slot (run by run)
        for r in runs:
            b1, b2 = jb1[r], jb2[r]
            N = {k: v[r] for k, v in L["n"].items()}
            Fl = {k: v[r] for k, v in L["f"].items()}
            v1x, v1y, w1 = imp[0][b1], imp[1][b1], imp[2][b1]
            v2x, v2y, w2 = imp[0][b2], imp[1][b2], imp[2][b2]
            with np.errstate(all="ignore"):
                for Q, a in ((N, n_acc[r]), (Fl, f_acc[r])):
                    v1x = A.mul_add(Q["c1x"], a, v1x); v1y = A.mul_add(Q["c1y"], a, v1y); w1 = A.mul_add(Q["c1a"], a, w1)
                    v2x = A.mul_add(Q["c2x"], a, v2x); v2y = A.mul_add(Q["c2y"], a, v2y); w2 = A.mul_add(Q["c2a"], a, w2)
            imp[0][b1], imp[1][b1], imp[2][b1] = v1x, v1y, w1
            imp[0][b2], imp[1][b2], imp[2][b2] = v2x, v2y, w2
        for which, count in ((0, iters), (1, pen_iters)):
            sw_iter[:, static] = -100
            sw_col[:, static] = 0
            for it in range(count):
                p = False
                for r in runs:
                    p |= visit(r, it, which)
                if not p:
                    break
    # FinishJoints, FinishBodies
    joints["normal_acc"][order] = n_acc
    joints["friction_acc"][order] = f_acc
    bodies["velocity"]["x"], bodies["velocity"]["y"], bodies["angular_velocity"] = imp
    bodies["displacing_velocity"]["x"], bodies["displacing_velocity"]["y"], bodies["displacing_angular_velocity"] = disp
