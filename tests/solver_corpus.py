"""Directed solver inputs: joint VALUES the scene and random generators never feed (tests/test_solver_corpus_cpu.py proves on the CPU
which arms of the solve each one takes, with the oracle's solver trace — oracle/phx_oracle.h PHXO_ST_* —, tests/test_solver_corpus_gpu.py
solves them on the device).  Two forms:

motifs()   isolated islands of one to three joints, each named for the labels it is built to take.  The islands share no body, so the
           order in which a schedule sweeps them cannot change what each one does; the three-joint chains take their labels under every
           permutation of their joints.  Every motif is repeated COPIES times with other contact-point ids (other priorities, other lanes).
dress()    re-values a path_edges.units_state topology with the same value classes, for the kernels only a large component reaches.

Conventions of a motif: every body sits at the origin and delta2 = delta1 + depth * normal, so the refresh's depth is the number
given and a joint without a lever arm (delta1 = 0) has no angular term: with unit inverse masses compInvMass is exactly 0.5 on both
limiters and the impulses below are exact in either arithmetic form.  Body 1 is pushed along +normal, the friction axis is
(-normal.y, normal.x).

A label is `name` or `name@k`: reached only if its phase runs at least k sweeps (impulse labels n_/f_/prod_/i_ need ci >= max(k, 1),
displacement labels d_ need pi >= max(k, 1)); labels of the refresh, the bodies and PreStep are reached whatever the iteration counts.

Not reachable, with the reason:
  limit < 0            accN >= 0 after a joint's first visit (dn >= -accN is the normal clamp), so limit = 0.3 * accN >= 0.
  cimF_zero alone      both limiters' masses are sums of the same non-negative terms: one is zero only where both bodies are static.
`f_force_eq_limit` (|force| == limit > 0) IS reached: a warm start whose PreStep cancels the relative velocity exactly leaves dn = df = 0
and force = the warm friction impulse = 0.3f * the warm normal impulse."""
import numpy as np

import phyx_amd

COPIES = 5
F32 = np.float32
SUB = 1e-39              # a subnormal float
TINY = 1.4e-45           # the smallest one: half of it rounds to zero


def _label(l):
    name, _, k = l.partition("@")
    return name, int(k or 0)


def required(labels, ci, pi):
    """the names among `labels` (with their @k) that a solve of ci / pi sweeps must reach"""
    out = set()
    for l in labels:
        name, k = _label(l)
        if name.startswith(("n_", "f_", "prod_", "i_")):
            ok = ci >= max(k, 1)
        elif name.startswith("d_"):
            ok = pi >= max(k, 1)
        else:
            ok = True
        if ok:
            out.add(name)
    return out




class _Builder:
    def __init__(self):
        self.bodies, self.cps, self.joints = [], [], []

    def body(self, v=(0.0, 0.0, 0.0), dv=(0.0, 0.0, 0.0), im=1.0, ii=0.05, static=False):
        """-> body index; v / dv = (x, y, angular) of the velocity / the displacing velocity"""
        self.bodies.append((v, dv, 0.0 if static else im, 0.0 if static else ii))
        return len(self.bodies) - 1

    def joint(self, b1, b2, depth=1.5, normal=(0.0, 1.0), r=(0.0, 0.0), n_acc=0.0, f_acc=0.0, follows=False):
        """a joint on (b1, b2); follows: the second joint of the unit the previous joint() call began (same body pair)"""
        if follows:
            assert self.joints and self.joints[-1][1:3] == (b1, b2) and len(self.cps) % 2 == 1
        elif len(self.cps) % 2:
            self.cps.append(None)                      # a unit begins at an even contact-point id
        self.cps.append((r, (r[0] + depth * normal[0], r[1] + depth * normal[1]), normal))
        self.joints.append((len(self.cps) - 1, b1, b2, n_acc, f_acc))


# ---- the motifs: name -> (builder function, labels, uses a static body, labels only the fp16 form takes, labels the fp16 form loses) --
# Under 16-bit body state a motif keeps its labels (most values here are halves: 0.25, 0.5, 1, 2, 3) but those in drop16, each with
# the reason beside it.
MOTIFS = {}


def motif(name, labels, static=False, labels16=(), drop16=()):
    def deco(fn):
        assert set(drop16) <= {_label(l)[0] for l in labels}
        MOTIFS[name] = (fn, tuple(labels), static, tuple(labels16), tuple(drop16))
        return fn
    return deco


@motif("resting contact, depth 1.5, cold", ["depth_1_2", "cold", "n_clamp_tie", "f_free", "f_limit_zero", "prod_none", "d_clamped", "d_unproductive"])
def _(b):
    b.joint(b.body(), b.body())


@motif("approach at 2, depth 0.5, sliding at +1", ["depth_lt1", "n_free", "f_clamp_pos", "prod_both"])
def _(b):
    b.joint(b.body(v=(1.0, -2.0, 0.0)), b.body(), depth=0.5)


@motif("approach at 2, depth 0.5, sliding at -1", ["depth_lt1", "n_free", "f_clamp_neg", "prod_both"])
def _(b):
    b.joint(b.body(v=(-1.0, -2.0, 0.0)), b.body(), depth=0.5)


@motif("approach at 2, depth 1.5, slow slide 0.25 inside the cone", ["n_free", "f_free", "prod_both"])
def _(b):
    b.joint(b.body(v=(0.25, -2.0, 0.0)), b.body())


@motif("approach at 2, no slide", ["n_free", "f_free", "prod_dn"])
def _(b):
    b.joint(b.body(v=(0.0, -2.0, 0.0)), b.body())


@motif("two-joint unit, dynamic pair, approach at 2 with lever arms", ["n_free", "prod_both"])
def _(b):
    a, c = b.body(v=(0.5, -2.0, 0.0)), b.body()
    b.joint(a, c, r=(0.5, -0.25))
    b.joint(a, c, r=(-0.5, -0.25), follows=True)


@motif("separating at 3 under a warm normal impulse 0.5", ["warm_normal", "n_clamp_strict", "f_limit_zero"])
def _(b):
    b.joint(b.body(v=(0.0, 3.0, 0.0)), b.body(), n_acc=0.5)


@motif("warm normal impulse 0.5 withdrawn exactly: the normal clamp on a tie", ["warm_normal", "n_clamp_tie"])
def _(b):
    b.joint(b.body(), b.body(), n_acc=0.5)


@motif("warm start normal 1, friction 0.1, sliding on", ["warm_normal", "warm_friction", "n_free", "f_free", "prod_df"])
def _(b):
    b.joint(b.body(v=(0.5, -1.0, 0.0)), b.body(v=(0.0, 1.0, 0.0)), n_acc=1.0, f_acc=0.1)


@motif("warm friction exactly at the cone: |force| == limit", ["warm_friction", "f_force_eq_limit", "f_free", "prod_none"],
       drop16=["f_force_eq_limit", "f_free"])             # (0.3f is no half: the rounded velocities no longer cancel PreStep exactly)
def _(b):
    mu = float(F32(0.3))
    b.joint(b.body(v=(mu, -1.0, 0.0)), b.body(v=(-mu, 1.0, 0.0)), n_acc=1.0, f_acc=mu)


@motif("approach at 1e-39, depth 1.5", ["depth_1_2", "i_subnormal", "n_free", "prod_none"], labels16=["h_flushed"],
       drop16=["i_subnormal", "n_free"])                  # (1e-39 is zero as a half: a resting contact, dn = 0 on the tie)
def _(b):
    b.joint(b.body(v=(0.0, -SUB, 0.0)), b.body())


@motif("friction underflow onto a -0.0 warm start", ["cold", "f_force_negzero", "i_subnormal", "f_limit_zero"], labels16=["h_flushed"],
       drop16=["f_force_negzero", "i_subnormal"])         # (-1.4e-45 is -0.0 as a half: 0 - (-1 * -0.0) is +0.0, the force +0.0)
def _(b):
    b.joint(b.body(v=(-TINY, 0.0, 0.0)), b.body(), f_acc=-0.0)


@motif("subnormal slip 3e-40 under a warm normal impulse 1", ["warm_normal", "i_subnormal", "f_free", "prod_none"], labels16=["h_flushed"],
       drop16=["i_subnormal"])                            # (3e-40 is zero as a half)
def _(b):
    b.joint(b.body(v=(3e-40, -1.0, 0.0)), b.body(v=(0.0, 1.0, 0.0)), n_acc=1.0)


@motif("deep contact 2.5", ["depth_gt2", "d_free", "d_productive", "d_unproductive@2"])
def _(b):
    b.joint(b.body(), b.body(), depth=2.5)


@motif("displacing velocity 0.25 into a shallow contact", ["disp_in_nonzero", "d_free", "d_productive"])
def _(b):
    b.joint(b.body(dv=(0.0, -0.25, 0.0)), b.body())


@motif("displacing velocity 0.25 out of a shallow contact", ["disp_in_nonzero", "d_clamped", "d_unproductive"])
def _(b):
    b.joint(b.body(dv=(0.0, 0.25, 0.125)), b.body(), r=(0.5, 0.0))


@motif("displacing velocity -0.0", ["disp_in_negzero", "d_clamped", "d_unproductive"])
def _(b):
    b.joint(b.body(dv=(-0.0, -0.0, -0.0)), b.body(dv=(0.0, -0.0, 0.0)))


@motif("displacing velocity 1e-39 into a shallow contact", ["disp_in_nonzero", "d_subnormal", "d_free", "d_unproductive"], labels16=["h_flushed"],
       drop16=["disp_in_nonzero", "d_subnormal", "d_free"])      # (zero as a half: nothing displaces, di = 0 on the clamp)
def _(b):
    b.joint(b.body(dv=(0.0, -SUB, 0.0)), b.body())


# (the normal points down, from the box to the belt: the belt's -2 along y is an approach, its 3 along x drags the box)
@motif("conveyor: static body2 moving at (3, -2, 0.5)", ["static_body2", "static_moving", "n_free", "f_clamp_pos", "prod_both"], static=True)
def _(b):
    b.joint(b.body(), b.body(v=(3.0, -2.0, 0.5), static=True), normal=(0.0, -1.0), r=(0.5, 0.25))


# A static body's -0.0 words.  The reference stores `word + 0 * impulse` into a static body like into any other (ref: Solver.cpp:866-889,
# 973-996): -0.0 + (+0.0) is +0.0, so the first visit whose product is a POSITIVE zero turns the word into +0.0 and it stays so.  Here
# velocity.y and displacing_velocity.y of the belt are -0.0, compMass2.y = (+1) * 0 and both first impulses are positive (the box
# comes down at 2, the contact is 0.5 too deep): the oracle returns +0.0 for both words.
STATIC_NEGZERO = "conveyor with -0.0 words: static body2 at (3, -0.0, 0.5), displacing (0, -0.0, 0), depth 2.5"


@motif(STATIC_NEGZERO, ["static_body2", "static_moving", "disp_in_negzero", "depth_gt2", "n_free", "d_free", "d_productive"], static=True)
def _(b):
    b.joint(b.body(v=(0.0, 2.0, 0.0)), b.body(v=(3.0, -0.0, 0.5), dv=(0.0, -0.0, 0.0), static=True), depth=2.5, normal=(0.0, -1.0), r=(0.5, 0.25))


@motif("kinematic platform: static body1 moving at (-1, -2, -0.25)", ["static_body1", "static_moving", "n_free", "prod_both"], static=True)
def _(b):
    b.joint(b.body(v=(-1.0, -2.0, -0.25), static=True), b.body(), r=(-0.5, 0.25))


@motif("two-joint unit, static body1", ["static_body1", "static_moving", "n_free"], static=True)
def _(b):
    s, a = b.body(v=(0.5, -1.0, 0.25), static=True), b.body(v=(0.0, 1.0, 0.0))
    b.joint(s, a, r=(0.5, 0.25))
    b.joint(s, a, r=(-0.5, 0.25), follows=True)


@motif("two-joint unit, static body2, deep", ["static_body2", "depth_gt2", "d_productive"], static=True)
def _(b):
    a, s = b.body(v=(0.25, -1.0, 0.0)), b.body(static=True)
    b.joint(a, s, depth=2.5, r=(0.5, -0.25))
    b.joint(a, s, depth=2.25, r=(-0.5, -0.25), follows=True)


@motif("static on static", ["static_both", "static_moving", "cimN_zero", "cimF_zero", "n_clamp_tie", "prod_none"], static=True)
def _(b):
    b.joint(b.body(v=(1.0, -1.0, 0.5), static=True), b.body(static=True), r=(0.5, 0.25))


@motif("two-joint unit, both bodies static", ["static_both", "cimN_zero", "cimF_zero"], static=True)
def _(b):
    s, t = b.body(static=True), b.body(v=(0.0, 2.0, 0.0), static=True)
    b.joint(s, t, depth=2.5)
    b.joint(s, t, depth=0.5, r=(0.25, 0.0), follows=True)


# Three-joint chains A - B - C - D.  J2 = (C, D) works along x; J1 = (B, C) along y is evaluated as long as C's tag is fresh and J0 = (A, B)
# only while B's is.  SLEEPER: J1 never has anything to do (no approach along y, and with accN = 0 its friction cone is a point), so J0 is
# evaluated in sweep 0 and skipped in sweep 1, in both phases, wherever the three joints stand in the sweep.
@motif("sleeper chain: a resting joint two links from the only working one", ["i_skipped@2", "d_skipped@2", "f_limit_zero", "prod_none", "prod_dn"])
def _(b):
    a, bb, c, d = b.body(), b.body(), b.body(v=(-2.0, 0.0, 0.0)), b.body()
    b.joint(a, bb)
    b.joint(bb, c)
    b.joint(c, d, depth=2.5, normal=(1.0, 0.0))


# WAKING: J2 has lever arms on both axes, so its friction impulse turns C and disturbs its own normal row: it stays productive for
# several sweeps and lifts C by a shrinking step each visit (C's y velocity after 1, 2, 3 visits of J2 alone: 0.4, 0.44, 0.444 in both
# arithmetic forms).  B leaves C (and A) at 0.442, between the second and the third: whichever of J1, J2 a sweep visits first, J1 has
# seen at most 0.44 by the end of sweep 1 (unproductive: J0 is skipped in sweep 1 wherever it stands) and sees 0.444 in sweep 2 or 3
# (productive: B's tag is raised and J0 is evaluated again, in sweep 4 at the latest).
WAKE = dict(r=(0.5, 0.5), ii=2.0, vx=-4.0, speed=0.442)


@motif("waking chain: the middle joint turns productive after the first sweeps", ["i_skipped@2", "i_resumed@5"])
def _(b):
    a, bb = b.body(), b.body(v=(0.0, WAKE["speed"], 0.0))
    c, d = b.body(v=(WAKE["vx"], 0.0, 0.0), ii=WAKE["ii"]), b.body(ii=WAKE["ii"])
    b.joint(bb, a)                                             # (B leaves A too: nothing to do until J1 stops B)
    b.joint(bb, c)
    b.joint(c, d, normal=(1.0, 0.0), r=WAKE["r"])


# DEEP: three contacts in a row, each 2^-7 deeper than the displacement pass allows, push against each other: the displacement sweeps
# shrink the error by a constant factor and end in their fourth or fifth sweep (all six orders, both arithmetic forms) while the
# impulses, with nothing moving, end in their first.  Whatever else shares its group (no other motif runs more than two
# displacement sweeps), that group's displacement sweeps outlast three impulse sweeps and end before the sixth.
DEEP_CHAIN_SWEEPS = (4, 5)


@motif("deep chain: three contacts just past the allowed penetration", ["depth_gt2", "d_free", "d_productive@3", "d_unproductive@5", "prod_none"])
def _(b):
    a, bb, c, d = b.body(), b.body(), b.body(), b.body()
    b.joint(a, bb, depth=2.0 + 2.0 ** -7)
    b.joint(bb, c, depth=2.0 + 2.0 ** -7)
    b.joint(c, d, depth=2.0 + 2.0 ** -7)


# fp16 body state: what the half stores see.  The incoming words are rounded when the group's working copy is made.
@motif("half tie: a velocity exactly between two halves", ["n_free"], labels16=["h_tie"])
def _(b):
    b.joint(b.body(v=(1.0 + 2.0 ** -11, -2.0, 3.0 * 2.0 ** -26)), b.body())


@motif("half subnormal: approach at 3e-6", ["n_free"], labels16=["h_subnormal"])
def _(b):
    b.joint(b.body(v=(0.0, -3e-6, 0.0)), b.body())


@motif("half flush: approach at 1e-9", ["n_free"], labels16=["h_flushed"], drop16=["n_free"])      # (zero as a half: dn = 0 on the tie)
def _(b):
    b.joint(b.body(v=(0.0, -1e-9, 0.0)), b.body())


CHAINS = [n for n in MOTIFS if "chain" in n]                     # the three-joint motifs: checked under all 6 permutations
NO_ISLAND = ("static on static", "two-joint unit, both bodies static")   # joints the reference's GatherIslands gives to no island
GROUP_LABELS = ("g_imp_early", "g_imp_full", "g_disp_first", "g_disp_early", "g_disp_full", "g_imp_outlasts", "g_disp_outlasts")
ITERS = [(6, 3), (3, 6), (1, 1), (9, 0)]
# Per-group labels that hold for ANY grouping of the islands (a device group is a bin of several; its sweeps are its slowest
# island's): one sweep of one is all of them; without displacement sweeps the impulses outlast them; no motif alone but the deep chain
# runs more than two displacement sweeps (tests/test_solver_corpus_cpu.py), so the deep chain's group runs three of three
# displacement sweeps, or 4..5 of six, which three impulse sweeps do not outlast.  The other
# labels depend on which islands share a group: the CPU test requires all seven over the four iteration counts on the host builder's groups.
GROUP_LABELS_ANY_GROUPING = {(1, 1): {"g_imp_full", "g_disp_full"}, (9, 0): {"g_imp_outlasts"}, (6, 3): {"g_disp_full"},
                             (3, 6): {"g_disp_early", "g_disp_outlasts"}}


class Corpus:
    """bodies, cps, joints (numpy, the solver's input) and instances = [(motif name, copy, joint indices)]"""

    def __init__(self, bodies, cps, joints, instances):
        self.bodies, self.cps, self.joints, self.instances = bodies, cps, joints, instances

    @property
    def state(self):
        return self.bodies, self.cps, self.joints


def _assemble(builds, seed):
    """builds: [(name, copy)] in contact-point order -> Corpus; the joint array is shuffled"""
    b = _Builder()
    spans = []
    for name, copy in builds:
        j0 = len(b.joints)
        MOTIFS[name][0](b)
        spans.append((name, copy, j0, len(b.joints)))
    if len(b.cps) % 2:
        b.cps.append(None)
    bodies = np.zeros(len(b.bodies), dtype=phyx_amd.rigid_body_dtype)
    bodies["index"] = np.arange(len(bodies))
    for i, (v, dv, im, ii) in enumerate(b.bodies):
        bodies["velocity"]["x"][i], bodies["velocity"]["y"][i], bodies["angular_velocity"][i] = v
        bodies["displacing_velocity"]["x"][i], bodies["displacing_velocity"]["y"][i], bodies["displacing_angular_velocity"][i] = dv
        bodies["inv_mass"][i], bodies["inv_inertia"][i] = im, ii
    cps = np.zeros(len(b.cps), dtype=phyx_amd.contact_point_dtype)
    cps["normal"]["y"] = 1.0                                    # (the ids no joint uses)
    for i, c in enumerate(b.cps):
        if c is not None:
            (cps["delta1"]["x"][i], cps["delta1"]["y"][i]), (cps["delta2"]["x"][i], cps["delta2"]["y"][i]), (cps["normal"]["x"][i], cps["normal"]["y"][i]) = c
    nj = len(b.joints)
    perm = np.random.default_rng(seed).permutation(nj) if seed is not None else np.arange(nj)
    joints = np.zeros(nj, dtype=phyx_amd.contact_joint_dtype)
    for k, (cp, b1, b2, n_acc, f_acc) in enumerate(b.joints):
        joints[perm[k]] = (cp, b1, b2, n_acc, f_acc)
    return Corpus(bodies, cps, joints, [(name, copy, perm[j0:j1]) for name, copy, j0, j1 in spans])


# Motifs left out of the GPU parity runs (tests/test_solver_corpus_gpu.py test_motifs) by name, each with the mismatch; they stay in the
# corpus and in the CPU tests.
GPU_LEFT_OUT = {
    STATIC_NEGZERO: "the static body's velocity.y and displacing_velocity.y: the oracle (and the reference, which stores word + 0 * impulse) "
                    "returns 0x00000000 for both, the device, which never stores a static body's record, returns the 0x80000000 it was given; "
                    "every other byte is equal (test_a_static_bodys_negative_zero_words_stay: DESIGN.md section 9 item 7)",
}


def motifs(dynamic_only=False, seed=17, leave_out=()):
    """Every motif (dynamic_only: those without a static body, so that no wave of the island kernel touches one) COPIES times; copy k
    begins 3 k motifs further down the list, so a motif's copies get contact-point ids of no common pattern."""
    names = [n for n in MOTIFS if not (dynamic_only and MOTIFS[n][2]) and n not in leave_out]
    builds = [(names[(i + 3 * k) % len(names)], k) for k in range(COPIES) for i in range(len(names))]
    return _assemble(builds, seed)


def motif_alone(name, perm=None):
    """One copy of one motif as a whole input, its joints in the order perm (default: as built)."""
    c = _assemble([(name, 0)], None)
    if perm is not None:
        c.joints = c.joints[np.asarray(perm)].copy()
    return c


def motif_labels(name, ci, pi, bits=32):
    fn, labels, static, labels16, drop16 = MOTIFS[name]
    if bits == 16:
        return (required(labels, ci, pi) - set(drop16)) | set(labels16)
    return required(labels, ci, pi)


def finite(bodies, joints):
    """every word a solve writes is finite"""
    return all(np.isfinite(bodies[f][n]).all() for f in ("velocity", "displacing_velocity") for n in ("x", "y")) \
        and np.isfinite(bodies["angular_velocity"]).all() and np.isfinite(bodies["displacing_angular_velocity"]).all() \
        and np.isfinite(joints["normal_acc"]).all() and np.isfinite(joints["friction_acc"]).all()


def largest_body_word(bodies):
    """the largest magnitude among the six velocity words of every body"""
    return max([np.abs(bodies[f][n]).max() for f in ("velocity", "displacing_velocity") for n in ("x", "y")]
               + [np.abs(bodies["angular_velocity"]).max(), np.abs(bodies["displacing_angular_velocity"]).max()])


def corpus_labels(names, ci, pi, bits=32):
    return set().union(*(motif_labels(n, ci, pi, bits) for n in names))


# every per-joint label of the trace but the fp16 ones is some motif's (the fp16 ones are the fp16 form's)
ALL_JOINT_LABELS = ("depth_lt1 depth_1_2 depth_gt2 cimN_zero cimF_zero static_body1 static_body2 static_both static_moving disp_in_nonzero "
                    "disp_in_negzero warm_normal warm_friction cold n_free n_clamp_strict n_clamp_tie f_free f_clamp_pos f_clamp_neg f_limit_zero "
                    "f_force_negzero f_force_eq_limit prod_dn prod_df prod_both prod_none i_subnormal i_skipped i_resumed d_free d_clamped "
                    "d_productive d_unproductive d_skipped d_subnormal").split()
HALF_LABELS = ("h_subnormal", "h_flushed", "h_tie")


# ---- dress(): the same value classes dealt over a path_edges topology ---------------------------------------------------------------
# name -> the labels the host schedule's replay must reach (tests/test_solver_corpus_cpu.py) and the device's (tests/
# test_solver_corpus_gpu.py), at both DRESSED_ITERS and in both arithmetic forms: every per-joint label the topology and the dealt
# values admit.  Left out, with the reason:
#   static_both, cimN_zero, cimF_zero   a case has at most one static body: no joint between two
#   static_body1                        the one static body on joints (static_spokes' body 0) is every star's spoke, a unit's body 2
#   static_body2, static_moving         only static_spokes has a joint on a static body (tail_of_3's static body 0 carries none)
#   f_force_eq_limit, f_force_negzero   exact cancellations: every body here carries several joints and a random velocity or lever arm, and
#                                       no sweep of the replay lands on one (f_force_negzero: twice in static_spokes in the source arithmetic form, never in the fused one)
#   i_resumed                           a skipped joint is evaluated again only if a neighbour turns productive after having been quiet; within
#                                       the six sweeps run here the residuals of these components only fall, and the replay counts none
#   n_clamp_tie                         needs dn == -accN exactly: a cold joint between two bodies dealt velocity 0, which units_257 and
#                                       lanes_256_257 do not hold (the three other cases do, and require it)
DRESSED_COMMON = ("depth_lt1 depth_1_2 depth_gt2 disp_in_nonzero disp_in_negzero warm_normal warm_friction cold n_free n_clamp_strict "
                  "f_free f_clamp_pos f_clamp_neg f_limit_zero prod_dn prod_df prod_both prod_none i_subnormal i_skipped d_free d_clamped "
                  "d_productive d_unproductive d_skipped d_subnormal").split()
DRESSED_ITERS = [(6, 3), (3, 6)]          # ci != pi both ways, as in tests/test_path_edges_gpu.py
DRESSED_STATIC = ["static_body2", "static_moving"]
DRESSED_CASES = {
    ("lds", "units_256"): DRESSED_COMMON + ["n_clamp_tie"],
    ("lds", "units_257"): DRESSED_COMMON,
    ("tail", "tail_of_3"): DRESSED_COMMON + ["n_clamp_tie"],
    ("tail", "static_spokes"): DRESSED_COMMON + ["n_clamp_tie"] + DRESSED_STATIC,
    ("parts", "lanes_256_257"): DRESSED_COMMON,
}
# the fp16 form of the LDS cases: subnormal floats are zero as halves, and the one exact tie of units_256 does not survive the rounding
DRESSED_DROP16 = ("i_subnormal", "d_subnormal", "n_clamp_tie")


def dressed_labels(case, ci, pi, bits=32):
    want = required(DRESSED_CASES[case], ci, pi)
    return (want - set(DRESSED_DROP16)) | set(HALF_LABELS) if bits == 16 else want


def dressed_state(kind, name):
    import path_edges as pe
    state = {"lds": pe.lds_state, "tail": pe.tail_state, "parts": pe.parts_state}[kind](name)
    return dress(state, seed=len(name))


def dress(state, seed):
    """Re-value a units_state topology (bodies and joints keep their indices, contact points their ids): every body at the origin with
    unit-ish masses; per UNIT a contact of one of the classes below, per body a velocity class; a static body moves at (3, -2, 0.5)
    and carries a displacing velocity.  Values only: the graph, and with it the
    schedule and its designed class sizes, stays as it was.  -> a new (bodies, cps, joints)"""
    bodies, cps, joints = (a.copy() for a in state)
    rng = np.random.default_rng(seed)
    nb, ncp = len(bodies), len(cps)
    static = (bodies["inv_mass"] == 0) & (bodies["inv_inertia"] == 0)
    bodies["pos"]["x"] = bodies["pos"]["y"] = 0.0
    bodies["inv_mass"] = np.where(static, 0.0, rng.choice([0.5, 1.0, 2.0], nb))
    bodies["inv_inertia"] = np.where(static, 0.0, rng.choice([0.03125, 0.0625], nb))
    # velocities: most bodies slow, some at rest, some creeping at subnormal speed
    cls = rng.integers(0, 8, nb)
    for f in ("x", "y"):
        v = rng.uniform(-1.0, 1.0, nb)
        v = np.where(cls == 0, 0.0, np.where(cls == 1, rng.choice([SUB, -SUB, 3e-40, -TINY], nb), v))
        bodies["velocity"][f] = v
    bodies["angular_velocity"] = np.where(cls <= 1, 0.0, rng.uniform(-0.25, 0.25, nb))
    # displacing velocities: mostly +0; some nonzero, some -0.0, some subnormal
    dcl = rng.integers(0, 16, nb)
    for f, field in (("x", "displacing_velocity"), ("y", "displacing_velocity")):
        d = np.where(dcl == 0, rng.uniform(-0.25, 0.25, nb), np.where(dcl == 1, -0.0, np.where(dcl == 2, SUB, 0.0)))
        bodies[field][f] = d
    bodies["displacing_angular_velocity"] = np.where(dcl == 0, rng.uniform(-0.0625, 0.0625, nb), np.where(dcl == 1, -0.0, 0.0))
    # kinematic statics: the static bodies move
    for i in np.flatnonzero(static):
        bodies["velocity"]["x"][i], bodies["velocity"]["y"][i], bodies["angular_velocity"][i] = 3.0, -2.0, 0.5
        bodies["displacing_velocity"]["x"][i], bodies["displacing_velocity"]["y"][i], bodies["displacing_angular_velocity"][i] = 0.125, -0.25, 0.0625
    # contacts, per contact-point id: axis-aligned or random unit normals, small lever arms, depth classes shallow / 1..2 / deep
    ang = np.where(rng.random(ncp) < 0.5, rng.integers(0, 4, ncp) * (np.pi / 2), rng.uniform(0, 2 * np.pi, ncp))
    nx, ny = np.cos(ang).astype(F32), np.sin(ang).astype(F32)
    nx[np.abs(nx) < 1e-6] = 0.0
    ny[np.abs(ny) < 1e-6] = 0.0
    depth = rng.choice([0.5, 0.75, 1.0, 1.5, 2.0, 2.25, 2.5], ncp)
    rx, ry = rng.uniform(-0.5, 0.5, ncp), rng.uniform(-0.5, 0.5, ncp)
    cps["normal"]["x"], cps["normal"]["y"] = nx, ny
    cps["delta1"]["x"], cps["delta1"]["y"] = rx, ry
    cps["delta2"]["x"], cps["delta2"]["y"] = rx + depth * nx, ry + depth * ny
    # warm starts, per joint: cold / normal only / normal and friction inside the cone / friction of -0.0
    nj = len(joints)
    w = rng.integers(0, 4, nj)
    n_acc = np.where(w == 0, 0.0, rng.uniform(0.0, 0.5, nj))
    joints["normal_acc"] = n_acc
    joints["friction_acc"] = np.where(w == 2, rng.uniform(-0.25, 0.25, nj) * n_acc, np.where(w == 3, -0.0, 0.0))
    return bodies, cps, joints
