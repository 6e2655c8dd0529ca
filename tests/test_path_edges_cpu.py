"""The constructions of tests/path_edges.py checked with the host builder (phx_schedule_colours / phx_schedule_groups): every case has the
class sizes in leaders and followers, the part contents and the group shape it was designed for, so that a broken generator shows on
every CPU run and the GPU tests in tests/test_path_edges_gpu.py cannot pass vacuously."""
import numpy as np
import pytest

import phyx_amd
import path_edges as pe
from helpers import is_static


def _host_colours(state):
    bodies, _, joints = state
    return phyx_amd.schedule_colours(joints["body1"], joints["body2"], is_static(bodies), joints["contact_point_index"])


@pytest.mark.parametrize("name", list(pe.TAIL_CASES))
def test_tail_constructions_have_the_designed_classes(name):
    """k_solve_tail's cases: leaders and followers per class exactly as designed, and the trailing run tail_first_class picks."""
    leaders, followers, on_static, tail = pe.TAIL_CASES[name]
    state = pe.tail_state(name)
    order, offs = _host_colours(state)
    L, F = pe.class_counts(order, offs, state[2])
    assert L.tolist() == leaders and F.tolist() == followers
    assert pe.tail_first_class(leaders) == tail
    n = len(leaders) - tail
    assert n == 0 or 2 <= n <= pe.TAIL_CLASSES_MAX
    if name == "exact_1024_behind_1025":
        assert leaders[tail - 1] == pe.TAIL_T + 1 and set(leaders[tail:]) == {pe.TAIL_T}
    if name == "over_64_trailing":
        assert len(leaders) > pe.TAIL_CLASSES_MAX + 1 and n == pe.TAIL_CLASSES_MAX and max(leaders[1:]) <= pe.TAIL_T
    if on_static is not None:       # every tail class holds units on the static body 0
        j = state[2]
        on0 = (j["body1"][order] == 0) | (j["body2"][order] == 0)
        assert all(on0[offs[c]:offs[c + 1]].sum() > 0 for c in range(tail, len(leaders)))


def test_shallow_contacts_stop_the_displacement_sweeps_early(oracle):
    """The tail case with displacement_iterations < pi: the oracle's replay of the host schedule leaves the displacement sweeps early."""
    state = pe.tail_state("tail_of_3", shallow=True)
    order, offs = _host_colours(state)
    b, cp, j = (a.copy() for a in state)
    st = oracle.solver_solve_grouped(b, cp, j, order, offs, np.array([0, len(j)]), 3, 6, oracle.STAG_COLOUR_SYNC)
    assert st.impulse_iterations == 3 and 1 < st.displacement_iterations < 6


def test_grid_construction_has_classes_past_one_grid_pass():
    """k_solve_colour's grid stops at 8192 x 64 = 524 288 lanes (grid_for's 2048 x 256 is the same count): one class of exactly that many
    leaders and one of one more, every leader with a follower."""
    state = pe.grid_state()
    order, offs = _host_colours(state)
    L, F = pe.class_counts(order, offs, state[2])
    assert L.tolist() == [pe.GRID_ITEMS + 1, pe.GRID_ITEMS] and F.tolist() == L.tolist()
    assert pe.GRID_ITEMS == 2048 * 256


def _parts_content(state, order, offs):
    """per interior class (level-0 classes first): {part: units} — level from the restated unit_part"""
    bodies, _, joints = state
    nb = len(bodies)
    lead = (joints["contact_point_index"][order] & 1) == 0
    out = []
    for c in range(len(offs) - 1):
        s = order[offs[c]:offs[c + 1]][lead[offs[c]:offs[c + 1]]]
        parts = [pe.unit_part(int(a), int(b), nb) for a, b in zip(joints["body1"][s], joints["body2"][s])]
        out.append(dict(zip(*np.unique(parts, return_counts=True))))
    return out


@pytest.mark.parametrize("name", list(pe.PARTS_CASES))
def test_parts_constructions_have_the_designed_parts(name):
    """The partitioned-component cases: one component of more than 1024 joints, every unit interior; level-0 classes of 256 units in a
    full part, the level-1 parts of the designed size; > 64 interior classes; CP_MAXU units in part 0."""
    nb, sizes, star0, dense0 = pe.PARTS_CASES[name]
    state = pe.parts_state(name)
    bodies, _, joints = state
    assert len(joints) > pe.COLOUR_B_MAX_JOINTS
    _, size = phyx_amd.schedule_islands(joints["body1"], joints["body2"], is_static(bodies))
    assert len(size) == 1                                                       # one component: partitioned
    order, offs = _host_colours(state)
    content = _parts_content(state, order, offs)
    P = (nb + pe.PART_BODIES - 1) // pe.PART_BODIES
    assert all(-1 not in c for c in content)                                    # every unit interior
    lvl = [0 if all(p < P for p in c) else 1 for c in content]
    assert all(all((p < P) == (l == 0) for p in c) for c, l in zip(content, lvl))  # a class holds one level's units
    assert lvl == sorted(lvl)                                                   # level 0's classes first
    per_part = {}
    for c in content:
        for p, n in c.items():
            per_part[p] = per_part.get(p, 0) + n
    assert P not in per_part                                                    # the first level-1 part is empty (test below)
    for k, s in enumerate(sizes):                                               # level-1 part P + k + 1: the designed classes
        got = [c.get(P + k + 1, 0) for c, l in zip(content, lvl) if l == 1]
        assert got[:len(s)] == s and not any(got[len(s):])
    if name == "lanes_256_257":
        assert nb % pe.PART_BODIES != 0 and per_part[P - 1] == nb % pe.PART_BODIES - 1     # the partial last part has interior units
        assert [content[0][p] for p in range(P - 1)] == [pe.PARTS_T] * (P - 1)         # a full part's class 0: 256 units, every lane
        assert sum(sizes[0]) == pe.PARTS_T                                              # every unit of the part owned by a lane
        assert sizes[1][0] < pe.PARTS_T < sizes[1][0] + sizes[1][1] == pe.PARTS_T + 1      # the 257th unit in the middle of class 1 ...
        assert len(sizes[1]) == 3 and sizes[1][2] > 0                                     # ... and a class whose `before` passes PARTS_T
        assert sum(l == 0 for l in lvl) <= pe.PARTS_CLASS_STRIDE and len(content) <= pe.PARTS_CLASS_STRIDE
    if name == "over_64_interior_classes":
        assert sum(l == 0 for l in lvl) > pe.PARTS_CLASS_STRIDE
    if dense0:
        assert per_part[0] == dense0 and sum(l == 0 for l in lvl) <= pe.PARTS_CLASS_STRIDE


def test_the_first_level1_part_can_hold_no_interior_unit():
    """k_solve_parts' first level-1 part starts at body -256 (csrc/schedule.h part_first_body) — but no unit can be interior to it: its
    bodies in range are [0, 256), all inside level-0 part 0, and unit_part gives level 0 precedence.  The negative base is reached only by
    the part's body loads and stores (the GPU cases sweep a component that covers it); no case can put a unit there."""
    for nb in (256, 300, 512, 1836):
        P = (nb + pe.PART_BODIES - 1) // pe.PART_BODIES
        a, b = np.meshgrid(np.arange(min(nb, 300)), np.arange(min(nb, 300)))
        parts = {pe.unit_part(int(x), int(y), nb) for x, y in zip(a.ravel(), b.ravel()) if x != y}
        assert P not in parts


@pytest.mark.parametrize("name", list(pe.LDS_CASES))
def test_lds_constructions_have_the_designed_shape(name):
    """The LDS group cases: the host builder bins the path component into the small shape (ISL_T = 256 lanes), the big one (ISL_T_BIG =
    512) or the HBM group exactly as designed."""
    units, two, shape = pe.LDS_CASES[name]
    bodies, _, joints = pe.lds_state(name)
    st = is_static(bodies)
    args = (joints["body1"], joints["body2"], st, joints["contact_point_index"])
    small = phyx_amd.schedule_groups(*args, lanes=pe.ISL_T, body_cap=pe.ISL_B)
    big = phyx_amd.schedule_groups(*args, lanes=pe.ISL_T_BIG, body_cap=pe.ISL_B_BIG)
    path_joints = units + two
    in_small = small["group_offsets"][small["lds_groups"]] == len(joints)
    in_big = big["group_offsets"][big["lds_groups"]] == len(joints)
    assert (shape, in_small, in_big) in {("small", True, True), ("big", False, True), ("hbm", False, False)}
    want = "hbm" if units > pe.ISL_T_BIG or path_joints > 2 * pe.ISL_T_BIG else "big" if units > pe.ISL_T or path_joints > 2 * pe.ISL_T else "small"
    assert want == shape


def test_the_lds_body_caps_cannot_bind():
    """ISL_B = 768 and ISL_B_BIG = 1024 (csrc/island_view.h) cannot bind: a component's bodies are at most its units + 1 (it is connected
    through its dynamic bodies; a static body adds at most one body per unit), and a bin never spans a multiple of BIN_CHUNK = 64
    component numbers, so a bin holds at most lanes + 64 bodies: 320 < 768 in the small shape, 576 < 1024 in the big one.  The densest
    bin there is — one-unit islands of two bodies each and a 257-unit path that selects the big shape — stays below both caps."""
    assert pe.ISL_T + pe.BIN_CHUNK < pe.ISL_B and pe.ISL_T_BIG + pe.BIN_CHUNK < pe.ISL_B_BIG
    a = np.arange(257)
    pairs = 258 + 2 * np.arange(2000)
    rows = np.concatenate([np.stack([a, a + 1, np.zeros_like(a)], axis=1), np.stack([pairs, pairs + 1, np.zeros_like(pairs)], axis=1)])
    bodies, _, joints = pe.units_state(9, 258 + 4000, rows)
    for lanes, cap in ((pe.ISL_T, pe.ISL_B), (pe.ISL_T_BIG, pe.ISL_B_BIG)):
        g = phyx_amd.schedule_groups(joints["body1"], joints["body2"], is_static(bodies), joints["contact_point_index"], lanes=lanes, body_cap=cap)
        go = g["group_offsets"]
        most = max(len(np.unique(np.concatenate([joints["body1"][g["order"][go[k]:go[k + 1]]], joints["body2"][g["order"][go[k]:go[k + 1]]]])))
                   for k in range(g["lds_groups"]))
        assert most <= lanes + pe.BIN_CHUNK < cap
