"""The scenes that more than one of the units' device tests use (tests/test_*_gpu.py): per kind the chain that its paths are tested on
and the mixed world that its life cycle runs in, built on the host.  Each returns (body rows for unit_lockstep.scene, lists): `lists`
one array per kind in the order of unit_spec.KINDS."""
import numpy as np

import angle_spec
import link_spec
import slider_spec
from unit_lockstep import O, X, Y, lists, pins as pin_rows, scene, worlds


# ---- pins ----
def chain(first_body, links, top, hang_from=-1, hang_anchor=None, spacing=10.0):
    """`links` boxes of 6 x 2 laid level with `top`, to its right, body numbers from first_body on; the first hangs from the world point
    `top` or from the point `hang_anchor` (its own frame) of body `hang_from`.  -> (body rows, pin rows).  The links are short of their
    joints (pins do not keep neighbours from colliding: only a sharp fold makes them touch)."""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(links)]
    pins = [(first_body, hang_from, (-h, 0.0), top if hang_from < 0 else hang_anchor)]
    pins += [(first_body + k, first_body + k - 1, (-h, 0.0), (h, 0.0)) for k in range(1, links)]
    return bodies, pins


def pin_mixed(links=12, extra_pair=True):
    """a chain from the world and, beside it, a pinned pair"""
    bodies, rows = chain(0, links, (0.0, 300.0))
    if extra_pair:
        bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-90.0, 300.0, 4.0, 1.5, False)]
        rows += [(links, links + 1, (5.0, 1.0), (-5.0, 0.0))]
    return bodies, lists(pins=pin_rows(rows))


# ---- links ----
def alternating_chain(units, top=(0.0, 500.0), spacing=10.0):
    """`units` boxes level with `top`; joints alternate pin / rod: a pin holds the neighbours' ends together, a rod of 2 joins points
    that lie 2 apart -> (body rows, pin rows, link rows)"""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(units)]
    pins, links = [(0, -1, (-h, 0.0), top)], []
    for k in range(1, units):
        if k % 2:
            links += [(k, k - 1, (-h + 1.0, 0.0), (h - 1.0, 0.0), 2.0, 2.0)]
        else:
            pins += [(k, k - 1, (-h, 0.0), (h, 0.0))]
    return bodies, pins, links


def link_mixed():
    """a 10-unit alternating chain, a pair on a spring, a body on a taut rope from the chain's body 4 and one on a slack rope"""
    bodies, rows, link_rows = alternating_chain(10, top=(0.0, 300.0))
    bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-85.0, 300.0, 4.0, 1.5, False)]
    link_rows += [(10, 11, (4.0, 0.0), (-4.0, 0.0), 5.0, 5.0, 2.0, 0.2)]
    bodies += [(45.0, 280.0, 2.0, 2.0, False), (200.0, 300.0, 2.0, 2.0, False)]
    link_rows += [(12, 4, (0.0, 2.0), (0.0, -1.0), 0.0, 10.0), (13, -1, (0.0, 0.0), (200.0, 320.0), 0.0, 60.0)]
    return bodies, lists(pins=pin_rows(rows), links=link_spec.make_links(link_rows))


# ---- angles ----
def limited_chain(count, top=(0.0, 500.0), spacing=10.0, limit=0.3):
    """`count` boxes level with `top`, pinned end to end from the world point `top`, every joint limited to +-limit
    -> (body rows, pins, angles): 2 count units in one component"""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(count)]
    pins = [(0, -1, (-h, 0.0), top)] + [(k, k - 1, (-h, 0.0), (h, 0.0)) for k in range(1, count)]
    angles = [(0, -1, -limit, limit)] + [(k, k - 1, -limit, limit) for k in range(1, count)]
    return bodies, pin_rows(pins), angle_spec.make_angles(angles)


def angle_mixed():
    """a limited chain of 10, a rod across it, a rope from its end, a welded pair (pin + lock) with a motor between the pair and a
    third body"""
    bodies, pins, angles = limited_chain(10, top=(0.0, 300.0), limit=0.2)
    links = link_spec.make_links([(4, 2, (0.0, 0.0), (0.0, 0.0), 20.0, 20.0), (9, -1, (5.0, 0.0), (100.0, 320.0), 0.0, 12.0)])
    bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-90.0, 300.0, 4.0, 1.5, False), (-80.0, 300.0, 2.0, 2.0, False)]
    pins = np.concatenate([pins, pin_rows([(10, 11, (5.0, 0.0), (-5.0, 0.0)), (12, 11, (-5.0, 0.0), (5.0, 0.0))])])
    angles = np.concatenate([angles, angle_spec.make_angles([(10, 11, 0.0, 0.0), (12, 11, -50.0, 50.0, 0.0, 0.0, 4.0, 0.05)])])
    return bodies, lists(pins=pins, links=links, angles=angles)


# ---- sliders: the four kinds ----
def mixed_chain(count, top=(0.0, 500.0), spacing=10.0):
    """`count` boxes level with `top`, joined end to end from the world point `top`, two units a joint, the four kinds in one component:
    joint k % 3 == 0 a pin and an angle limited to +-0.3, 1 a slider along the body before (limits +-1) and an angle lock (a telescope),
    2 a pin and a spring link between the centres"""
    h = spacing / 2.0
    bodies = [(top[0] + spacing * (k + 0.5), top[1], 3.0, 1.0, False) for k in range(count)]
    pins, links, angles, sliders = [], [], [], []
    for k in range(count):
        b, a2 = (k - 1, (h, 0.0)) if k else (-1, top)
        if k % 3 == 1:
            sliders.append((k, b, (-h, 0.0), a2, X, -1.0, 1.0))
            angles.append((k, b, 0.0, 0.0))
        else:
            pins.append((k, b, (-h, 0.0), a2))
            if k % 3 == 0:
                angles.append((k, b, -0.3, 0.3))
            else:
                links.append((k, b, O, O, spacing, spacing, 3.0, 0.5))
    return bodies, [pin_rows(pins), link_spec.make_links(links), angle_spec.make_angles(angles), slider_spec.make_sliders(sliders)]


def mixed():
    """a mixed chain of 12 and, beside it, a carriage on a world rail with a motor and a second carriage on the first, sprung"""
    bodies, (pins, links, angles, sliders) = mixed_chain(12, top=(0.0, 300.0))
    n = len(bodies)
    bodies += [(-100.0, 300.0, 4.0, 1.5, False), (-100.0, 310.0, 2.0, 2.0, False)]
    sliders = np.concatenate([sliders, slider_spec.make_sliders([(n, -1, O, (-100.0, 300.0), X, -20.0, 20.0, 0.0, 0.0, 4.0, 5.0e-4),
                                                                 (n + 1, n, O, (0.0, 10.0), Y, 0.0, 0.0, 2.0, 0.4)])])
    angles = np.concatenate([angles, angle_spec.make_angles([(n, -1, 0.0, 0.0)])])
    return bodies, [pins, links, angles, sliders]


MIXED = {"pin": pin_mixed, "link": link_mixed, "angle": angle_mixed, "slider": mixed}      # per kind the world of its life-cycle tests


def mixed_world(kind_name, **how):
    """the device world of MIXED[kind_name], before its first step"""
    bodies, units = MIXED[kind_name](**how)
    pw, _ = worlds(scene(bodies), units, with_oracle=False)
    return pw
