"""Random search for the narrowphase trace's labels (oracle/phx_oracle.h PHXO_T_*): how many of N random box pairs, each walked
through three phases (a pose, a small move of it, another), reach every label through the traced per-pair entry
(oracle.binding.trace_pairs).  CPU only.  It settles which labels tests/narrowphase_corpus.py may leave off REQUIRED.

usage: narrowphase_search.py [pairs [seed]]      (default 2 000 000 pairs, seed 1)"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from oracle import binding as ob

SIZES = np.array([0.0, 0.25, 0.5, np.nextafter(np.float32(1), np.float32(0)), 1.0, 1.5, 2.0, 3.0, 5.0, 8.0, 12.0], dtype=np.float32)
ANGLES = np.array([0.0, 0.05, 0.0995, 0.1002, 0.1005, 0.3, 0.7854, 1.4706, 1.5708, 3.1416, -1.5708, -0.1002], dtype=np.float32)


def frames(angle):
    """xVector, yVector as RigidBody's constructor makes them (ref: Coords2.h:10-17, with pi = 3.141592f)."""
    a = angle.astype(np.float32)
    q = (a + np.float32(3.141592) / np.float32(2.0)).astype(np.float32)
    return (np.cos(a.astype(np.float64)).astype(np.float32), np.sin(a.astype(np.float64)).astype(np.float32),
            np.cos(q.astype(np.float64)).astype(np.float32), np.sin(q.astype(np.float64)).astype(np.float32))


def bodies_of(px, py, angle, sx, sy):
    b = np.zeros(len(px), dtype=ob.body_dtype)
    b["pos"]["x"], b["pos"]["y"] = px, py
    b["xv"]["x"], b["xv"]["y"], b["yv"]["x"], b["yv"]["y"] = frames(angle)
    b["geom_size"]["x"], b["geom_size"]["y"] = sx, sy
    return b


def draw(rng, n):
    """2n bodies: pair k is bodies 2k, 2k + 1, the second placed so that the two touch, overlap or just miss."""
    pick = lambda: np.where(rng.random(2 * n) < 0.5, rng.choice(SIZES, 2 * n), rng.uniform(0, 12, 2 * n)).astype(np.float32)
    sx, sy = pick(), pick()
    ang = np.where(rng.random(2 * n) < 0.6, rng.choice(ANGLES, 2 * n) + rng.choice([0.0, 1.5707963, 3.1415927, -1.5707963], 2 * n),
                   rng.uniform(-3.2, 3.2, 2 * n)).astype(np.float32)
    px = rng.uniform(-20, 20, 2 * n).astype(np.float32)
    py = rng.uniform(-20, 20, 2 * n).astype(np.float32)
    # the second body of each pair: beside or above the first, at about the sum of the half-extents, give or take
    side = rng.random(n) < 0.5
    reach_x, reach_y = sx[0::2] + sx[1::2], sy[0::2] + sy[1::2]
    slack = np.where(rng.random(n) < 0.3, 0.0, rng.normal(0, 0.6, n))
    along = rng.uniform(-1.1, 1.1, n)
    sign = rng.choice([-1.0, 1.0], n)
    px[1::2] = px[0::2] + np.where(side, sign * (reach_x + slack), along * reach_x)
    py[1::2] = py[0::2] + np.where(side, along * reach_y, sign * (reach_y + slack))
    return px.astype(np.float32), py.astype(np.float32), ang, sx, sy


def search(n, seed, chunk=200000):
    rng = np.random.default_rng(seed)
    names = ob.trace_labels()
    total = np.zeros(len(names), dtype=np.int64)
    overflows = 0
    for start in range(0, n, chunk):
        k = min(chunk, n - start)
        px, py, ang, sx, sy = draw(rng, k)
        pts = np.zeros(2 * k, dtype=ob.contact_point_dtype)
        pts["solver_index"] = -1
        cnt = np.zeros(k, dtype=np.int32)
        reached = np.zeros((k, 2), dtype=np.uint64)
        for phase in range(3):
            if phase:
                # move one body or both: nothing, along x or y by about 2, a small turn
                kind = rng.integers(0, 6, 2 * k)
                step = rng.choice([0.5, 1.9, 2.0, 2.1, 3.0, -2.0, -2.1, 6.0], 2 * k)
                px = (px + np.where(kind == 1, step, 0.0)).astype(np.float32)
                py = (py + np.where(kind == 2, step, 0.0)).astype(np.float32)
                ang = (ang + np.where(kind == 3, rng.choice([0.01, -0.01, 0.1, 1.5707963], 2 * k), 0.0)).astype(np.float32)
                both = rng.random(k) < 0.5                         # half of the pairs move as one: the second body follows the first
                dx, dy = px[0::2] - px0[0::2], py[0::2] - py0[0::2]
                px[1::2] = np.where(both, px0[1::2] + dx, px[1::2]); py[1::2] = np.where(both, py0[1::2] + dy, py[1::2])
            px0, py0 = px.copy(), py.copy()
            pts, cnt, masks, over = ob.trace_pairs(bodies_of(px, py, ang, sx, sy), pts, cnt)
            overflows += over
            reached |= masks
        for i in range(len(names)):
            total[i] += int(np.count_nonzero(reached[:, i >> 6] >> np.uint64(i & 63) & np.uint64(1)))
    return dict(zip(names, total.tolist())), overflows


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000000
    seed = int(sys.argv[2]) if len(sys.argv) > 2 else 1
    counts, overflows = search(n, seed)
    for name, c in counts.items():
        print("%-24s %9d" % (name, c))
    print("pairs %d, seed %d, overflows %d; never reached: %s" % (n, seed, overflows, [k for k, c in counts.items() if c == 0]))
