"""The cost of the pin pass (include/phyx_amd.h PINS): a synchronised World::Update of one world of hanging chains, with and without
its pins, on the same build.

    python tools/pins_bench.py [--chains 4096] [--links 16] [--iterations 32] [--steps 200] [--warmup 60] [--repeats 5] [--no-pins] [--ropes] [--hinges] [--rails] [--breakable] [--only WORLD] [--import-from DIR]

The world: a ground and `chains` chains of `links` links (boxes of 2 x 8, 10 apart), each hung from a world pin, side by side.  The
pinned world runs under gravity (the pins carry the chains); the pinless twin has the same bodies and gravity 0, so that they stay
where they are and the rest of the step — broadphase, narrowphase, the empty contact solve — sees the same load.  Each repeat times
`steps` updates between two synchronisations with the host clock, the two worlds alternating; the result is one JSON line per world
with the median and every repeat.  --no-pins times the pinless world alone, and --import-from takes phyx_amd from another tree (a
build of the parent commit), which together give the parent's time for the same world.  The pass's own kernel time comes from a
kernel trace of `--steps N --repeats 1` (k_solve_pins in the statistics), in a run of its own.

--ropes adds a third world, "links" (include/phyx_amd.h LINKS): the pinned world plus one rope per chain from its last link to a world
point beside and below it, half a unit short, so that every rope is taut: 4096 more units in the same pass.  (`--links` was taken: it
is the chains' length.)  --only pins|pinless|links|angles|sliders runs that world alone, for a kernel trace in which k_solve_pins is one world's.

--hinges adds the world "angles" (include/phyx_amd.h ANGLES): the pinned world plus one limit per pin, [0, 0.6] rad on the angle of
each link against the one above it (the first: against the world).  A chain that hangs straight has theta = 0 = lower exactly, so
every limit is engaged on every step with C = 0 and goes through its whole arithmetic while the chains hang as still as in the
pinned world - as many angle units again as pins, in the same components.  (A lower limit above 0 bends every joint against
gravity and the chains writhe: 0.01 rad on the CPU spec at 32 sweeps.)

--rails adds the world "sliders" (include/phyx_amd.h SLIDERS): the pinned world plus one slider per link, its centre on a vertical world
rail through where it hangs, limited to [0, 5] along it.  A chain that hangs still has s = 0 = lower and t . e = 0 exactly, so on
every step row P and the lower stop are both engaged with C = 0 and go through their whole arithmetic while the chains hang as still
as in the pinned world - as many slider units again as pins, in the same components.

--breakable adds the world "breakable" (include/phyx_amd.h BREAKS): the pinned world with a finite break limit on every pin, 1000, far
above a chain's weight (the top pin of 16 links carries about 0.5), so that the break test runs behind every pass, its 4-byte count
comes down at every step and nothing ever breaks: the same pass on the same units, plus what a world with limits pays per step.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np


def build(phyx_amd, chains, links, pinned, spacing=10.0, ropes=False, hinges=False, rails=False, breakable=False):
    pw = phyx_amd.World(0, gravity=-200.0 if pinned else 0.0)
    pw.AddBody((0.0, 0.0), 0.0, (8.0 * chains + 100.0, 10.0), static=True)
    rows = np.zeros((chains * links, 5), dtype=np.float32)
    c, k = np.divmod(np.arange(chains * links), links)
    top = 40.0 + spacing * links
    rows[:, 0] = 8.0 * (c - chains / 2.0)
    rows[:, 1] = top - spacing * (k + 0.5)
    rows[:, 3], rows[:, 4] = 1.0, 4.0
    for r in rows:
        pw.AddBody((float(r[0]), float(r[1])), 0.0, (float(r[3]), float(r[4])))
    if pinned:
        from phyx_amd.api import pin_dtype
        pins = np.zeros(chains * links, dtype=pin_dtype)
        body = 1 + np.arange(chains * links)
        pins["body1"] = body
        pins["body2"] = np.where(k == 0, -1, body - 1)
        pins["anchor1"] = (0.0, spacing / 2.0)
        pins["anchor2"] = (0.0, -spacing / 2.0)
        heads = k == 0
        pins["anchor2"][heads, 0] = rows[heads, 0]
        pins["anchor2"][heads, 1] = top
        pw.add_pins(pins)
        if breakable:
            pw.set_break_limits("pin", np.arange(len(pins)), np.full(len(pins), 1000.0, dtype=np.float32))
    if ropes:
        from phyx_amd.api import link_dtype
        last = np.flatnonzero(k == links - 1)
        r = np.zeros(chains, dtype=link_dtype)
        r["body1"], r["body2"] = 1 + last, -1
        r["anchor1"] = (0.0, -spacing / 2.0)                     # the chain's free end, at (x, top - spacing * links) ...
        r["anchor2"][:, 0] = rows[last, 0] + 3.0
        r["anchor2"][:, 1] = top - spacing * links - 4.0         # ... 5 from this point, on a rope of 4.5
        r["max_length"] = 4.5
        pw.add_links(r)
    if hinges:
        from phyx_amd.api import angle_dtype
        body = 1 + np.arange(chains * links)
        h = np.zeros(chains * links, dtype=angle_dtype)
        h["body1"] = body
        h["body2"] = np.where(k == 0, -1, body - 1)
        h["lower"], h["upper"] = 0.0, 0.6
        pw.add_angles(h)
    if rails:
        from phyx_amd.api import slider_dtype
        r = np.zeros(chains * links, dtype=slider_dtype)
        r["body1"], r["body2"] = 1 + np.arange(chains * links), -1
        r["anchor2"][:, 0], r["anchor2"][:, 1] = rows[:, 0], rows[:, 1]
        r["axis"] = (0.0, 1.0)
        r["lower"], r["upper"] = 0.0, 5.0
        pw.add_sliders(r)
    return pw


def timed(pw, cfg, steps, dt=1.0 / 60.0):
    pw.sync()
    t0 = time.perf_counter()
    for _ in range(steps):
        pw.Update(dt, cfg)
    pw.sync()
    return (time.perf_counter() - t0) * 1e3 / steps


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--chains", type=int, default=4096)
    ap.add_argument("--links", type=int, default=16)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=60)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--iterations", type=int, default=32, help="pin sweeps per step (a hanging chain of 16 links is not stable at the default 8)")
    ap.add_argument("--no-pins", action="store_true")
    ap.add_argument("--ropes", action="store_true", help="also time the pinned world with one taut rope per chain (the 'links' world)")
    ap.add_argument("--hinges", action="store_true", help="also time the pinned world with one engaged limit per pin (the 'angles' world)")
    ap.add_argument("--rails", action="store_true", help="also time the pinned world with one engaged slider per link (the 'sliders' world)")
    ap.add_argument("--breakable", action="store_true", help="also time the pinned world with a break limit on every pin that none reaches (the 'breakable' world)")
    ap.add_argument("--only", choices=("pins", "pinless", "links", "angles", "sliders", "breakable"), default=None, help="run this world alone")
    ap.add_argument("--import-from", default=None)
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.import_from) if a.import_from else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import phyx_amd
    cfg = phyx_amd.Configuration(phyx_amd.SOLVE_AVX2, phyx_amd.ISLAND_MULTIPLE_SLOPPY, 15, 15)
    want = [a.only] if a.only else ([] if a.no_pins else ["pins"]) + ["pinless"] + (["links"] if a.ropes else []) + (["angles"] if a.hinges else []) + (["sliders"] if a.rails else []) + (["breakable"] if a.breakable else [])
    worlds = {name: build(phyx_amd, a.chains, a.links, name != "pinless", ropes=(name == "links"), hinges=(name == "angles"), rails=(name == "sliders"), breakable=(name == "breakable")) for name in want}
    for name, pw in worlds.items():
        if name != "pinless":
            pw.pin_iterations = a.iterations
    for pw in worlds.values():
        timed(pw, cfg, a.warmup)
    times = {name: [] for name in worlds}
    for _ in range(a.repeats):
        for name, pw in worlds.items():
            times[name].append(timed(pw, cfg, a.steps))
    for name, pw in worlds.items():
        out = {"world": name, "tree": os.path.dirname(os.path.abspath(phyx_amd.__file__)), "chains": a.chains, "links": a.links, "bodies": pw.counts()[0],
               "manifolds": pw.counts()[1], "steps": a.steps, "ms_per_step_median": round(statistics.median(times[name]), 4),
               "ms_per_step": [round(t, 4) for t in times[name]]}
        if name == "links":
            out.update(links=pw.link_count(), link_impulse_min=float(pw.links()["impulse"].min()), link_impulse_max=float(pw.links()["impulse"].max()))
        if name == "angles":
            imp = pw.angles()["impulse"]
            out.update(angles=pw.angle_count(), angle_impulse_max=float(np.abs(imp).max()))
        if name == "sliders":
            got = pw.sliders()
            out.update(sliders=pw.slider_count(), slider_impulse_max=float(np.abs(got["impulse"]).max()), slider_axis_impulse_max=float(np.abs(got["axis_impulse"]).max()))
        if name == "breakable":
            out.update(break_events=len(pw.break_events()), break_limit_max=float(pw.break_limits("pin").max()))
        if name != "pinless":
            s = pw.pin_schedule()
            out.update(pins=pw.pin_count(), lds_groups=s["lds_groups"], groups=len(s["group_offsets"]) - 1, classes=len(s["class_offsets"]) - 1,
                       iterations=pw.pin_iterations, schedule_builds=pw.pin_schedule_builds(), impulse_max=float(np.abs(pw.pins()["impulse"]).max()))
        print(json.dumps(out))


if __name__ == "__main__":
    main()
