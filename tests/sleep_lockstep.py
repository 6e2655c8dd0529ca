"""The harness of the sleeping device tests (tests/test_sleep_gpu.py): twins.  World A has sleeping on; world B has it off, and after
every step the test computes sleep_spec on B's state and applies its decisions to B with set_inverse_masses / set_velocities — which is
what the contract says A is.  After every step every byte of the two states and A's sleep states against the spec's are compared."""
import numpy as np

import phyx_amd
import sleep_spec
from unit_lockstep import DT, G, KINDS, NAMES, cfg, lists_of


class Twins:
    def __init__(self, scene, params, mode=phyx_amd.ISLAND_MULTIPLE_SLOPPY, lists=None, gravity=G, prepare=None):
        self.a, self.b = phyx_amd.World(0, gravity=gravity), phyx_amd.World(0, gravity=gravity)
        for w in (self.a, self.b):
            w.add_scene(scene)
            for kind, units in zip(KINDS, lists or ()):
                getattr(w, kind.add)(units)
            if prepare:
                prepare(w)
        self.a.set_sleeping(*params)
        self.params = sleep_spec.Params(*params)
        self.state = sleep_spec.new_state(len(scene["px"]))
        self.cfg = cfg(mode)
        self.units = lists is not None
        self.flags = False
        self.slept, self.woken = [], []      # per step, the spec's decisions

    # ---- the spec's side ----
    def unit_pairs(self):
        return sleep_spec.unit_pairs(lists_of(self.b) if self.units else None)

    def graph(self):
        return self.b.manifolds, self.unit_pairs(), (self.b.body_flags() if self.flags else None)

    def put_to_sleep(self, slept):
        if slept:
            self.b.set_inverse_masses(slept, np.zeros((len(slept), 2), dtype=np.float32))
            self.b.set_velocities(slept, np.zeros((len(slept), 3), dtype=np.float32))

    def restore(self, woken):
        if woken:
            self.b.set_inverse_masses(woken, np.stack([self.state["inv_mass"][woken], self.state["inv_inertia"][woken]], axis=1))

    def wake_on_b(self, named):
        """what a call that names `named` does first: their sleeping components wake -> the woken bodies"""
        manifolds, units, flags = self.graph()
        woken = sleep_spec.wake_components(self.state, named, manifolds, units, flags)
        self.restore(woken)
        return woken

    def wake_everything_on_b(self):
        woken = np.flatnonzero(self.state["asleep"]).tolist()
        self.state["asleep"][woken] = 0; self.state["timer"][woken] = 0
        self.restore(woken)
        return woken

    # ---- the step ----
    def step(self, s, dt=DT):
        units = self.unit_pairs()      # the lists as this step's pin pass solves them: a unit that breaks in this step is still an edge in it
        self.a.Update(dt, self.cfg)
        self.b.Update(dt, self.cfg)
        bodies = self.b.bodies
        manifolds, flags = self.b.manifolds, (self.b.body_flags() if self.flags else None)
        slept, woken = sleep_spec.decide(self.state, bodies["inv_mass"], bodies["inv_inertia"], bodies["velocity"]["x"], bodies["velocity"]["y"],
                                         bodies["angular_velocity"], manifolds, units, flags, self.params, dt)
        self.put_to_sleep(slept)
        self.restore(woken)
        self.slept.append(slept); self.woken.append(woken)
        self.same("at step %d" % s)

    def same(self, what):
        assert self.a.counts() == self.b.counts(), "counts differ %s" % what
        for name, x, y in zip(NAMES, self.a.state(), self.b.state()):
            assert x.tobytes() == y.tobytes(), "%s differ %s" % (name, what)
        if self.units:
            for kind, x, y in zip(KINDS, lists_of(self.a), lists_of(self.b)):
                assert x.tobytes() == y.tobytes(), "%s differ %s" % (kind.plural, what)
        self.same_states(what)

    def same_schedules(self, what):
        """the pin pass's schedule of the next step, the static set (the sleepers) part of it"""
        x, y = self.a.pin_schedule(), self.b.pin_schedule()
        assert sorted(x) == sorted(y)
        for key in x:
            assert np.array_equal(x[key], y[key]), "the pin schedules' %s differ %s" % (key, what)

    def same_states(self, what):
        b = self.b.bodies
        want = sleep_spec.shown(self.state, b["inv_mass"], b["inv_inertia"])
        got = self.a.sleep_states()
        assert got.dtype == want.dtype
        if got.tobytes() != want.tobytes():
            bad = np.flatnonzero([g.tobytes() != w.tobytes() for g, w in zip(got, want)])
            raise AssertionError("sleep states differ %s: bodies %s, device %s, spec %s" % (what, bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist()))
        asleep = int(self.state["asleep"].sum())
        assert self.a.sleep_counts()[0] == asleep, "asleep count %s" % what

    def asleep(self):
        return np.flatnonzero(self.state["asleep"]).tolist()
