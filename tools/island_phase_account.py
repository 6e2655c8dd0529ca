"""The island kernel's launch, accounted for: every phase stamp of the TRACE instantiation (phx_solver_set_trace; island_view.h
ISL_PHASE_WORDS) for the cfg-2 solve as one table that sums to the span of the launch, the real shader clock during the launch, and
where a working wave's class step goes.  Prints markdown (profiles/island_phase_account.md is this tool's output plus the rocprofv3
launch time of the same session).  usage: island_phase_account.py [columns=1000] [rows=200] [iters=20]"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import phyx_amd
from phyx_amd import scenes, Configuration

cols = int(sys.argv[1]) if len(sys.argv) > 1 else 1000
rows = int(sys.argv[2]) if len(sys.argv) > 2 else 200
iters = int(sys.argv[3]) if len(sys.argv) > 3 else 20
w = phyx_amd.World(0, gravity=-200.0); w.add_scene(scenes.stack(cols, rows))
cfg = Configuration(2, 2, iters, iters)
for _ in range(3): w.Update(1 / 60, cfg)
w.PreSolve(1 / 60)
s = phyx_amd.Solver(0)
db, dc, dj = (phyx_amd.DeviceArray(a) for a in (w.bodies, w.contactPoints, w.contactJoints))
r = s.bench(db, dc, dj, cfg, 3, 20)
plain_us = 1e3 * r.impulse_kernel_ms / max(r.bracketed_launches, 1)
s.set_trace(True, waves=False)
r = s.bench(db, dc, dj, cfg, 2, 5)
traced_us = 1e3 * r.impulse_kernel_ms / max(r.bracketed_launches, 1)
t = s.island_trace().astype(np.int64)
p = s.phase_trace().astype(np.int64)
ran = t[:, 0] != 0
t, p = t[ran], p[ran]
TICK = 100.0                                           # stamps: the constant 100 MHz clock
# the stamps in the order the kernel passes them
order = [("workgroup started (dispatch ramp)", t[:, 0]), ("set-up level 1 back (descriptor, unit record, body ids)", p[:, 0]),
         ("set-up level 2 back (bodies, joints, contact points)", p[:, 1]), ("records in LDS, compared", p[:, 2]),
         ("barrier + arrival issued", t[:, 1]), ("Refresh computed", p[:, 3]), ("barrier + tag table zeroed + barrier", t[:, 2]),
         ("PreStep class 0", p[:, 4]), ("PreStep class 1", p[:, 5]), ("PreStep class 2", p[:, 6]), ("PreStep class 3", p[:, 7]),
         ("arrival forwarded (pre-stepped)", t[:, 3]), ("first sweep (both halves unless quiet)", p[:, 8]), ("remaining sweeps", t[:, 4]),
         ("commit decided (wait + barrier)", p[:, 9]), ("results and counters issued", p[:, 10]), ("stores have left (vmcnt(0))", t[:, 5])]
t0 = t[:, 0].min()
at = np.zeros((len(t), len(order)))
prev = np.full(len(t), t0, dtype=np.int64)
for k, (_, col) in enumerate(order):
    cur = np.where(col == 0, prev, col)               # (a group with fewer than four classes leaves the later PreStep stamps out)
    at[:, k] = (cur - prev) / TICK
    prev = cur
end = (t[:, 5] - t0) / TICK
span = end.max()
slow = int(np.argmax(end))
med = int(np.argsort(end)[len(end) // 2])
ticks = t[:, 6] >> 4
mhz = ticks / ((t[:, 5] - t[:, 0]) / TICK)
print("# Island kernel: phase account (cfg 2, %d x %d, %d sweeps, %d workgroups)\n" % (cols, rows, iters, len(t)))
print("Launch by HIP events: %.2f us untraced (the product kernel), %.2f us traced (phase stamps only): THE STAMPED BUILD IS SLOWER, every duration"
      " below is the stamped build's.  First workgroup start -> last store left: %.2f us.\n" % (plain_us, traced_us, span))
print("Shader clock during the launch (s_memtime ticks / s_memrealtime ticks x 100 MHz, per workgroup): median %.0f MHz, min %.0f, max %.0f.\n" % (np.median(mhz), mhz.min(), mhz.max()))
print("| phase (time since the previous stamp, us) | median over groups | p95 | max | median-end group | slowest group |")
print("|---|---|---|---|---|---|")
for k, (name, _) in enumerate(order):
    print("| %s | %.2f | %.2f | %.2f | %.2f | %.2f |" % (name, np.median(at[:, k]), np.percentile(at[:, k], 95), at[:, k].max(), at[med, k], at[slow, k]))
print("| **sum** (= the group's last stamp since the launch's first) | %.2f | | | %.2f | %.2f |" % (np.median(at, axis=0).sum(), at[med].sum(), at[slow].sum()))
print("\nThe slowest group's column sums to the span, %.2f us; the same (traced) launch by HIP events is %.2f us: residual %.2f us (events bracket the"
      " dispatch and the kernel's end).  The product kernel's launch is %.2f us: the stamps cost %.2f us.\n" % (span, traced_us, traced_us - span, plain_us, traced_us - plain_us))
ncol = t[:, 7] >> 32; sw = t[:, 7] & 0xffffffff
steps = ncol * np.maximum(sw - 1, 1)
per = (t[:, 4] - np.where(p[:, 8] == 0, t[:, 3], p[:, 8])) / TICK / steps
print("Classes per group: median %d; sweeps executed: max %d.  A class step of the remaining sweeps: median %.3f us = %.0f cycles at the measured clock.\n"
      % (np.median(ncol), sw.max(), np.median(per), np.median(per) * np.median(mhz)))

s.set_trace(True, waves=True)                          # once more with the per-wave counts: where a working wave's step goes
s.bench(db, dc, dj, cfg, 1, 2)
p = s.phase_trace()[ran]
rowsw = p[:, 16:16 + 8 * 8].reshape(len(p), 8, 8).astype(np.float64)
n = (p[:, 16:16 + 64].reshape(len(p), 8, 8)[:, :, 5] & np.uint64(0xffffffff)).astype(np.float64)
names = ["barrier released -> LDS data back", "-> last FMA", "-> stores issued", "-> lgkmcnt(0)", "-> barrier released"]
print("## Inside one class step of the working wave (impulse-only sweeps, shader cycles, median over waves of the per-wave mean; only steps in"
      " which the wave's first lane was evaluated; the traced step carries five s_memtime reads and one extra lgkmcnt(0))\n")
print("| interval | plain wave | wave that touches the ground |")
print("|---|---|---|")
tot = [0.0, 0.0]
for k in range(5):
    cell = []
    for g in (0, 1):
        m = (n > 0) & (rowsw[:, :, 6] == g)
        v = np.median(rowsw[:, :, k][m] / n[m]) if m.any() else float("nan")
        tot[g] += v; cell.append(v)
    print("| %s | %.0f | %.0f |" % (names[k], cell[0], cell[1]))
print("| **sum** | %.0f | %.0f |" % (tot[0], tot[1]))
print("\nSteps counted (the wave's first lane has a unit of the class and the skip test let it through): %d." % n.sum())
