"""The non-linearity inspection (vb_inspect_nonlinearities, csrc/inspect.hip + the expected-delta kernels of
csrc/visual.hip / csrc/small.hip) of a synthetic config after one linearization and solve: prints the reference's block of
the worst factors, and times it -- the wall time of one call, the device times of its x0 pass, x1 pass and
selection (vb_inspect_device_ms) and, beside them, the same build's vb_bench_kernel(10) (the visual
linearization: what the x0 pass evaluates, storing a 576 B record where the x0 pass stores 24 B) and
vb_bench_kernel(15) (the visual cost pass: what the x1 pass evaluates).

    python scripts/inspect_scale.py [config] [--k N] [--precision fp64|mixed]      (default C, k 5)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from visual_inertial_bundle_adjustment_amd import synth  # noqa: E402
from visual_inertial_bundle_adjustment_amd.engine import HipEngine  # noqa: E402
from visual_inertial_bundle_adjustment_amd.nonlinearity import format_nonlinearities  # noqa: E402

args = [a for a in sys.argv[1:] if not a.startswith("--")]
which = args[0] if args else "C"
k = int(sys.argv[sys.argv.index("--k") + 1]) if "--k" in sys.argv else 5
precision = sys.argv[sys.argv.index("--precision") + 1] if "--precision" in sys.argv else "fp64"
p = synth.generate(synth.config(which))
g = HipEngine(imu_calib_options=p.imu_calib_options, precision=precision)
synth.load_into(g, p)
print(f"config {which} ({precision}): {p.summary()}", flush=True)
g.linearize(True, False)
g.damp_factor_solve(1e-5)
r = g.inspect_nonlinearities(k=k)  # the first call pays the kernels' load and the inspection's setup
g.restore()
print(format_nonlinearities(r), end="")
print(f"{r['n_compared']} factors compared")

wall, ms = [], []
for _ in range(5):
    g.synchronize()
    t = time.perf_counter()
    g.inspect_nonlinearities(k=k)
    wall.append(1e3 * (time.perf_counter() - t))
    ms.append(g.inspect_device_ms())
    g.restore()
x0, x1, sel = (1e3 * float(np.median([m[i] for m in ms])) for i in range(3))
lin_us, cost_us = g.bench_kernel(10, 20), g.bench_kernel(15, 50)
print(f"inspect_nonlinearities(k={k}): {np.median(wall):.2f} ms wall (median of 5; {min(wall):.2f} to {max(wall):.2f})")
print(f"x0 pass (all kinds) {x0:.1f} us; visual linearization, vb_bench_kernel(10): {lin_us:.1f} us; ratio {x0 / lin_us:.2f}")
print(f"x1 pass (all kinds, score and keys) {x1:.1f} us; visual cost pass, vb_bench_kernel(15): {cost_us:.1f} us; "
      f"ratio {x1 / cost_us:.2f}")
print(f"selection {sel:.1f} us")
g.close()
