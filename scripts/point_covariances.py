"""Covariance of every free landmark point of a config in one vb_compute_point_covariances call
(csrc/pointcov.hip): wall time of the call, its phases, and the part after the selected inversion
(request upload, kernel, read-back) with the gather it implies.

    python scripts/point_covariances.py [config]      (default C)
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
from test_landmark_paths_gpu import panel_columns  # noqa: E402
from visual_inertial_bundle_adjustment_amd import synth  # noqa: E402
from visual_inertial_bundle_adjustment_amd.engine import HipEngine  # noqa: E402

which = sys.argv[1] if len(sys.argv) > 1 else "C"
p = synth.generate(synth.config(which))
g = HipEngine(imu_calib_options=p.imu_calib_options)
synth.load_into(g, p)
pts = np.flatnonzero(np.asarray(p.const[0]) == 0)
cols = panel_columns(p)[pts].astype(np.float64)
# Z entries the kernel reads: the diagonal tiles whole and the strict lower tiles, about half of n_p^2
gather = 0.5 * 8.0 * float(np.sum(cols * cols))
print(f"config {which}: {p.summary()}; {len(pts)} free points, panels of {int(cols.min())} to {int(cols.max())} columns "
      f"(mean {cols.mean():.0f}), about {gather / 1e9:.1f} GB of Z gathered", flush=True)
for rep in range(3):  # the first call pays the kernels' load
    g.synchronize()
    t = time.perf_counter()
    covs, used = g.compute_point_covariances(pts)
    dt = time.perf_counter() - t
    pro, inv, rest = g.point_covariance_times()
    print(f"call {rep}: {len(covs)} blocks in {dt:.3f} s wall (damping {used:g}); prologue {pro:.1f} ms, selected "
          f"inversion {inv:.1f} ms, after the selected inversion {rest:.1f} ms, conversion to matrices "
          f"{1e3 * dt - pro - inv - rest:.1f} ms; the gather at {gather / 1e6 / rest:.0f} GB/s", flush=True)
top = np.array([np.linalg.eigvalsh(0.5 * (c + c.T))[[0, -1]] for c in covs])
print(f"eigenvalues: smallest {top[:, 0].min():.3e}, largest {top[:, 1].max():.3e}; "
      f"{int(np.sum(top[:, 0] <= 0))} blocks not positive definite")
g.close()
