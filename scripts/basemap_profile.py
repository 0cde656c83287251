"""Device time of the base-map kernels at config C: the frozen scene of tests/basemap_scenes.py with 1% of the
rigs (100) as key rigs, three LM steps (linearize, damp / factor / solve, box-plus, comparable cost, restore).
Run it under `rocprofv3 --kernel-trace --stats` for the per-kernel times of basemap_lin_kernel,
basemap_sum_kernel and basemap_cost_kernel; alone it prints the factor counts."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import basemap_scenes as bs  # noqa: E402
from visual_inertial_bundle_adjustment_amd.engine import HipEngine  # noqa: E402


def main():
    which = sys.argv[1] if len(sys.argv) > 1 else "C"
    n_key = int(sys.argv[2]) if len(sys.argv) > 2 else 100
    p = bs.frozen_scene(which, n_key=n_key)
    e = bs.load(HipEngine, p)
    bm = p.basemap
    print(f"config {which}: {len(bm.T_bodyimu_world)} key rigs, {bm.num_factors} base-map factors on "
          f"{len(set(bm.point.tolist()))} points; {p.summary()}")
    for it in range(3):
        c0 = e.linearize(True, False)
        e.damp_factor_solve(1e-5)
        e.backup()
        e.apply_step(0)
        c1, stats = e.cost(True)
        e.restore()
        print(f"step {it}: cost {c0:.9g} -> {c1:.9g}, CostStats {stats}")
    e.close()


if __name__ == "__main__":
    main()
