"""The calibration evaluation against factory (calib_eval.compare_calibration_vs_factory: the projection offsets
of EvalCalibration.cpp:57-116 through vb_calib_projection_offsets), printed and timed.

    python scripts/calib_eval.py [--host-only] [--rigs N] [--host-every K]

1. The adapter problem of the golden session (tests/golden/session_small): the report text, then the device
   time of the kernels (vb_calib_eval_device_ms), the wall time of the call, and the host library's time
   (libviba_host, vbh_calib_projection_offsets) on the same pair list.
2. A synthetic pair list of config-C size: N rigs (default 10000, at 10 Hz: 5 s calibration windows of 50 rigs)
   x 4 cameras (three 640 x 480 Fisheye624 and the golden session's 1408 x 1408 one), every window's variables
   perturbed beside the factory values.  The device gets one pair per (camera, window) with the window's rig
   count as its weight; the host library gets every (rig, camera) entry as a pair of weight 1, the way the
   reference walks rigCamToModelIndex (--host-every K: only every K-th rig, to shorten the run; the time is
   then printed as measured, with the fraction).  The two results are compared where they cover the same
   entries.
--host-only skips everything that needs a GPU (the host timing of part 2 alone).
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import calib_eval_scenes as CS  # noqa: E402
from visual_inertial_bundle_adjustment_amd import calib_eval as CE  # noqa: E402
from visual_inertial_bundle_adjustment_amd import kinds as K  # noqa: E402


def opt(name, default):
    return type(default)(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


host_only = "--host-only" in sys.argv
n_rigs, host_every = opt("--rigs", 10000), opt("--host-every", 1)
GOLDEN = os.path.join(ROOT, "tests", "golden", "session_small")


def timed(fn, repeat=1):
    best, out = None, None
    for _ in range(repeat):
        t = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t
        best = dt if best is None else min(best, dt)
    return out, best


def worst(a, b):
    has = a["count"] > 0
    assert np.array_equal(a["count"], b["count"])
    return max(float(np.max(np.abs(a[k][has] - b[k][has]) / CS.eps(b[k][has]))) for k in ("mean", "rmse", "p50", "p90"))


# ------------------------------------------------------------------ 1. the golden session
if not host_only:
    from visual_inertial_bundle_adjustment_amd import adapter, session
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    sd = session.SessionData.load(GOLDEN)
    m = session.Matcher.build(sd)
    p = adapter.build_problem(sd, m)
    e = adapter.load_into(HipEngine(reproj_loss=p.reproj_loss, imu_loss=p.imu_loss,
                                    imu_calib_options=p.imu_calib_options), p)
    print(f"golden session: {p.summary()}", flush=True)
    print(CE.show_calibration_comp_results(CE.compare_calibration_vs_factory(e, p, sd, m)))
    fcal = sd.factory_calib
    fcam = np.array([fcal.cameras[m.slam_cam_to_factory[c]].camera_data(False, False) for c in range(p.n_cam)])
    fT = np.array([fcal.T_cam_bodyimu[m.slam_cam_to_factory[c]] for c in range(p.n_cam)])
    iv, ev, cam, w = CE.camera_pairs(p)
    args = (fcam, fT, iv, ev, cam, w, cam, p.n_cam, CE.DISTANCES)
    dev, wall = timed(lambda: e.calib_projection_offsets(*args), 5)
    host, host_s = timed(lambda: CE.host_projection_offsets(e.get_vars(K.VAR_CAM_INTR), e.get_vars(K.VAR_CAM_EXTR), *args))
    print(f"golden session, {len(iv)} pairs for {int(w.sum())} (rig, camera) entries: device kernels "
          f"{e.calib_eval_device_ms():.3f} ms, call {1e3 * wall:.2f} ms wall (best of 5); host library on the pairs "
          f"{1e3 * host_s:.1f} ms; worst statistic difference {worst(dev, host):.2e} of the bound", flush=True)
    e.close()

# ------------------------------------------------------------------ 2. config-C size
per_window = 50
n_win = (n_rigs + per_window - 1) // per_window
golden_cam, golden_T = CS.golden_camera()
fac = CS.factory_cameras()
fcam = np.array([CS.fisheye(240.0 + 5 * c, 318.7 - c, 241.3 + c, 640, 480) for c in range(3)] + [golden_cam])
fT = np.array([fac["f120"][1], fac["linear"][1], fac["small"][1], golden_T])
intr, extr, cam, weight = [], [], [], []
for c in range(4):
    for wdw in range(n_win):
        ci, Tv = CS.perturbed(fcam[c], fT[c], 1000 * c + wdw)
        intr.append(ci), extr.append(Tv), cam.append(c)
        weight.append(min(per_window, n_rigs - wdw * per_window))
intr, extr = np.array(intr), np.array(extr)
cam, weight = np.array(cam, np.int32), np.array(weight, np.int64)
var = np.arange(len(cam), dtype=np.int32)
print(f"config-C size: {n_rigs} rigs x 4 cameras = {int(weight.sum())} entries in {len(var)} distinct pairs "
      f"(grids {[CE.grid_shape(c[2], c[3]) for c in fcam]})", flush=True)

# every (rig, camera) entry as its own pair, the reference's walk (optionally every host_every-th rig)
rigs = np.arange(0, n_rigs, host_every)
entry_var = np.concatenate([c * n_win + rigs // per_window for c in range(4)]).astype(np.int32)
entry_cam = np.repeat(np.arange(4, dtype=np.int32), len(rigs))
host, host_s = None, 0.0
for c in range(4):   # one call per camera (a series is one camera's), so that the run shows its progress
    sel = entry_cam == c
    part_out, dt = timed(lambda: CE.host_projection_offsets(intr, extr, fcam, fT, entry_var[sel], entry_var[sel],
                                                            entry_cam[sel], np.ones(int(sel.sum()), np.int64),
                                                            entry_cam[sel], 4, CE.DISTANCES))
    print(f"  host library, camera {c}: {int(sel.sum())} entries in {dt:.2f} s", flush=True)
    host_s += dt
    if host is None:
        host = part_out
    else:
        for k in host:
            host[k][c] = part_out[k][c]
part = "" if host_every == 1 else f" (every {host_every}th rig only: 1 / {host_every} of the entries)"
print(f"host library, {len(entry_var)} entries expanded{part}: {host_s:.2f} s", flush=True)
host_w, host_w_s = timed(lambda: CE.host_projection_offsets(intr, extr, fcam, fT, var, var, cam, weight, cam, 4,
                                                            CE.DISTANCES))
print(f"host library on the {len(var)} weighted pairs: {1e3 * host_w_s:.1f} ms")
if host_every == 1:
    print(f"  expanded vs weighted on the host: worst statistic difference {worst(host, host_w):.2e} of the bound")

if not host_only:
    e = HipEngine()
    chain = np.zeros((3, 24))
    chain[:, :4] = [0, 4, 640, 480]
    chain[:, 9] = [-2.0, 0.0, 1.5]
    e.set_vars(K.VAR_CAM_INTR, np.vstack([intr, chain]), np.r_[np.ones(len(intr)), np.zeros(3)].astype(np.uint8))
    e.set_vars(K.VAR_CAM_EXTR, extr, np.ones(len(extr), np.uint8))
    consts = np.zeros((2, 17))
    consts[:, :4] = 1.0
    n = len(intr)
    e.add_factors(K.F_RW_CAM_INTR, np.array([[n, n + 1], [n + 1, n + 2]], np.int32), None, consts)
    e.finalize()
    args = (fcam, fT, var, var, cam, weight, cam, 4, CE.DISTANCES)
    e.calib_projection_offsets(*args)   # the first call pays the code object's load
    dev, wall = timed(lambda: e.calib_projection_offsets(*args), 5)
    print(f"device, {len(var)} weighted pairs: kernels {e.calib_eval_device_ms():.3f} ms, call {1e3 * wall:.2f} ms wall "
          f"(best of 5); worst statistic difference to the host library on the same pairs {worst(dev, host_w):.2e} "
          f"of the bound")
    if host_every == 1:
        print(f"  host expanded / device call = {host_s / wall:.0f}x; worst statistic difference to the expanded host "
              f"run {worst(dev, host):.2e} of the bound")
    e.close()
