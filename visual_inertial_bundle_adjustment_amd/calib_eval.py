"""Estimated calibration against factory: SingleSessionAdapter::compareCalibrationVsFactory and
showCalibrationCompResults (viba/single_session/EvalCalibration.cpp:15-152), what ark_vi_ba prints under
--eval-calib-vs-factory (interfaces/ark/main_AriaKit_ViBa.cpp:116-120).

The image projection offsets (:57-116) are the expensive part and run on the device
(HipEngine.calib_projection_offsets, vb_calib_projection_offsets); an engine without that call is answered by
the host library (host_projection_offsets, vbh_calib_projection_offsets).  The other statistics are one value
per (rig, sensor): computed here from engine.get_vars, once per distinct variable, weighted by its rig count.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np

from .adapter import ImuJacIndices
from .session import so3_act

DISTANCES = (0.5, 1.0, 2.0, 4.0, 8.0, 16.0)   # EvalCalibration.cpp:59
STEP_X, STEP_Y = 20.0, 15.0                   # :73


@dataclass
class Stats:
    """What showCalibrationCompResults reads of a StatsValueContainer."""
    count: int
    p50: float
    p90: float
    mean: float
    rmse: float

    @staticmethod
    def of(values, weights=None) -> "Stats":
        """of the multiset holding values[i] weights[i] times (StatsValueContainer.cpp:22-71)"""
        v = np.asarray(values, np.float64).reshape(-1)
        w = np.ones(len(v), np.int64) if weights is None else np.asarray(weights, np.int64).reshape(-1)
        v, w = v[w > 0], w[w > 0]
        n = int(w.sum())
        if n == 0:
            return Stats(0, math.nan, math.nan, math.nan, math.nan)
        order = np.argsort(v, kind="stable")
        v, w = v[order], w[order]
        end = np.cumsum(w)

        def at(k):
            return float(v[np.searchsorted(end, k, side="right")])

        def px(pct):
            pos = (pct / 100.0) * (n - 1)
            below, above = math.floor(pos), math.ceil(pos)
            if below == above:
                return at(below)
            wa = pos - below
            return at(below) * (1.0 - wa) + at(above) * wa
        wf = w.astype(np.float64)
        return Stats(n, px(50.0), px(90.0), float((wf * v).sum() / n), math.sqrt(float((wf * v * v).sum() / n)))


def grid_shape(width: float, height: float) -> tuple:
    """(nx, ny) of the reference's pixel grid (:73-77): x = fmod(w / 2, 20), + 20, ... < w and
    y = fmod(h / 2, 15), + 15, ... < h; pixel index g = ix * ny + iy."""
    if not (1 <= width <= 32767 and 1 <= height <= 32767):
        return 0, 0
    nx, x = 0, math.fmod(width * 0.5, STEP_X)
    while x < width:
        nx, x = nx + 1, x + STEP_X
    ny, y = 0, math.fmod(height * 0.5, STEP_Y)
    while y < height:
        ny, y = ny + 1, y + STEP_Y
    return nx, ny


def grid_pixels(width: float, height: float) -> np.ndarray:
    """the grid's pixels in index order, (nx * ny, 2)"""
    nx, ny = grid_shape(width, height)
    x0, y0 = math.fmod(width * 0.5, STEP_X), math.fmod(height * 0.5, STEP_Y)
    return np.array([(x0 + STEP_X * ix, y0 + STEP_Y * iy) for ix in range(nx) for iy in range(ny)]).reshape(-1, 2)


def offsets_call(call, factory_cam, factory_T, cam_intr_var, cam_extr_var, fcam_of_pair, weight, series_of_pair,
                 n_series, distances, want_values=False) -> dict:
    """Marshal the arguments vb_calib_projection_offsets and vbh_calib_projection_offsets share (from n_fcam on)
    and call `call(*args)`, which raises on an error code."""
    fc = np.ascontiguousarray(factory_cam, np.float64).reshape(-1, 24)
    fT = np.ascontiguousarray(factory_T, np.float64).reshape(-1, 7)
    if len(fc) != len(fT):
        raise ValueError("factory_cam and factory_T must have one row per factory camera")
    iv, ev, fp, sp = (np.ascontiguousarray(a, np.int32).reshape(-1)
                      for a in (cam_intr_var, cam_extr_var, fcam_of_pair, series_of_pair))
    w = np.ascontiguousarray(weight, np.int64).reshape(-1)
    if not len(iv) == len(ev) == len(fp) == len(sp) == len(w):
        raise ValueError("the per-pair arrays must have one entry per pair")
    dist = np.ascontiguousarray(distances, np.float64).reshape(-1)
    ns, nd = int(n_series), len(dist)
    max_grid = max([int(np.prod(grid_shape(c[2], c[3]))) for c in fc], default=0)
    shape = (max(ns, 0), nd)
    count = np.zeros(shape, np.int64)
    mean, rmse, p50, p90 = (np.full(shape, np.nan) for _ in range(4))
    values = np.full((len(iv), nd, max_grid), np.nan) if want_values else None
    valid = np.zeros((len(fc), max_grid), np.uint8) if want_values else None
    call(len(fc), fc.ctypes.data, fT.ctypes.data, len(iv), iv.ctypes.data, ev.ctypes.data, fp.ctypes.data,
         w.ctypes.data, sp.ctypes.data, ns, nd, dist.ctypes.data, count.ctypes.data, mean.ctypes.data,
         rmse.ctypes.data, p50.ctypes.data, p90.ctypes.data, None if values is None else values.ctypes.data,
         None if valid is None else valid.ctypes.data)
    out = {"count": count, "mean": mean, "rmse": rmse, "p50": p50, "p90": p90}
    if want_values:
        out["values"], out["valid"] = values, valid.astype(bool)
    return out


def host_projection_offsets(cam_intr, cam_extr, factory_cam, factory_T, cam_intr_var, cam_extr_var, fcam_of_pair,
                            weight, series_of_pair, n_series, distances, want_values=False) -> dict:
    """HipEngine.calib_projection_offsets on the host (libviba_host, vbh_calib_projection_offsets), the camera
    variables given as arrays: cam_intr (n, 24), cam_extr (n, 7).  Every listed pair is evaluated."""
    from ._lib import load_host_lib
    lib = load_host_lib()
    ci = np.ascontiguousarray(cam_intr, np.float64).reshape(-1, 24)
    ce = np.ascontiguousarray(cam_extr, np.float64).reshape(-1, 7)

    def call(*a):
        if lib.vbh_calib_projection_offsets(len(ci), ci.ctypes.data, len(ce), ce.ctypes.data, *a) != 0:
            raise ValueError("vbh_calib_projection_offsets: invalid argument")
    return offsets_call(call, factory_cam, factory_T, cam_intr_var, cam_extr_var, fcam_of_pair, weight,
                        series_of_pair, n_series, distances, want_values)


def rotation_angle(q) -> float:
    """|SO3::log()| of a unit quaternion (x y z w), as Sophus evaluates it"""
    x, y, z, w = (float(v) for v in q)
    sqn = x * x + y * y + z * z
    if sqn < 1e-20:
        return abs(2.0 / w - (2.0 / 3.0) * sqn / (w * w * w)) * math.sqrt(sqn)
    n = math.sqrt(sqn)
    return abs(2.0 * (math.atan2(-n, -w) if w < 0 else math.atan2(n, w)))


def _extrinsics_error(T_var, T_factory) -> tuple:
    """(rotation [deg], translation [mm]) of T_var * T_factory^-1 (:31-37, :123-127) = (R_var R_f^-1,
    t_var - R_var R_f^-1 t_f): in this form a variable equal to the factory value reads exactly 0"""
    T_var, T_factory = np.asarray(T_var, np.float64), np.asarray(T_factory, np.float64)
    # q_var * conj(q_f), the vector part grouped so that equal quaternions cancel term by term
    va, wa, vb, wb = T_var[:3], T_var[3], T_factory[:3], T_factory[3]
    q = np.concatenate([(wb * va - wa * vb) - np.cross(va, vb), [wa * wb + float(np.dot(va, vb))]])
    tr = T_var[4:] - so3_act(q, T_factory[4:])
    return math.degrees(rotation_angle(q)), float(np.linalg.norm(tr)) * 1000.0


def camera_delta_components(var, factory) -> dict:
    """VarSpec<CameraModelParam>::boxMinus(var, factory) cut by CameraModelParam::eachNamedDeltaComponent
    (CameraModelParam.cpp:26-48, 69-86), as norms; var / factory: 24-double camera records."""
    if var[0] != 1.0:
        raise ValueError("Calib field enumeration unsupported for camera type Linear")
    n = int(var[1])
    delta = [float(a) - float(b) for a, b in zip(var[9:9 + n], factory[9:9 + n])]
    out = {"1_FocalLength": delta[0:1], "2_PrincipalPt": delta[1:3], "3_Distorsion": delta[3:9],
           "4_Tangential": delta[9:11], "5_ThinPrism": delta[11:15]}
    if var[7] != 0:
        if factory[4] == 0:
            raise ValueError("factory camera without a readout time (std::bad_optional_access)")
        out["6_ReadoutTime"] = [float(var[5]) - float(factory[5])]
    if var[8] != 0:
        out["7_TimeOffset"] = [float(var[6]) - float(factory[6])]
    return {k: float(np.linalg.norm(v)) for k, v in out.items()}


def imu_delta_components(var, factory, mask: int) -> dict:
    """ImuCalibParam::boxMinus(var, factory) cut by eachNamedDeltaComponent (ImuCalibParam.cpp:119-208), as
    norms, for the estimated blocks of the option mask; var / factory: 32-double records (column-major
    non-orthogonality matrices)."""
    v, f = np.asarray(var, np.float64), np.asarray(factory, np.float64)
    jac = ImuJacIndices(mask)
    d = v - f

    def m(base, r, c):
        return d[base + 3 * c + r]
    out = {}
    if jac.gB >= 0:
        out["1_GyroBiasRadSec"] = d[6:9]
    if jac.aB >= 0:
        out["2_AccelBiasMSec2"] = d[9:12]
    if jac.gS >= 0:
        out["3_GyroScale"] = 1.0 / v[0:3] - 1.0 / f[0:3]
    if jac.aS >= 0:
        out["4_AccelScale"] = 1.0 / v[3:6] - 1.0 / f[3:6]
    if jac.gN >= 0:
        out["5_GyroNonOrth"] = [m(12, 0, 1), m(12, 0, 2), m(12, 1, 0), m(12, 1, 2), m(12, 2, 0), m(12, 2, 1)]
    if jac.aN >= 0:
        out["6_AccelNonOrth"] = [m(21, 0, 1), m(21, 0, 2), m(21, 1, 2)]
    if jac.rT >= 0:
        out["7_RefImuTimeOffset"] = [d[31]]
    if jac.gaT >= 0:
        out["8_GyroAccelTimeOffset"] = [(v[30] - v[31]) - (f[30] - f[31])]
    return {k: float(np.linalg.norm(x)) for k, x in out.items()}


def distance_label(dist: float) -> str:
    """setfill('.') << setw(4) << int(dist * 100) (:104-105)"""
    return str(int(dist * 100)).rjust(4, ".")


def _distinct(handles) -> tuple:
    u, n = np.unique(np.asarray(handles, np.int64), return_counts=True)
    return u, n.astype(np.int64)


def camera_pairs(problem) -> tuple:
    """The distinct (intrinsics variable, extrinsics variable) pairs of rigCamToModelIndex / rigCamToExtrIndex
    over the problem's rigs, with their rig counts: (cam_intr_var, cam_extr_var, slam camera, weight)."""
    nr = len(problem.rig_ts_us)
    var, cam, w = [], [], []
    for c in range(problem.n_cam):
        u, n = _distinct([problem.cam_var(r, c) for r in range(nr)])   # both maps index the same variable row
        var += list(u)
        cam += [c] * len(u)
        w += list(n)
    var = np.array(var, np.int32)
    return var, var.copy(), np.array(cam, np.int32), np.array(w, np.int64)


def compare_calibration_vs_factory(engine, problem, sd, matcher) -> dict:
    """compareCalibrationVsFactory (:26-152) at the engine's current variables: label -> Stats, labels and
    units as the reference's.  problem: the adapter's SessionProblem; sd / matcher: its session."""
    fcal = sd.factory_calib
    nr = len(problem.rig_ts_us)
    cam_intr, cam_extr = engine.get_vars(4).reshape(-1, 24), engine.get_vars(5).reshape(-1, 7)
    imu_calib, imu_extr = engine.get_vars(6).reshape(-1, 32), engine.get_vars(7).reshape(-1, 7)
    fcam = np.array([fcal.cameras[matcher.slam_cam_to_factory[c]].camera_data(False, False)
                     for c in range(problem.n_cam)]).reshape(-1, 24)
    fT = np.array([fcal.T_cam_bodyimu[matcher.slam_cam_to_factory[c]] for c in range(problem.n_cam)]).reshape(-1, 7)
    stats = {}

    def add(label, per_var: list, weights):
        for key in per_var[0] if per_var else ():
            stats[label + key] = Stats.of([d[key] for d in per_var], weights)

    for c in range(problem.n_cam):   # camera extrinsics (:29-38)
        u, n = _distinct([problem.cam_var(r, c) for r in range(nr)])
        err = [_extrinsics_error(cam_extr[v], fT[c]) for v in u]
        add(f"Cam{c}.Extr.", [{"RotDegs": e[0], "TrMMs": e[1]} for e in err], n)
    for c in range(problem.n_cam):   # camera intrinsics (:40-55)
        u, n = _distinct([problem.cam_var(r, c) for r in range(nr)])
        add(f"Cam{c}.Intr.", [camera_delta_components(cam_intr[v], fcam[c]) for v in u], n)

    # image projection offsets (:57-116)
    iv, ev, cam, w = camera_pairs(problem)
    args = (fcam, fT, iv, ev, cam, w, cam, problem.n_cam, DISTANCES)
    if hasattr(engine, "calib_projection_offsets"):
        off = engine.calib_projection_offsets(*args)
    else:
        off = host_projection_offsets(cam_intr, cam_extr, *args)
    for c in range(problem.n_cam):
        for j, dist in enumerate(DISTANCES):
            if off["count"][c, j] > 0:   # a label exists once a sample was added
                stats[f"Cam{c}.ProjOffsetAt{distance_label(dist)}cm"] = Stats(
                    int(off["count"][c, j]), float(off["p50"][c, j]), float(off["p90"][c, j]),
                    float(off["mean"][c, j]), float(off["rmse"][c, j]))

    for i in range(1, problem.n_imu):   # imu extrinsics (:118-128; IMU 0 is the body frame and has no variable)
        u, n = _distinct([problem.imu_extr_var(r, i) for r in range(nr)])
        Tf = fcal.T_imu_bodyimu[matcher.slam_imu_to_factory[i]]
        err = [_extrinsics_error(imu_extr[v], Tf) for v in u]
        add(f"Imu{i}.Extr.", [{"RotDegs": e[0], "TrMMs": e[1]} for e in err], n)
    for i in range(problem.n_imu):      # imu intrinsics (:131-151)
        u, n = _distinct([problem.imu_var(r, i) for r in range(nr)])
        fm = fcal.imu_models[matcher.slam_imu_to_factory[i]]
        add(f"Imu{i}.Intr.", [imu_delta_components(imu_calib[v], fm, problem.imu_calib_options) for v in u], n)
    return stats


def show_calibration_comp_results(stats: dict) -> str:
    """showCalibrationCompResults (:15-23): the labels in std::map order (bytes), the numbers as an ostream
    prints a double (%g, 6 significant digits)."""
    body = "".join(f"{key}:\n  p50: {s.p50:g}, p90: {s.p90:g}, mean: {s.mean:g}, rmse: {s.rmse:g}\n"
                   for key, s in sorted(stats.items(), key=lambda kv: kv[0].encode()))
    return f"Calibration Eval:\n{body}"
