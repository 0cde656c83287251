"""vb_calib_projection_offsets on the MI355X (csrc/calib_eval.hip), fp64 and mixed builds, against the host
library (libviba_host, vbh_calib_projection_offsets) and the 50-digit restatement (calib_eval_scenes.hp_offsets).

Bound: 1e-10 max(1, |ref|) px for every sample value, and for mean / rmse / p50 / p90, each 1-Lipschitz in the
sup norm of the samples; counts, valid flags and the present / absent pattern are exact.  A sample may be left
out only under the skip cap (calib_eval_scenes.skip_mask), and the cameras are chosen so that none is.

Measured on the MI355X (both builds give the same bits: the kernels do not depend on VIBA_MIXED):
    device vs host library, four cameras: values 9.5e-13 px (7.2e-3 of the bound), statistics 5.4e-4 of the
                                          bound, 0 skipped
    device vs 50 digits, 50 x 47 camera:  values 1.6e-14 px (1.6e-4 of the bound), statistics 4.4e-5 of the bound
    adapter problem of the golden session, HIP engine vs host fallback: 1.9e-3 of the bound over 57 keys
"""
from __future__ import annotations

import os

import numpy as np
import pytest

import calib_eval_scenes as CS
from visual_inertial_bundle_adjustment_amd import kinds as K
from visual_inertial_bundle_adjustment_amd.engine import HipEngine, VbError

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
NAMES = ["golden", "f120", "linear", "small"]
STATS = ("mean", "rmse", "p50", "p90")


def make_engine(s: dict, precision: str = "fp64") -> HipEngine:
    """A finalized engine whose camera variables are the scene's (constant), beside a three-variable chain of
    Linear intrinsics under two random-walk factors, so that there is something to solve and to cost."""
    e = HipEngine(precision=precision)
    n = len(s["cam_intr"])
    chain = np.zeros((3, 24))
    chain[:, :4] = [0, 4, 640, 480]
    chain[:, 9] = [-2.0, 0.0, 1.5]
    e.set_vars(K.VAR_CAM_INTR, np.vstack([s["cam_intr"], chain]), np.r_[np.ones(n), np.zeros(3)].astype(np.uint8))
    e.set_vars(K.VAR_CAM_EXTR, CS.extr_rows(s), np.ones(n, np.uint8))
    consts = np.zeros((2, 17))
    consts[:, :4] = 1.0
    e.add_factors(K.F_RW_CAM_INTR, np.array([[n, n + 1], [n + 1, n + 2]], np.int32), None, consts)
    e.finalize()
    return e


@pytest.fixture(scope="module")
def four():
    """the four-camera scene and its host-library result, shared and left unchanged"""
    s = CS.scene(NAMES, rot180_pair=(2, 1))
    ref = CS.host(s)
    for v in ref.values():
        v.setflags(write=False)
    return s, ref


def compare(out: dict, ref: dict, skip=None) -> tuple:
    """exact flags / pattern / counts; returns the worst value and statistic error over the bound"""
    assert np.array_equal(out["valid"], ref["valid"])
    present = ~np.isnan(ref["values"])
    if skip is not None:
        assert not skip.any(), f"{int(skip.sum())} samples fall under the skip cap: choose another camera"
    assert np.array_equal(~np.isnan(out["values"]), present)
    assert np.array_equal(out["count"], ref["count"])
    dv = np.abs(out["values"][present] - ref["values"][present])
    worst_v = float(np.max(dv / CS.eps(ref["values"][present]), initial=0.0))
    worst_s = 0.0
    for k in STATS:
        has = ref["count"] > 0
        assert np.array_equal(np.isnan(out[k]), ~has), k
        worst_s = max(worst_s, float(np.max(np.abs(out[k][has] - ref[k][has]) / CS.eps(ref[k][has]), initial=0.0)))
    print(f"worst value error {float(dv.max(initial=0.0)):.3e} px ({worst_v:.3e} of the bound), "
          f"worst statistic {worst_s:.3e} of the bound")
    return worst_v, worst_s


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_device_matches_host_library(four, precision):
    """Four cameras, 3 pairs each with the weights 1, 7 and 3e6 (N > 2^31), one pair turned by 180 degrees (all
    of its samples absent), one series without a pair (count 0, NaN).  Measured: values 9.5e-13 px, statistics
    5.4e-4 of the bound, 0 skipped."""
    s, ref = four
    assert ref["count"].max() > 2 ** 31 and (ref["count"][-1] == 0).all()
    assert np.isnan(ref["values"][7]).all()                       # the turned pair
    assert (~ref["valid"][1]).sum() > 100 and ref["valid"][1].sum() > 100   # f120: an invalid outer region
    behind = np.isnan(ref["values"][3, 0]) & ref["valid"][1]      # f120 at 0.5 m: samples behind the camera
    assert behind.sum() > 0
    skip = CS.skip_mask(CS.host_margins(s), s)
    e = make_engine(s, precision)
    out = e.calib_projection_offsets(*CS.scene_args(s), want_values=True)
    worst_v, worst_s = compare(out, ref, skip)
    assert worst_v <= 1.0 and worst_s <= 1.0
    assert e.calib_eval_device_ms() > 0.0


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
def test_device_matches_50_digits(precision):
    """The 50 x 47 camera (nine pixels: less than a wave) against the 50-digit restatement.  Measured: values
    1.6e-14 px, statistics 4.4e-5 of the bound."""
    s = CS.scene(["small"], weights=(1, 7, 3))
    ref = CS.hp_offsets(s)
    n, mean, rmse, p50, p90 = (np.array(x) for x in zip(*[
        CS.expanded_stats(*_series_samples(ref["values"], s, 0, j)) for j in range(len(CS.DISTANCES))]))
    ref.update(count=np.array([n, 0 * n]), mean=np.array([mean, mean * np.nan]), rmse=np.array([rmse, rmse * np.nan]),
               p50=np.array([p50, p50 * np.nan]), p90=np.array([p90, p90 * np.nan]))
    out = make_engine(s, precision).calib_projection_offsets(*CS.scene_args(s), want_values=True)
    worst_v, worst_s = compare(out, ref, CS.skip_mask(ref, s))
    assert worst_v <= 1.0 and worst_s <= 1.0


def _series_samples(values, s, series, j):
    """(values, weights) of the present samples of one series at distance j"""
    v, w = [], []
    for p in np.flatnonzero(s["series_of_pair"] == series):
        x = values[p, j][~np.isnan(values[p, j])]
        v.append(x), w.append(np.full(len(x), s["weight"][p]))
    return np.concatenate(v), np.concatenate(w)


def test_two_calls_are_bit_identical_and_leave_the_handle_alone(four):
    s, _ = four
    e = make_engine(s)
    e.linearize(True, False)
    before = [e.get_vars(k).copy() for k in range(K.NUM_VAR_KINDS)]
    cost = e.cost(False)
    a = e.calib_projection_offsets(*CS.scene_args(s), want_values=True)
    b = e.calib_projection_offsets(*CS.scene_args(s), want_values=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    for k in range(K.NUM_VAR_KINDS):
        assert e.get_vars(k).tobytes() == before[k].tobytes(), k
    assert e.cost(False) == cost


def test_adapter_problem_matches_host_fallback():
    """compare_calibration_vs_factory on the adapter problem of the golden session: the HIP engine against the
    host fallback (an engine that only has get_vars), every key.  Measured: 1.9e-3 of the bound over 57 keys."""
    from visual_inertial_bundle_adjustment_amd import adapter, session
    from visual_inertial_bundle_adjustment_amd.calib_eval import compare_calibration_vs_factory
    sd = session.SessionData.load(os.path.join(HERE, "golden", "session_small"))
    m = session.Matcher.build(sd)
    p = adapter.build_problem(sd, m)
    e = adapter.load_into(HipEngine(reproj_loss=p.reproj_loss, imu_loss=p.imu_loss,
                                    imu_calib_options=p.imu_calib_options), p)

    class VarsOnly:
        def get_vars(self, k):
            return e.get_vars(k)
    dev, host = compare_calibration_vs_factory(e, p, sd, m), compare_calibration_vs_factory(VarsOnly(), p, sd, m)
    assert list(dev) == list(host) and any("ProjOffsetAt" in k for k in dev)
    worst = 0.0
    for k in dev:
        assert dev[k].count == host[k].count, k
        for f in ("p50", "p90", "mean", "rmse"):
            a, b = getattr(dev[k], f), getattr(host[k], f)
            worst = max(worst, abs(a - b) / float(CS.eps(b)))
    print(f"worst key error {worst:.3e} of the bound over {len(dev)} keys")
    assert worst <= 1.0


def test_run_session_logs_the_evaluation(tmp_path):
    """run_session(eval_calib_vs_factory=True) logs the block after the final histogram; with the flag off the
    log and the outputs are what they are without it; it also runs when the optimization is skipped."""
    from visual_inertial_bundle_adjustment_amd import adapter
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    golden = os.path.join(HERE, "golden", "session_small")
    # without the solve and the point refinement the run is the same bits every time (two LM runs differ in the
    # last digits: fp64 atomics), so logs and files can be compared as they are
    on, off, default = [], [], []
    kw = {"optimize": False, "refine": False}
    _, _, summary = adapter.run_session(golden, str(tmp_path / "on"), log=on.append, eval_calib_vs_factory=True, **kw)
    adapter.run_session(golden, str(tmp_path / "off"), log=off.append, eval_calib_vs_factory=False, **kw)
    adapter.run_session(golden, str(tmp_path / "default"), log=default.append, **kw)
    blocks = [x for x in on if x.startswith("Calibration Eval:\n")]
    assert summary is None and len(blocks) == 1 and on[-1] == blocks[0]
    assert "Cam0.ProjOffsetAt..50cm:\n  p50: " in blocks[0] and "Imu0.Intr.1_GyroBiasRadSec:\n" in blocks[0]
    assert off == default == on[:-1]
    for name in ("online_calibration.jsonl", "open_loop_framerate_trajectory.csv",
                 "closed_loop_framerate_trajectory.csv"):
        ref = (tmp_path / "default" / name).read_bytes()
        assert (tmp_path / "on" / name).read_bytes() == ref and (tmp_path / "off" / name).read_bytes() == ref
    # with the solve, through the settings field: after the final histogram, the last thing logged
    full = []
    adapter.run_session(golden, None, optimizer_settings=Settings.default(max_num_iterations=2), log=full.append,
                        show_histogram=True, settings=adapter.InitSettings(eval_calib_vs_factory=True))
    assert full[-1].startswith("Calibration Eval:\n") and "-~oOo~-" in full[-2] and "optimize:" in full[-3]


def test_error_codes(four):
    s, _ = four
    a = list(CS.scene_args(s))
    e = HipEngine()
    e.set_vars(K.VAR_CAM_INTR, s["cam_intr"], None)
    e.set_vars(K.VAR_CAM_EXTR, CS.extr_rows(s), None)
    with pytest.raises(VbError) as x:
        e.calib_projection_offsets(*a)
    assert x.value.code == -2                                     # VB_E_STATE before vb_finalize
    e = make_engine(s)

    def bad(i, value, code=-1):
        b = list(a)
        b[i] = value
        with pytest.raises(VbError) as x:
            e.calib_projection_offsets(*b)
        assert x.value.code == code, x.value

    def poke(arr, value):
        arr = np.array(arr)
        arr[1] = value
        return arr
    n_intr = len(s["cam_intr"]) + 3
    bad(2, poke(a[2], n_intr)), bad(2, poke(a[2], -1))            # intrinsics variable out of range
    bad(3, poke(a[3], len(s["cam_extr"]))), bad(3, poke(a[3], -1))   # extrinsics variable
    bad(4, poke(a[4], len(NAMES))), bad(4, poke(a[4], -1))        # factory camera
    bad(5, poke(a[5], -1))                                        # negative weight
    bad(6, poke(a[6], a[7])), bad(6, poke(a[6], -1))              # series out of range
    bad(8, np.zeros(0))                                           # n_dist <= 0
    out = e.calib_projection_offsets(*a)                          # and the handle still answers
    assert out["count"][0, 0] > 0
    # VB_E_UNSUPPORTED on a landmark shard and on a partitioned rank, as for the residual report
    from visual_inertial_bundle_adjustment_amd import synth
    p = synth.generate(synth.config("A"))
    shard = synth.load_into(HipEngine(imu_calib_options=p.imu_calib_options), p, finalize=False)
    shard.set_landmark_shard(0, 100, True)
    part = synth.load_into(HipEngine(imu_calib_options=p.imu_calib_options), p, finalize=False)
    part.set_partition(0, 2)
    for h in (shard, part):
        h.finalize()
        with pytest.raises(VbError) as x:
            h.calib_projection_offsets(*a)
        assert x.value.code == -6
