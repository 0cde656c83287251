"""The device triangulation (vb_triangulate_points, csrc/triangulate.hip) against the oracle's triangulatePoint
on the same arrays: the track set of tests/triang_scenes.py (track lengths around the wave width, outliers,
degenerate and failing geometry; tests/test_triangulate.py shows on the CPU that none of its flags hangs on
the last bits), the tracks the adapter builds from two session folders, and the adapter with the device as
its provider."""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import pytest

import triang_scenes
from oracle.refcpu import rs_row_poses as ref_row_poses
from oracle.refcpu import triangulate as ref_triangulate
from visual_inertial_bundle_adjustment_amd import adapter, engine, session, synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "session_small")
POINT_REL = 1e-9   # tests/test_session.py and tests/test_session_gpu.py use the same for this stage


def compare(arrays, label):
    """device vs oracle on one set of arrays: every ok flag, every inlier flag, every point"""
    ref_pts, ref_ok, ref_inl = ref_triangulate(*arrays)
    pts, ok, inl = engine.triangulate(*arrays)
    ms = engine.triangulate.last_device_ms
    diff = float(np.abs(pts - ref_pts).max()) if len(pts) else 0.0
    tol = triang_scenes.point_tolerance(ref_pts, POINT_REL)
    print(f"{label}: {len(ok)} tracks, {len(inl)} observations, {int(ref_ok.sum())} triangulated; ok flags differing "
          f"{int((ok != ref_ok).sum())}, inlier flags differing {int((inl != ref_inl).sum())}, max point difference "
          f"{diff:.3e} (tolerance {tol:.3e}), device {ms:.3f} ms")
    assert pts.shape == ref_pts.shape and ok.shape == ref_ok.shape and inl.shape == ref_inl.shape
    np.testing.assert_array_equal(ok, ref_ok)
    np.testing.assert_array_equal(inl, ref_inl)
    assert diff <= tol
    assert ms > 0.0 and math.isfinite(ms)
    return pts, ok, inl


def test_scene_matches_oracle():
    s = triang_scenes.scene()
    pts, ok, inl = compare(s.arrays, "scene")
    # rejected tracks leave a zero point and zero flags
    bad = np.flatnonzero(ok == 0)
    assert len(bad) == 6 and not pts[bad].any()
    for name in ("empty_first", "empty_last", "len_2", "outliers_many", "degenerate", "behind"):
        assert ok[s.special[name]] == 0 and not inl[s.obs(name)].any()


def test_single_tracks_and_track_order():
    """a track's result does not depend on its neighbours or its slot in the workgroup: each special track alone,
    and the whole set reversed"""
    s = triang_scenes.scene()
    ref_pts, ref_ok, ref_inl = ref_triangulate(*s.arrays)
    n = len(s.start) - 1
    order = np.arange(n)[::-1]
    lens = np.diff(s.start)[order]
    start = np.zeros(n + 1, np.int64)
    start[1:] = np.cumsum(lens)
    idx = np.concatenate([np.arange(s.start[t], s.start[t + 1]) for t in order]).astype(np.int64)
    pts, ok, inl = engine.triangulate(start, s.seeds[order], s.Tcw[idx], s.camvar[idx], s.cams, s.uv[idx], s.sqrt_h[idx])
    np.testing.assert_array_equal(ok, ref_ok[order])
    np.testing.assert_array_equal(inl, ref_inl[idx])
    assert np.abs(pts - ref_pts[order]).max() <= triang_scenes.point_tolerance(ref_pts, POINT_REL)
    for name in ("len_3", "len_65", "len_130", "faces_away", "behind"):
        t, sl = s.special[name], s.obs(name)
        one = (np.array([0, sl.stop - sl.start]), s.seeds[t:t + 1], s.Tcw[sl], s.camvar[sl], s.cams, s.uv[sl], s.sqrt_h[sl])
        p1, ok1, inl1 = engine.triangulate(*one)
        assert ok1[0] == ref_ok[t] and np.array_equal(inl1, ref_inl[sl]), name
        assert np.abs(p1[0] - ref_pts[t]).max() <= triang_scenes.point_tolerance(ref_pts, POINT_REL), name


@functools.lru_cache(maxsize=None)
def golden_adapter():
    sd = session.SessionData.load(GOLDEN)
    a = adapter.SessionAdapter(sd, session.Matcher.build(sd), None, ref_row_poses)
    return sd, a, a.problem()


def test_session_small_tracks_match_oracle():
    _, a, _ = golden_adapter()
    compare(a.triangulation["inputs"], "session_small")


def test_generated_session_tracks_match_oracle(tmp_path):
    p = synth.generate(synth.config("miniB", n_kf=80, n_lm=400))
    synth.write_session(p, str(tmp_path))
    sd = session.SessionData.load(str(tmp_path))
    a = adapter.SessionAdapter(sd, session.Matcher.build(sd), None, ref_row_poses)
    a.problem()
    compare(a.triangulation["inputs"], "miniB n_kf=80 n_lm=400")


def test_adapter_with_the_device_provider():
    """build_problem(triangulate=engine.triangulate) against the default host path on session_small: the same
    points kept, the same visual factors, the points within the stage's tolerance"""
    sd, a, p = golden_adapter()
    b = adapter.SessionAdapter(sd, session.Matcher.build(sd), None, ref_row_poses, triangulate=engine.triangulate)
    q = b.problem()
    np.testing.assert_array_equal(q.point_ids, p.point_ids)
    np.testing.assert_array_equal(q.fvars[0], p.fvars[0])
    np.testing.assert_array_equal(q.fivals[0], p.fivals[0])
    np.testing.assert_array_equal(q.fconsts[0], p.fconsts[0])
    assert q.triangulated == p.triangulated and q.tried_tracks == p.tried_tracks
    assert np.abs(q.vars[0] - p.vars[0]).max() <= triang_scenes.point_tolerance(p.vars[0], POINT_REL)
    np.testing.assert_array_equal(b.triangulation["ok"], a.triangulation["ok"])
    np.testing.assert_array_equal(b.triangulation["inliers"], a.triangulation["inliers"])
    q2 = adapter.build_problem(sd, row_poses=ref_row_poses, triangulate=engine.triangulate)
    np.testing.assert_array_equal(q2.vars[0], q.vars[0])   # the device path repeats itself bit for bit
