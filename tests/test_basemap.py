"""Base-map visual factors without a GPU: the C-ABI's declarations and exports, the scenes of
tests/basemap_scenes.py on the CPU oracle in constant-variable form (P2: what the GPU tests compare the engine
against must exercise every loss zone and failure class before anything is compared), the finalize stage as a
stand-alone program under AddressSanitizer and UBSan (tests/cpp/basemap_check.cpp), and the report's
`Base map factors` text against a golden string."""
from __future__ import annotations

import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import basemap_scenes as bs
from oracle.refcpu import RefEngine
from test_symbolic import FLAGS, HIPCC, SANITIZE, dump_generated
from visual_inertial_bundle_adjustment_amd import report as R
from visual_inertial_bundle_adjustment_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "visual_inertial_bundle_adjustment_amd", "csrc")
REF = os.path.join(ROOT, "oracle", "_ref")
GOLDEN = os.path.join(ROOT, "tests", "golden", "basemap_report.txt")
ENTRY_POINTS = ("vb_set_basemap", "vb_add_basemap_factors", "vb_num_basemap_factors", "vb_basemap_errors",
                "vb_basemap_histogram")
VB_E_ARG = -1


# ---------------------------------------------------------------- the C-ABI
def test_header_declares_and_libraries_export_the_entry_points():
    with open(os.path.join(ROOT, "include", "viba_hip.h")) as fh:
        header = fh.read()
    libdir = os.path.join(ROOT, "visual_inertial_bundle_adjustment_amd", "lib")
    for name in ENTRY_POINTS:
        assert re.search(rf"^int {name}\(vb_handle h,", header, re.M), name
    assert "BaseMapVisualFactor" in header and "MultiSessionProblemImpl.h:19-40" in header
    assert "vb_inspect_nonlinearities and vb_factor_expected_delta leave the" in header
    for lib in ("libviba_hip.so", "libviba_hip_mixed.so"):
        syms = subprocess.run(["nm", "-D", "--defined-only", os.path.join(libdir, lib)], capture_output=True, text=True,
                              check=True).stdout
        for name in ENTRY_POINTS:
            assert re.search(rf" T {name}$", syms, re.M), (lib, name)
    # the 14 factor kinds stay: the base map is a table of the handle
    from visual_inertial_bundle_adjustment_amd import kinds
    assert kinds.NUM_FACTOR_KINDS == 14 and re.search(r"VB_NUM_FACTOR_KINDS\s*=?\s*14", header)


def test_problem_containers_carry_an_optional_basemap():
    from visual_inertial_bundle_adjustment_amd.adapter import SessionProblem
    assert synth.GeneratedProblem().basemap is None and SessionProblem().basemap is None
    assert synth.generate(synth.config("A")).basemap is None


# ---------------------------------------------------------------- the oracle on P2
def _rows(ref, first, n):
    """the appended visual rows' residuals and validity on the oracle"""
    e, valid = np.zeros((n, 2)), np.zeros(n, bool)
    for i in range(n):
        m, r, _ = ref.eval_factor(0, first + i, with_jac=False)
        e[i, :m], valid[i] = r, m > 0
    return e, valid


@functools.lru_cache(maxsize=None)
def oracle_step(scene, which):
    """P2 on the oracle: the appended rows at x0, then after one LM step (one_step's first half)"""
    p1, p2, first = bs.scene_pair(scene, which)
    ref = bs.load(RefEngine, p2)
    n = p1.basemap.num_factors
    e0, v0 = _rows(ref, first, n)
    ref.linearize(True, False)
    ref.damp_factor_solve(1e-5)
    step = ref.get_step(0)
    ref.backup()
    ref.apply_step(0)
    e1, v1 = _rows(ref, first, n)
    return {"e0": e0, "v0": v0, "v1": v1, "step": step, "points1": ref.get_vars(0)}


@pytest.mark.parametrize("scene,which", bs.CASES)
def test_oracle_scene_exercises_every_zone_and_failure_class(scene, which):
    p1, p2, first = bs.scene_pair(scene, which)
    bm = p1.basemap
    o = oracle_step(scene, which)
    n = bm.num_factors
    norm = np.linalg.norm(o["e0"][o["v0"]], axis=1)
    zones = (int((norm < 1).sum()), int(((norm >= 1) & (norm < 3)).sum()), int((norm >= 3).sum()))
    print(f"{scene} {which}: {n} rows, {int((~o['v0']).sum())} failing at x0, |e| < 1 / 1..3 / >= 3: {zones}, "
          f"{int((o['v0'] & ~o['v1']).sum())} valid -> invalid, {int((~o['v0'] & o['v1']).sum())} invalid -> valid")
    assert len(p2.fivals[0]) == first + n and np.all(p2.fivals[0][first:] == -1) and np.all(p2.fvars[0][first:, 4] == -1)
    if scene == "frozen":
        assert len(bm.T_bodyimu_world) == 3 and n > 100
        assert all(z > 0 for z in zones), zones  # quadratic, Huber and cut-off zone of the reprojection loss
        assert (~o["v0"]).sum() >= 20  # failing at the linearization point: cached -1, numPrevInvalid
        const_rows = p1.const[0][bm.point] == 1
        assert const_rows.sum() >= 10 and len(np.unique(bm.point[const_rows])) == 10  # cost and CostStats only
        assert np.all(o["step"][np.unique(bm.point[const_rows])] == 0.0)
    else:
        assert n == 60 and o["v0"].all()  # valid at x0 ...
        assert np.abs(o["e0"]).max() < 1e-6  # ... with the target on the principal point
        assert (o["v0"] & ~o["v1"]).sum() >= 1  # ... failing after the step: numInvalid, the cached cost counted
    # no row's validity hangs on rounding, before or after the step
    for what, z, valid in (("x0", bs.camera_depths(p1), o["v0"]), ("the step", bs.camera_depths(p1, o["points1"]), o["v1"])):
        assert np.array_equal(z >= 1e-6, valid)
        margin = float(np.abs(z - 1e-6).min())
        print(f"{scene} {which}: min |z - 1e-6| at {what} {margin:.3e}")
        assert margin > 1e-7


def test_oracle_accepts_lone_points_and_all_constant_rows():
    """a point that only constant-rig rows see gets a finite, non-zero step; a row whose arguments are all
    constant adds cost and leaves its point where it is (the two facts the engine's lone landmarks and
    constant-point factors are compared against)"""
    p1 = bs.lone_scene()
    p2, first = bs.constant_form(p1)
    ref = bs.load(RefEngine, p2)
    c0 = ref.linearize(True, False)
    ref.damp_factor_solve(1e-5)
    step = ref.get_step(0)
    lone, const = bs.LONE_POINTS, bs.CONST_POINTS
    assert np.isfinite(c0) and np.all(np.isfinite(step[lone])) and np.all(np.abs(step[lone]).max(axis=1) > 0)
    assert np.all(step[const] == 0.0)


# ---------------------------------------------------------------- the finalize stage, stand-alone
@functools.lru_cache(maxsize=None)
def checker():
    os.makedirs(REF, exist_ok=True)
    obj, main, exe = (os.path.join(REF, n) for n in ("basemap_symbolic_host.o", "basemap_check.o", "basemap_check"))
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(CSRC, "symbolic.hip"), "-o", obj])
    subprocess.check_call([HIPCC, *FLAGS, "-c", os.path.join(ROOT, "tests", "cpp", "basemap_check.cpp"), "-o", main])
    subprocess.check_call([HIPCC, *SANITIZE, "-o", exe, main, obj])
    return exe


def dump_with_basemap(path, p, points=None):
    dump_generated(path, p)
    pts = np.asarray(p.basemap.point if points is None else points, np.int32)
    with open(path, "ab") as f:
        np.array([len(pts)], np.int64).tofile(f)
        pts.tofile(f)
    return str(path)


def run_checker(*args):
    r = subprocess.run([checker(), *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout


@pytest.mark.parametrize("name", ["frozen-A", "edge-miniB", "lone-A", "none-A"])
def test_finalize_stage_orders_the_factors(name, tmp_path):
    if name == "lone-A":
        p = bs.lone_scene()
    elif name == "none-A":
        p = synth.generate(synth.config("A"))
        p.basemap = synth.BaseMap(np.zeros((0, 7)), np.zeros(0, np.int32), np.zeros((0, 7)), np.zeros((0, 24)))
    else:
        p = bs.scene_pair(*name.split("-"))[0]
    out = run_checker(dump_with_basemap(tmp_path / "p.bin", p))
    print(out)
    if name == "lone-A":
        assert f"{len(bs.LONE_POINTS)} lone" in out
    elif name == "none-A":
        assert "no base-map factors" in out
    else:
        assert " 0 lone" in out and f"{p.basemap.num_factors} base-map factors" in out


def test_finalize_stage_rejects_an_unknown_point(tmp_path):
    p = synth.generate(synth.config("A"))
    p.basemap = None
    path = dump_with_basemap(tmp_path / "p.bin", p, points=[0, len(p.const[0])])
    assert f"ok: {VB_E_ARG} " in run_checker(path, "--expect", str(VB_E_ARG))


# ---------------------------------------------------------------- the report's text
def report_arrays():
    """fixed per-factor arrays: 40 base-map factors over every pixel bin, 3 failing; 6 visual factors"""
    e = np.array([[0.15 * i, 0.05 * (i % 7)] for i in range(40)])
    valid = np.ones(40, bool)
    valid[[4, 19, 33]] = False
    sq = 0.5 * (e ** 2).sum(axis=1)
    s = 2 * sq
    cost = np.where(s < 1, 0.5 * s, np.where(s < 9, 0.5 * (2 * np.sqrt(s) - 1), 0.5 * 5.0))  # HuberLossWithCutoff(1, 3)
    bm = {"raw": e, "sq_unweighted": sq, "cost": cost, "valid": valid}
    ev = np.array([[0.2, 0.1], [0.7, -0.4], [1.5, 0.3], [0.0, 0.05], [2.5, 2.5], [0.4, 0.4]])
    sv = 0.5 * (ev ** 2).sum(axis=1)
    vis = {"raw": ev, "sq_unweighted": sv, "sq_weighted": sv, "cost": sv, "valid": np.ones(6, bool)}
    return vis, bm


@pytest.mark.parametrize("simple", [False, True])
def test_report_text_matches_the_golden_string(simple):
    vis, bm = report_arrays()
    rep = R.residual_report(R.ArraySource({0: vis}, basemap=bm), simple_stats=simple)
    assert [s.title for s in rep.sections] == ["visual factors", "Base map factors"]
    sec = rep.sections[1]
    assert (sec.n_factors, sec.n_failing) == (40, 3) and ("pixel" in sec.histograms) == (not simple)
    with open(GOLDEN, encoding="utf-8") as fh:
        golden = fh.read().split("=====\n")
    assert sec.text == golden[1 if simple else 0]
    # without base-map factors the report is what it was, byte for byte
    plain = R.residual_report(R.ArraySource({0: vis}), simple_stats=simple)
    assert [s.text for s in plain.sections] == [rep.sections[0].text]
