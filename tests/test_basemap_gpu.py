"""Base-map visual factors on the GPU (csrc/basemap.hip, the landmark / refinement / report hooks and the C-ABI):
the HIP engine on P1 (a handle with a base map) against the unchanged CPU oracle on P2, the same problem in
constant-variable form (tests/basemap_scenes.py), and against the 50-digit reference (tests/hp_reference.py).

Bounds are the project's own: assert_step_parity of tests/test_parity_gpu.py (costs 1e-10, gradient 1e-10, step
1e-8, sub-step 1e-7, variables 1e-10, CostStats exact), gradient_entry_errors 1e-10 for the point kind, the
trajectory rule of test_optimize_trajectory_matches_oracle, the refinement bounds of
test_refine_points_matches_oracle, the report bounds of tests/test_residual_report_gpu.py, the covariance bound of
tests/test_point_covariances.py (1e-7) and the mixed-build figures of test_mixed_precision_step_tolerance.  The
HIP engine on P2 runs beside P1 as a control and its figures are printed.  Every test here needs the base-map
entry points and fails on an engine without them.

Measured on an MI355X (worst over the scenes of a check).  One step, P1 against the oracle on P2 (the control, the
engine on P2, in brackets): cost 5e-15 (5e-15), accepted cost 3e-13 (2e-13), gradient 1.2e-13 (1.2e-13), step
3.0e-11 (3.0e-11), sub-step 1.4e-10 (1.4e-10), variables 3.9e-12 (3.9e-12), CostStats equal; point gradient entries
1.4e-12 (A) and 3.6e-12 (miniB) of their terms' magnitudes.  `optimize`: 5 iterations on both engines, final costs
equal to the 12 digits printed.  Refinement: statistics equal, costs and points within their bounds.  Against 50
digits, both builds alike: cost 1.9e-12, point gradient 2.0e-12, point step 3.5e-11; at z = 2e-6 cost 8.2e-9 and
gradient 5.3e-9 relative (inside `case_bounds`), the step's backward error 3e-3 of its bound.  Report: rows 2.0e-13,
norms and costs 7.2e-13, every count equal, no oracle value near an edge.  Point covariances: 1.6e-13 against the
engine on P2, 1.9e-11 against the oracle.  Mixed build on miniB: gradient 2.5e-8, step 3.3e-5.  No bound was
widened and no kernel changed for a figure."""
from __future__ import annotations

import functools

import numpy as np
import pytest
from mpmath import mp, mpf

import basemap_scenes as bs
import hp_reference as hp
import visual_scenes as vs
from oracle.refcpu import RefEngine
from parity_util import gradient_entry_errors, one_step, rel
from test_parity_gpu import assert_step_parity
from test_residual_report_gpu import check_histogram, code_of, visual_cost_of
from test_visual_reference import case_bounds, loss_probe
from visual_inertial_bundle_adjustment_amd import kinds as K
from visual_inertial_bundle_adjustment_amd import report as R
from visual_inertial_bundle_adjustment_amd import synth
from visual_inertial_bundle_adjustment_amd.engine import Settings

pytestmark = pytest.mark.gpu

APPENDED_KINDS = (1, 4, 5)  # P2 appends constant poses, intrinsics and extrinsics: compare the first n rows
PER_KIND = ("grad", "step", "substep", "vars1")
ARG, STATE, UNSUPPORTED = -1, -2, -6


def hip():
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    return HipEngine


def trimmed(out, p1):
    """one_step's result on P2 with the rows of the appended constant variables (all zero steps) cut off"""
    o = dict(out)
    for key in PER_KIND:
        rows = list(out[key])
        for k in APPENDED_KINDS:
            extra = rows[k][len(p1.const[k]):]
            if key != "vars1":
                assert np.all(extra == 0.0), (key, k)
            rows[k] = rows[k][:len(p1.const[k])]
        o[key] = rows
    return o


@functools.lru_cache(maxsize=None)
def oracle_one_step(scene, which):
    p1, p2, _ = bs.scene_pair(scene, which)
    r = bs.load(RefEngine, p2)
    return r, trimmed(one_step(r), p1)


def figures(og, orf):
    return {"cost0": abs(og["cost0"] - orf["cost0"]) / abs(orf["cost0"]),
            "cost1": abs(og["cost1"] - orf["cost1"]) / abs(orf["cost1"]),
            "grad": max(rel(a, b) for a, b in zip(og["grad"], orf["grad"]) if b.size),
            "step": max(rel(a, b) for a, b in zip(og["step"], orf["step"]) if b.size),
            "substep": max(rel(a, b) for a, b in zip(og["substep"], orf["substep"]) if b.size),
            "vars1": max(rel(a, b) for a, b in zip(og["vars1"], orf["vars1"]) if b.size)}


def show(what, fig):
    print(f"[basemap] {what}: " + ", ".join(f"{k} {v:.2e}" for k, v in fig.items()))


# ---------------------------------------------------------------- 1. one LM step
@pytest.mark.parametrize("scene,which", bs.CASES)
def test_one_lm_step_matches_the_oracle_in_constant_form(scene, which):
    p1, p2, _ = bs.scene_pair(scene, which)
    r, orf = oracle_one_step(scene, which)
    g = bs.load(hip(), p1)
    assert g.num_basemap_factors() == p1.basemap.num_factors
    assert g.reduced_order() == r.reduced_order() and g.total_order() == r.total_order()
    og = one_step(g)
    control = trimmed(one_step(bs.load(hip(), p2)), p1)
    show(f"{scene} {which} P1 (base map) vs oracle P2", figures(og, orf))
    show(f"{scene} {which} P2 (control)  vs oracle P2", figures(control, orf))
    print(f"[basemap] {scene} {which} CostStats {og['stats1']} / control {control['stats1']} / oracle {orf['stats1']}")
    assert_step_parity(og, orf)
    worst = gradient_entry_errors(og["grad"][:1], orf["grad"][:1], r)
    print(f"[basemap] {scene} {which} point gradient entries / term magnitudes: {worst}")
    assert worst[0] < 1e-10, worst
    g.close()


# ---------------------------------------------------------------- 2. trajectory
@pytest.mark.parametrize("scene", ["frozen", "edge"])
def test_optimize_trajectory_matches_the_oracle(scene):
    p1, p2, _ = bs.scene_pair(scene, "A")
    g, r = bs.load(hip(), p1), bs.load(RefEngine, p2)
    assert not g.spec_prepare()  # no speculative linearization beside base-map factors: the plain controller
    s = Settings.default(max_num_iterations=5)
    sg, sr = g.optimize(s), r.optimize(s)
    print(f"[basemap] {scene} A optimize: {sg.num_iterations} iterations, final cost {sg.final_cost:.12g} / {sr.final_cost:.12g}")
    assert sg.num_iterations == sr.num_iterations and sg.num_troubled_seqs == sr.num_troubled_seqs
    assert abs(sg.initial_cost - sr.initial_cost) <= 1e-11 * sr.initial_cost
    assert abs(sg.final_cost - sr.final_cost) <= 1e-9 * sr.final_cost
    for k in range(1, K.NUM_VAR_KINDS - 1):
        n = len(p1.const[k])
        if n:
            assert rel(g.get_vars(k), r.get_vars(k)[:n]) < 1e-7, K.VAR_NAMES[k]
    g.close()


# ---------------------------------------------------------------- 3. point refinement
@pytest.mark.parametrize("name", ["frozen-A", "lone-A"])
def test_refine_points_matches_the_oracle(name):
    """refinePoints with the points' base-map factors (PointRefinement.cpp:30-39); lone-A: points that only
    base-map factors see are refined too"""
    p1 = bs.lone_scene() if name == "lone-A" else bs.scene_pair("frozen", "A")[0]
    p2, _ = bs.constant_form(p1)
    g, r = bs.load(hip(), p1), bs.load(RefEngine, p2)
    (sg, eg), stg = g.refine_points()
    (sr, er), str_ = r.refine_points()
    print(f"[basemap] {name} refine: cost {sg:.6g} -> {eg:.6g} (oracle {sr:.6g} -> {er:.6g}), stats {stg} / {str_}")
    assert stg == str_
    assert abs(sg - sr) <= 1e-10 * sr and abs(eg - er) <= 1e-10 * er
    assert rel(g.get_vars(0), r.get_vars(0)) < 1e-9
    if name == "lone-A":
        assert np.abs(g.get_vars(0)[bs.LONE_POINTS] - p1.vars[0][bs.LONE_POINTS]).max() > 0  # they moved
    assert_step_parity(one_step(g), trimmed(one_step(r), p1))  # the LM step from the refined points
    g.close()


def test_lone_landmarks_step_with_the_oracle():
    """free points with base-map factors and no visual row: landmarks with an empty observation range and panel
    (landmark_lone_kernel), and constant points whose base-map factors add cost and CostStats only"""
    p1 = bs.lone_scene()
    p2, _ = bs.constant_form(p1)
    g, r = bs.load(hip(), p1), bs.load(RefEngine, p2)
    og, orf = one_step(g), trimmed(one_step(r), p1)
    show("lone A vs oracle P2", figures(og, orf))
    assert_step_parity(og, orf)
    assert np.all(np.abs(og["step"][0][bs.LONE_POINTS]).max(axis=1) > 0) and np.all(og["step"][0][bs.CONST_POINTS] == 0)
    # their covariance is not offered; a point with visual rows keeps its own
    assert code_of(lambda: g.compute_point_covariances([int(bs.LONE_POINTS[0])])) == UNSUPPORTED
    covs, _ = g.compute_point_covariances([0])
    assert covs[0].shape == (3, 3)
    g.close()


# ---------------------------------------------------------------- 4. the 50-digit reference
def one_factor_engine(case, consts, reproj_loss=(1.0, 3.0), precision="fp64"):
    """case.build's one-factor problem (point 0 and the case's pose, extrinsics and camera as variables, one
    VB_F_VISUAL row) beside point 1, the same X, alone with one base-map factor whose key rig and camera hold the
    case's pose, extrinsics and record as constants"""
    e = hip()(reproj_loss=reproj_loss, precision=precision)
    c = case.const
    e.set_vars(K.VAR_POINT, np.stack([case.X, case.X]), np.array([c[0], 0], np.uint8))
    e.set_vars(K.VAR_POSE, case.pose[None], np.array([c[1]], np.uint8))
    e.set_vars(K.VAR_CAM_INTR, case.cam[None], np.array([c[3]], np.uint8))
    e.set_vars(K.VAR_CAM_EXTR, case.extr[None], np.array([c[2]], np.uint8))
    e.add_factors(K.F_VISUAL, np.array([[0, 0, 0, 0, -1]]), np.array([-1]), np.asarray(consts, float)[None])
    e.set_basemap(T_bodyimu_world=case.pose[None], keyrig_of_camera=[0], T_cam_bodyimu=case.extr[None], cams=case.cam[None])
    e.add_basemap_factors([1], [0], np.asarray(consts, float)[None])
    e.finalize()
    return e


@hp._hp
def point_step(ref, lam):
    """-(damped rho' Jp^T Jp)^-1 rho' Jp^T e of the point block alone, at 50 digits; the 2-norm condition
    number of the damped block (its eigenvalues at 50 digits: at z = 2e-6 they span 21 decades); the block"""
    Jp, lam = ref.J[0], mpf(float(lam))
    H = mp.zeros(3, 3)
    for i in range(3):
        for j in range(3):
            H[i, j] = ref.drho * (Jp[0][i] * Jp[0][j] + Jp[1][i] * Jp[1][j])
        H[i, i] = H[i, i] * (1 + lam) + lam
    x = mp.lu_solve(H, mp.matrix([ref.grad[0][i] for i in range(3)]))
    ev = [abs(v) for v in mp.eigsy(H, eigvals_only=True)]
    return np.array([-float(x[i]) for i in range(3)]), float(max(ev) / min(ev)), np.array(H.tolist(), float)


def pick_lambda(ref, step_tol=1e-8):
    """the first damping of 1e-5 x 10^k with cond(damped block) 2^-52 64 < step_tol on the reference's own
    matrix (MicroBundle.pick_lambda's rule): a step mismatch is then not conditioning"""
    for k in range(12):
        lam = 1e-5 * 10.0 ** k
        step, cond, H = point_step(ref, lam)
        if cond * vs.EPS * 64 < step_tol:
            break
    return lam, step, cond, H


def check_basemap_factor(e, case, ref, consts, tag, cost_tol, g_tol):
    """the base-map factor of point 1 against the reference: its reported cost, the linearization's and the
    cost pass's totals (the visual row of point 0 is the same factor: twice the reference), the point gradient
    and the point step"""
    got = e.basemap_errors()
    c_lin = e.linearize(True, False)
    c_pass, stats = e.cost(False)
    grad = e.get_gradient(K.VAR_POINT)[1]
    if not ref.valid:
        assert not got["valid"][0] and got["cost"][0] == 0.0 and np.all(got["raw"] == 0.0)
        assert c_lin == 0.0 and c_pass == 0.0 and tuple(stats) == (2, 2, 2) and np.all(grad == 0.0)
        return {}
    cost = float(ref.cost)
    assert got["valid"][0] and tuple(stats) == (2, 0, 0)
    gr = hp.to_float(ref.grad[0])
    fig = {"cost": abs(got["cost"][0] - cost) / cost, "total": abs(c_lin - 2 * cost) / (2 * cost),
           "grad": float(np.abs(grad - gr).max() / max(np.abs(gr).max(), 1e-300))}
    assert abs(got["cost"][0] - cost) <= cost_tol, (tag, got["cost"][0], cost)
    assert abs(c_lin - 2 * cost) <= 2 * cost_tol and abs(c_pass - 2 * cost) <= 2 * cost_tol, (tag, c_lin, c_pass, cost)
    assert np.abs(grad - gr).max() <= g_tol, (tag, grad, gr)
    if ref.drho == 0:  # beyond the cutoff: no weight, a zero gradient and step
        assert np.all(grad == 0.0)
    lam, step, cond, H = pick_lambda(ref)
    e.damp_factor_solve(lam)
    got_step = e.get_step(K.VAR_POINT)[1]
    if case.illcond:
        # z = 2e-6: the block's eigenvalues span 21 decades at any damping the loop tries (d uv / d p_c ~ f / z
        # against the damping along the ray), so no forward bound on the step means anything.  The backward
        # error does: the engine's step solves its own system, whose gradient is off by at most g_tol
        # (case_bounds) and whose block by two Jacobian factors at 1e-10 each plus the solve's 1e-8
        resid = np.abs(H @ (got_step - step)).max()
        bound = g_tol + (2e-10 + 1e-8) * np.abs(H).max() * np.abs(step).max() * 3
        fig["step (backward error / bound)"] = float(resid / bound)
        assert resid <= bound, (tag, lam, cond, got_step, step)
    elif np.abs(step).max() > 0:
        assert cond * vs.EPS * 64 < 1e-8, (tag, lam, cond)  # on the reference alone: a mismatch is not conditioning
        fig["step"] = float(np.abs(got_step - step).max() / np.abs(step).max())
        assert fig["step"] <= 1e-8, (tag, lam, cond, got_step, step)
    else:
        assert np.all(got_step == 0.0)
    return fig


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("case", vs.geometric_cases(), ids=repr)
def test_basemap_factor_matches_the_reference(case, precision):
    for target in vs.E_TARGETS:
        consts = case.consts_for(target)
        ref = case.reference(consts)
        assert ref.valid == case.expect_valid
        cost_tol, g_tol = 0.0, 0.0
        if ref.valid:
            _, _, cost_tol, g_tols = case_bounds(case, ref, consts)
            g_tol = g_tols[0]
        e = one_factor_engine(case, consts, precision=precision)
        fig = check_basemap_factor(e, case, ref, consts, f"{case} {precision}", cost_tol, g_tol)
        show(f"{case} {precision} vs 50 digits", fig)
        e.close()


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("name,reproj_loss,s", vs.LOSS_CASES, ids=[c[0] for c in vs.LOSS_CASES])
def test_basemap_factor_loss_zones(name, reproj_loss, s, precision):
    case, consts, ref = loss_probe(name, reproj_loss, s)
    e = one_factor_engine(case, consts, reproj_loss=reproj_loss, precision=precision)
    gmax = np.abs(hp.to_float(ref.grad[0])).max()
    fig = check_basemap_factor(e, case, ref, consts, f"{name} {precision}", 1e-10 * float(ref.cost), 1e-10 * gmax)
    show(f"{name} {precision} vs 50 digits", fig)
    if name.startswith("cutoff"):
        assert gmax == 0.0
    e.close()


# ---------------------------------------------------------------- 5. the report
@functools.lru_cache(maxsize=None)
def oracle_rows(scene, which):
    """the oracle's residuals, validity and costs of P2's appended rows at x0"""
    p1, p2, first = bs.scene_pair(scene, which)
    ref = bs.load(RefEngine, p2)
    n = p1.basemap.num_factors
    raw, valid = np.zeros((n, 2)), np.zeros(n, bool)
    for i in range(n):
        m, e, _ = ref.eval_factor(K.F_VISUAL, first + i, with_jac=False)
        raw[i, :m], valid[i] = e, m > 0
    sq = 0.5 * (raw ** 2).sum(axis=1)
    cost = np.zeros(n)
    cost[valid] = visual_cost_of(2.0 * sq[valid])
    return raw, valid, sq, cost


@pytest.mark.parametrize("precision", ["fp64", "mixed"])
@pytest.mark.parametrize("scene,which", [("frozen", "A"), ("frozen", "miniB")])
def test_report_matches_the_oracle(scene, which, precision):
    """(the frozen scenes: the edge scene's residuals are exactly zero, on the histograms' first edge)"""
    p1, p2, first = bs.scene_pair(scene, which)
    raw, valid, sq, cost = oracle_rows(scene, which)
    n = len(raw)
    e = bs.load(hip(), p1, precision=precision)
    got = e.basemap_errors()
    assert got["raw"].shape == (n, 2) and np.array_equal(got["valid"], valid)
    scale = np.maximum(1.0, np.linalg.norm(raw, axis=1))
    worst = {"raw": float((np.abs(got["raw"] - raw).max(axis=1) / scale).max()),
             "sq": float((np.abs(got["sq_unweighted"] - sq) / np.maximum(1e-300, sq))[valid].max()),
             "cost": float((np.abs(got["cost"] - cost) / np.maximum(1e-300, cost))[valid].max())}
    assert np.all(got["raw"][~valid] == 0) and np.all(got["cost"][~valid] == 0) and np.all(got["sq_unweighted"][~valid] == 0)
    assert np.array_equal(got["sq_weighted"], got["sq_unweighted"])
    assert n > 130
    for lo, m in ((0, 1), (37, 91), (63, 2), (n - 1, 1), (n - 40, 40), (5, 0), (n, 0)):
        part = e.basemap_errors(lo, m)
        for key, v in part.items():
            assert len(v) == m and np.array_equal(v, got[key][lo:lo + m]), (lo, m, key)
    values = np.sqrt(2.0 * sq)
    for which_err, hist in ((K.ERR_UNWEIGHTED, R.pixel_histogram()), (K.ERR_WEIGHTED, R.weighted_histogram())):
        h = e.basemap_histogram(which_err, hist.edges)
        as_groups = {"counts": h["counts"][None], "cost": np.array([h["cost"]]), "n_factors": np.array([h["n_factors"]]),
                     "n_failing": np.array([h["n_failing"]])}
        worst["hist cost"] = max(worst.get("hist cost", 0.0),
                                 check_histogram(as_groups, values, valid, cost, hist.edges, None, 1, f"which {which_err}"))
        assert h["n_factors"] == n and h["n_failing"] == int((~valid).sum())
    show(f"{scene} {which} {precision} report vs oracle", worst)
    assert max(worst.values()) <= 1e-10
    # the visual kind's report counts no base-map factor
    vh = e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, R.weighted_histogram().edges)
    assert vh["n_factors"][0] == len(p1.fivals[0]) == e.num_factors(K.F_VISUAL)
    # the formatted report: the visual sections, then one `Base map factors` section
    rep = R.residual_report(e)
    titles = [s.title for s in rep.sections]
    assert titles.count("Base map factors") == 1 and titles.index("Base map factors") == titles.index("visual factors") + 1
    sec = rep.sections[titles.index("Base map factors")]
    assert (sec.n_factors, sec.n_failing) == (n, int((~valid).sum())) and abs(sec.cost - cost.sum()) <= 1e-10 * cost.sum() + 1e-300
    e.close()


def test_report_leaves_the_lm_state_untouched():
    """the state test of tests/test_residual_report_gpu.py with the base-map report calls in between: one
    linearization and solve, the step applied and undone before and after them"""
    p1 = bs.scene_pair("frozen", "miniB")[0]
    a = bs.load(hip(), p1)
    a.linearize(True, False)
    a.damp_factor_solve(1e-5)

    def stepped(x):
        x.backup()
        ratios = x.apply_step(0)
        cost, stats = x.cost(True)
        out = (ratios, cost, stats, [x.get_vars(k) for k in range(K.NUM_VAR_KINDS)])
        x.restore()
        return out

    def same_state(x):
        return ([x.get_step(k) for k in range(K.NUM_VAR_KINDS - 1)], [x.get_gradient(k) for k in range(K.NUM_VAR_KINDS - 1)],
                [x.get_vars(k) for k in range(K.NUM_VAR_KINDS)])

    before, state0 = stepped(a), same_state(a)
    a.basemap_errors()
    a.basemap_histogram(K.ERR_WEIGHTED, R.weighted_histogram().edges)
    a.basemap_histogram(K.ERR_UNWEIGHTED, R.pixel_histogram().edges)
    R.residual_report(a)
    state1, after = same_state(a), stepped(a)
    for s0, s1 in zip(state0, state1):
        for u, v in zip(s0, s1):
            assert np.array_equal(u, v)
    assert before[0][0] == after[0][0] and before[2] == after[2]
    for u, v in zip(before[3], after[3]):
        assert np.array_equal(u, v)
    assert abs(before[1] - after[1]) <= 1e-12 * abs(after[1])
    # and a following one_step is the oracle's
    assert_step_parity(one_step(a), oracle_one_step("frozen", "miniB")[1])
    a.close()


# ---------------------------------------------------------------- 6. point covariances
def test_point_covariances_with_basemap_rows():
    """3 x 3 marginals of 50 points with base-map rows on the frozen scene of A, at the linearization point:
    the engine on P1 against the engine on P2 and against the oracle on P2 (bound: tests/test_point_covariances.py)"""
    p1, p2, _ = bs.scene_pair("frozen", "A")
    with_rows = np.unique(p1.basemap.point[p1.const[0][p1.basemap.point] == 0])
    pts = with_rows[:: max(1, len(with_rows) // 50)][:50]
    assert len(pts) == 50
    g1, g2, r = bs.load(hip(), p1), bs.load(hip(), p2), bs.load(RefEngine, p2)
    c1, u1 = g1.compute_point_covariances(pts)
    c2, u2 = g2.compute_point_covariances(pts)
    cr, ur = r.compute_point_covariances(pts)
    assert u1 == u2 == ur
    e12 = max(rel(a, b) for a, b in zip(c1, c2))
    e1r = max(rel(a, b) for a, b in zip(c1, cr))
    print(f"[basemap] point covariances, 50 points: P1 vs engine P2 {e12:.2e}, P1 vs oracle P2 {e1r:.2e}")
    assert e12 < 1e-7 and e1r < 1e-7
    g1.close(), g2.close()


# ---------------------------------------------------------------- 7. the mixed build
def test_mixed_build_step_tolerance():
    """miniB frozen scene on libviba_hip_mixed.so against the fp64 oracle, within the figures of
    test_mixed_precision_step_tolerance: cost0 1e-10, CostStats exact, gradient 1e-6, step 1e-3"""
    p1 = bs.scene_pair("frozen", "miniB")[0]
    orf = oracle_one_step("frozen", "miniB")[1]
    g = bs.load(hip(), p1, precision="mixed")
    og = one_step(g)
    fig = figures(og, orf)
    show("frozen miniB mixed vs fp64 oracle", fig)
    assert abs(og["cost0"] - orf["cost0"]) <= 1e-10 * orf["cost0"]
    assert tuple(og["stats1"]) == tuple(orf["stats1"])
    assert fig["grad"] < 1e-6 and fig["step"] < 1e-3
    g.close()


# ---------------------------------------------------------------- 8. error paths, the empty case
def test_error_paths():
    p1 = bs.scene_pair("frozen", "A")[0]
    bm = p1.basemap
    new = lambda: hip()(imu_calib_options=p1.imu_calib_options)
    e = new()
    for k in range(K.NUM_VAR_KINDS):
        e.set_vars(k, p1.vars[k], p1.const[k])
    e.add_basemap_factors([], [], np.zeros((0, 6)))  # n == 0 succeeds, even before a base map is set
    # factors before a base map; an index out of range
    assert code_of(lambda: e.add_basemap_factors(bm.point[:1], bm.camera[:1], bm.consts[:1])) == ARG
    assert code_of(lambda: e.set_basemap(T_bodyimu_world=bm.T_bodyimu_world, keyrig_of_camera=[0, 1, 3],
                                         T_cam_bodyimu=bm.T_cam_bodyimu, cams=bm.cams)) == ARG
    e.set_basemap(bm)
    assert code_of(lambda: e.add_basemap_factors([0], [3], bm.consts[:1])) == ARG
    assert code_of(lambda: e.add_basemap_factors([0], [-1], bm.consts[:1])) == ARG
    assert code_of(lambda: e.add_basemap_factors([-1], [0], bm.consts[:1])) == ARG
    e.add_basemap_factors([], [], np.zeros((0, 6)))  # n == 0 succeeds
    assert e.num_basemap_factors() == 0
    rows = [0, 1, 2, 3, 4, 5, bm.num_factors - 1]  # the last row names the third camera
    e.add_basemap_factors(bm.point[rows], bm.camera[rows], bm.consts[rows])
    assert e.num_basemap_factors() == 7 and bm.camera[rows[-1]] == 2
    # a smaller base map under the factors that name its cameras
    assert code_of(lambda: e.set_basemap(T_bodyimu_world=bm.T_bodyimu_world[:1], keyrig_of_camera=[0],
                                         T_cam_bodyimu=bm.T_cam_bodyimu[:1], cams=bm.cams[:1])) == ARG
    e.set_basemap(bm)  # a re-upload (applyWorldTransformation) is fine
    # shards, partitions: not beside base-map factors, in either order
    assert code_of(lambda: e.set_landmark_shard(0, 10, True)) == UNSUPPORTED
    assert code_of(lambda: e.set_partition(0, 2)) == UNSUPPORTED
    sharded = new()
    sharded.set_basemap(bm)
    sharded.set_landmark_shard(0, 10, True)
    assert code_of(lambda: sharded.add_basemap_factors(bm.point[:1], bm.camera[:1], bm.consts[:1])) == UNSUPPORTED
    # the report before vb_finalize
    assert code_of(lambda: e.basemap_errors(0, 1)) == STATE
    assert code_of(lambda: e.basemap_histogram(K.ERR_WEIGHTED, [0.0, 1.0])) == STATE
    for f in range(K.NUM_FACTOR_KINDS):
        if len(p1.fivals[f]):
            e.add_factors(f, p1.fvars[f], p1.fivals[f], p1.fconsts[f])
    e.finalize()
    # after vb_finalize
    assert code_of(lambda: e.set_basemap(bm)) == STATE
    assert code_of(lambda: e.add_basemap_factors(bm.point[:1], bm.camera[:1], bm.consts[:1])) == STATE
    assert code_of(lambda: e.set_deferred(True)) == UNSUPPORTED
    assert not e.spec_prepare()
    assert code_of(lambda: e.basemap_errors(7, 1)) == ARG and code_of(lambda: e.basemap_errors(-1, 1)) == ARG
    assert code_of(lambda: e.basemap_histogram(K.ERR_ROT_DEG, [0.0, 1.0])) == ARG
    assert code_of(lambda: e.basemap_histogram(K.ERR_WEIGHTED, [1.0, 1.0])) == ARG
    assert code_of(lambda: e.basemap_histogram(K.ERR_WEIGHTED, [])) == ARG
    assert len(e.basemap_errors(7, 0)["cost"]) == 0 and len(e.basemap_errors()["cost"]) == 7
    # an unknown point is found at vb_finalize, as a factor's unknown variable handle is
    bad = new()
    for k in range(K.NUM_VAR_KINDS):
        bad.set_vars(k, p1.vars[k], p1.const[k])
    bad.set_basemap(bm)
    bad.add_basemap_factors([len(p1.const[0])], [0], bm.consts[:1])
    assert code_of(bad.finalize) == ARG
    # kind 14 stays rejected: the base map is no factor kind
    assert code_of(lambda: e.factor_errors(14)) == ARG
    for x in (e, sharded, bad):
        x.close()


def test_basemap_without_factors_changes_nothing_and_resources_return():
    """a handle with a base map and zero factors steps exactly as one without (nothing of the base map is
    uploaded or launched: the speculative path stays available), and every device byte, pinned byte, event and
    stream is given back by close()"""
    import gc
    from visual_inertial_bundle_adjustment_amd.engine import live_resources
    gc.collect()  # (engines other tests dropped give their resources back now, not in the middle of this one)
    start = live_resources()
    p = synth.generate(synth.config("A"))
    bm = bs.scene_pair("frozen", "A")[0].basemap
    plain = bs.load(hip(), p)
    e = hip()(imu_calib_options=p.imu_calib_options)
    e.set_basemap(bm)
    e.add_basemap_factors([], [], np.zeros((0, 6)))
    synth.load_into(e, p)
    assert e.num_basemap_factors() == 0 and e.spec_prepare()
    a, b = one_step(e), one_step(plain)
    assert a["stats1"] == b["stats1"] and a["cost0"] == pytest.approx(b["cost0"], rel=1e-13)
    for key in PER_KIND:
        for u, v in zip(a[key], b[key]):
            assert rel(u, v) < 1e-9 if v.size else True, key  # two engines differ by their atomics' order alone
    assert len(e.basemap_errors()["cost"]) == 0
    h = e.basemap_histogram(K.ERR_WEIGHTED, R.weighted_histogram().edges)
    assert h["n_factors"] == 0 and not h["counts"].any()
    assert [s.title for s in R.residual_report(e).sections] == [s.title for s in R.residual_report(plain).sections]
    full = bs.load(hip(), bs.scene_pair("frozen", "A")[0])
    one_step(full), full.refine_points(), full.basemap_errors()
    for x in (e, plain, full):
        x.close()
    assert live_resources() == start
