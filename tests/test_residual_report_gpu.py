"""The residual report on the device (vb_factor_errors / vb_error_histogram: visual_report_kernel of csrc/visual.hip,
small_report_kernel of csrc/small.hip, bin_values_kernel and the C-ABI of csrc/report.hip), for the fp64
and the mixed build.

Main input: synth.config("miniB") after parity_util.make_failing: all 14 kinds, rolling shutter, 23,967
visual factors (odd, no multiple of 64) of which the oracle reports 506 failing, one factor of kind 9 and two
of kind 3 (sub-wave launches).  References: the CPU oracle's eval_factor (the functor's raw residual, m == 0
when it fails) for the per-factor values and the histograms, the 50-digit tests/hp_small_factors.py /
tests/hp_reference.py for the weighted norm and the cost of the kinds with a precision matrix.

Bounds (the project's own: tests/test_parity_configs.py, tests/test_small_factor_reference*.py): residual rows
1e-10 max(1, |e_ref|), squared norms and costs 1e-10 relative, `valid`, histogram counts, n_factors and n_failing
exact.  The histogram comparison may skip only factors whose oracle value lies within 1e-9 max(1, edge) of an
edge; on this input there is none (the test asserts 0 skipped).  Both builds get the same bounds: the report
reuses vis_eval<false> / rs_eval<false> and small_eval, which are fp64 in the mixed build too (it rounds only
the stored Jacobian records and Y panels, which the report neither reads nor writes).

Measured on an MI355X (worst over the factors of a check; the fp64 and the mixed build give the same
figures to the digits shown): against the oracle on miniB, residual rows 2.6e-12 of max(1, |e_ref|),
sq_unweighted 2.4e-12, visual cost 8.4e-12, the sum of all costs
against the oracle's cost(False) below one ulp; against the 50-digit reference, sq_weighted and cost 1.7e-14 on
the micro inertial bundle, 2.8e-13 under the kappa_2 = 1e6 covariance, 8.4e-16 on the pose-prior scenes (rank4_h
included), visual micro bundle rows 1.0e-14, norms and cost 1.1e-12; per-group cost sums 3.5e-15 (visual), 8.4e-16
(small kinds); every count, n_factors, n_failing and `valid` equal, no factor skipped.  Run-to-run spread of two
engines that never call the report (the control of the state test): largest step ratio 5.9e-13, cost 9.9e-14.
No bound was widened and no kernel changed for a figure.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import small_factor_scenes as sc
import visual_scenes as vs
from hp_reference import loss as hp_loss
from parity_util import make_failing
from visual_inertial_bundle_adjustment_amd import kinds as K
from visual_inertial_bundle_adjustment_amd import report as R
from visual_inertial_bundle_adjustment_amd import synth

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp64", "mixed")
HERE = os.path.dirname(os.path.abspath(__file__))
IMU_KINDS = (K.F_IMU, K.F_IMU_SEC_COMMON, K.F_IMU_SEC_SPLIT)
REPROJ = (1.0, 3.0)


def hip():
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    return HipEngine


def show(what, value):
    print(f"[residual report] {what}: {value:.3e}")
    return value


@functools.lru_cache(maxsize=None)
def problem():
    p = synth.generate(synth.config("miniB"))
    make_failing(p)
    return p


@functools.lru_cache(maxsize=None)
def oracle():
    """per kind the oracle's raw rows (zero-padded to the C-ABI's row size), valid flags; its cost(False)"""
    from oracle.refcpu import RefEngine
    p = problem()
    ref = synth.load_into(RefEngine(imu_calib_options=p.imu_calib_options), p)
    out = {}
    for k in range(K.NUM_FACTOR_KINDS):
        n = len(p.fivals[k])
        raw, valid = np.zeros((n, K.FACTOR_ERROR_SIZE[k])), np.zeros(n, bool)
        for i in range(n):
            m, e, _ = ref.eval_factor(k, i, with_jac=False)
            raw[i, :m], valid[i] = e, m > 0
        out[k] = (raw, valid)
    return out, ref.cost(False)[0]


@functools.lru_cache(maxsize=None)
def engine(precision):
    p = problem()
    return synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p)


def visual_cost_of(s):
    """0.5 rho(s) of the reprojection loss, in fp64 from the 50-digit loss"""
    return np.array([0.5 * float(hp_loss(float(x), *REPROJ)[0]) for x in s])


# ---------------------------------------------------------------- 1. per-factor values against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_factor_errors_match_the_oracle(precision):
    e = engine(precision)
    ref, ref_cost = oracle()
    assert int((~ref[K.F_VISUAL][1]).sum()) == 506
    total, worst_raw, worst_sq = 0.0, 0.0, 0.0
    for k in range(K.NUM_FACTOR_KINDS):
        raw, valid = ref[k]
        got = e.factor_errors(k)
        assert got["raw"].shape == raw.shape and len(raw) == e.num_factors(k) > 0
        assert np.array_equal(got["valid"], valid)
        scale = np.maximum(1.0, np.linalg.norm(raw, axis=1))
        worst_raw = max(worst_raw, float((np.abs(got["raw"] - raw).max(axis=1) / scale).max()))
        sq = 0.5 * (raw ** 2).sum(axis=1)
        worst_sq = max(worst_sq, float((np.abs(got["sq_unweighted"] - sq) / np.maximum(1.0, sq)).max()))
        assert np.all(got["raw"][~valid] == 0) and np.all(got["cost"][~valid] == 0) and np.all(got["sq_weighted"][~valid] == 0)
        if k == K.F_VISUAL:
            cost = visual_cost_of(2.0 * sq[valid])
            worst_cost = float((np.abs(got["cost"][valid] - cost) / np.maximum(1e-300, cost)).max())
            assert np.array_equal(got["sq_weighted"], got["sq_unweighted"])
        elif k not in IMU_KINDS and k != K.F_POSE_PRIOR:
            # the functor whitens its own return and the loss is trivial: both norms and the cost are 0.5 |e|^2
            assert np.array_equal(got["sq_weighted"], got["sq_unweighted"]) and np.array_equal(got["cost"], got["sq_weighted"])
        total += float(got["cost"].sum())
    show(f"{precision} raw row, / max(1, |e_ref|)", worst_raw)
    show(f"{precision} sq_unweighted, relative", worst_sq)
    show(f"{precision} visual cost, relative", worst_cost)
    worst_total = show(f"{precision} total cost, relative", abs(total - ref_cost) / abs(ref_cost))
    assert worst_raw <= 1e-10 and worst_sq <= 1e-10 and worst_cost <= 1e-10 and worst_total <= 1e-10


@pytest.mark.parametrize("precision", PRECISIONS)
def test_factor_errors_sub_ranges(precision):
    """rows [first, first + n) that start and end inside a wave, the last row, an empty range: the rows of
    the full call, bit for bit"""
    e = engine(precision)
    for k, ranges in ((K.F_VISUAL, ((0, 1), (37, 91), (63, 2), (64, 64), (1000, 777), (23966, 1), (23900, 67), (5, 0))),
                      (K.F_IMU, ((3, 70), (0, 1), (65, 5))), (K.F_IMU_SEC_SPLIT, ((1, 1),)), (K.F_RW_CAM_INTR, ((1, 2),)),
                      (K.F_OMEGA_PRIOR, ((10, 100),))):
        full = e.factor_errors(k)
        for first, n in ranges:
            part = e.factor_errors(k, first, n)
            for key, v in part.items():
                assert len(v) == n and np.array_equal(v, full[key][first:first + n]), (k, first, n, key)
    tail = e.factor_errors(K.F_VISUAL, 23000)
    assert len(tail["cost"]) == 967


# ---------------------------------------------------------------- 2. weighted norm and cost, 50 digits
def small_scenes():
    return [sc.micro_bundle(), sc.whitening_scene()] + list(sc.pose_prior_cases())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scene", small_scenes(), ids=repr)
def test_weighted_norm_and_cost_match_the_reference(scene, precision):
    e = scene.build(hip(), precision=precision)
    dense = scene.dense()
    by_kind = {}
    for i in scene.factor_order():
        by_kind.setdefault(scene.factors[i][0], []).append(dense.factors[i][0].evaluate())
    worst_w, worst_c = 0.0, 0.0
    for k, evs in by_kind.items():
        got = e.factor_errors(k)
        assert len(got["cost"]) == len(evs) and got["valid"].all()
        for row, ev in enumerate(evs):
            sw, cost = float(ev["s"]) / 2, float(ev["cost"])
            worst_w = max(worst_w, abs(got["sq_weighted"][row] - sw) / max(sw, 1e-300))
            worst_c = max(worst_c, abs(got["cost"][row] - cost) / max(cost, 1e-300))
    show(f"{precision} {scene!r} sq_weighted vs 50 digits, relative", worst_w)
    show(f"{precision} {scene!r} cost vs 50 digits, relative", worst_c)
    assert worst_w <= 1e-10 and worst_c <= 1e-10


@pytest.mark.parametrize("precision", PRECISIONS)
def test_visual_micro_bundle_matches_the_reference(precision):
    mb = vs.micro_bundle()
    got = mb.build(hip(), precision=precision).factor_errors(K.F_VISUAL)
    worst_e, worst_c = 0.0, 0.0
    for row, f in enumerate(mb.dense().factors):
        assert f.valid and got["valid"][row]
        e = np.array([float(f.e[0]), float(f.e[1])])
        worst_e = max(worst_e, np.abs(got["raw"][row] - e).max() / max(1.0, np.linalg.norm(e)))
        for key in ("sq_unweighted", "sq_weighted"):
            worst_c = max(worst_c, abs(got[key][row] - float(f.s) / 2) / (float(f.s) / 2))
        worst_c = max(worst_c, abs(got["cost"][row] - float(f.cost)) / float(f.cost))
    show(f"{precision} visual micro bundle raw", worst_e)
    show(f"{precision} visual micro bundle norms and cost, relative", worst_c)
    assert worst_e <= 1e-10 and worst_c <= 1e-10


# ---------------------------------------------------------------- 3. histograms
def check_histogram(got, values, valid, cost, edges, groups, n_groups, what):
    """counts against numpy.searchsorted(side="right") of the oracle's values, exactly; a factor within
    1e-9 max(1, edge) of an edge may be skipped, and none is"""
    edges = np.asarray(edges, float)
    g = np.zeros(len(values), np.int64) if groups is None else np.asarray(groups, np.int64)
    near = np.zeros(len(values), bool)
    for ed in edges:
        near |= valid & (np.abs(values - ed) <= 1e-9 * max(1.0, abs(ed)))
    assert int(near.sum()) == 0, f"{what}: {int(near.sum())} oracle values on an edge"
    want = np.zeros((n_groups, len(edges) + 1), np.int64)
    np.add.at(want, (g[valid], np.searchsorted(edges, values[valid], side="right")), 1)
    assert np.array_equal(got["counts"], want), what
    assert np.array_equal(got["n_factors"], np.bincount(g, minlength=n_groups)), what
    assert np.array_equal(got["n_failing"], np.bincount(g[~valid], minlength=n_groups)), what
    ref = np.bincount(g[valid], weights=cost[valid], minlength=n_groups)
    return float((np.abs(got["cost"] - ref) / np.maximum(1e-300, np.abs(ref))).max()) if len(values) else 0.0


@pytest.mark.parametrize("precision", PRECISIONS)
def test_visual_histograms_match_the_oracle(precision):
    e, p = engine(precision), problem()
    raw, valid = oracle()[0][K.F_VISUAL]
    values = np.sqrt(2.0 * (0.5 * (raw ** 2).sum(axis=1)))
    cost = np.zeros(len(values))
    cost[valid] = visual_cost_of(values[valid] ** 2)
    cams = p.fvars[K.F_VISUAL][:, 3].astype(np.int32)
    n_groups = int(cams.max()) + 2  # one extra, empty group
    assert 2 < n_groups <= K.REPORT_MAX_GROUPS
    worst = 0.0
    for which, hist in ((K.ERR_UNWEIGHTED, R.pixel_histogram()), (K.ERR_WEIGHTED, R.weighted_histogram())):
        got = e.error_histogram(K.F_VISUAL, which, hist.edges)
        worst = max(worst, check_histogram(got, values, valid, cost, hist.edges, None, 1, f"which {which}"))
        assert got["n_factors"][0] == 23967 and got["n_failing"][0] == 506
        got = e.error_histogram(K.F_VISUAL, which, hist.edges, cams, n_groups)
        worst = max(worst, check_histogram(got, values, valid, cost, hist.edges, cams, n_groups, f"which {which} by camera"))
        assert got["n_factors"][-1] == 0 and not got["counts"][-1].any() and got["cost"][-1] == 0.0
        again = e.error_histogram(K.F_VISUAL, which, hist.edges, cams, n_groups)
        assert np.array_equal(again["counts"], got["counts"])  # integer atomics: reproducible
    show(f"{precision} group cost, relative", worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("precision", PRECISIONS)
def test_small_kind_histograms_match_the_oracle(precision):
    e = engine(precision)
    ref = oracle()[0]
    worst = 0.0
    for k in range(1, K.NUM_FACTOR_KINDS):
        raw, valid = ref[k]
        full = e.factor_errors(k)
        n = len(raw)
        groups = (np.arange(n) * 7 % 3).astype(np.int32)
        if k in IMU_KINDS:
            for which, hist in ((K.ERR_ROT_DEG, R.rot_histogram()), (K.ERR_VEL_CM_S, R.vel_histogram()),
                                (K.ERR_POS_CM, R.pos_histogram())):
                values = R.error_values({"raw": raw}, which)
                # the reference's layout (this input's errors are large: mostly its last bin), and the same 25x wider
                for edges in (hist.edges, [25.0 * x for x in hist.edges]):
                    for g, ng in ((None, 1), (groups, 3)):
                        got = e.error_histogram(k, which, edges, g, ng)
                        worst = max(worst, check_histogram(got, values, valid, full["cost"], edges, g, ng, f"kind {k} which {which}"))
        # unweighted: from the oracle's rows; weighted: the device's own per-factor values, pinned to the
        # 50-digit reference above (the oracle has no weighted norm for the kinds with a precision matrix)
        hist = R.weighted_histogram()
        values = np.sqrt(2.0 * (0.5 * (raw ** 2).sum(axis=1)))
        fine = np.concatenate([hist.edges, np.geomspace(1e-6, 50.0, 25)])
        fine = np.unique(fine)[:K.REPORT_MAX_EDGES]
        for edges in (hist.edges, fine):
            near = np.abs(values[:, None] - np.asarray(edges)[None, :]) <= 1e-9 * np.maximum(1.0, np.asarray(edges))[None, :]
            edges = [ed for ed, bad in zip(edges, near.any(axis=0)) if not bad]
            got = e.error_histogram(k, K.ERR_UNWEIGHTED, edges, groups, 3)
            worst = max(worst, check_histogram(got, values, valid, full["cost"], edges, groups, 3, f"kind {k} unweighted"))
        got = e.error_histogram(k, K.ERR_WEIGHTED, hist.edges)
        want = R.ArraySource({k: full}).error_histogram(k, K.ERR_WEIGHTED, hist.edges)
        assert np.array_equal(got["counts"], want["counts"]) and got["n_factors"][0] == n and got["n_failing"][0] == 0
    show(f"{precision} small kinds group cost, relative", worst)
    assert worst <= 1e-10


@pytest.mark.parametrize("precision", PRECISIONS)
def test_a_value_on_an_edge_goes_to_the_upper_bin(precision):
    """a random-walk factor between two identical variables has |e| == 0.0 exactly: bin 1 of edges starting
    at 0, bin 0 of edges starting at 0.1 (Histogram.cpp:18-22, std::upper_bound).  Exactly zero in floating
    point: the intrinsics walk's difference of equal parameters, and the SE3 walk T T^-1 of a pose with the
    identity rotation (a general quaternion's q q^-1 rounds to 1e-16 off the identity, here as anywhere)."""
    e = hip()(precision=precision)
    e.set_vars(K.VAR_CAM_INTR, np.repeat(vs.fisheye_record()[None, :], 2, axis=0))
    e.set_vars(K.VAR_CAM_EXTR, np.repeat(np.array([[0.0, 0.0, 0.0, 1.0, 0.5, -1.0, 2.0]]), 2, axis=0))
    e.add_factors(K.F_RW_CAM_INTR, np.array([[0, 1]], np.int32), None, np.full((1, 17), 3.0))
    e.add_factors(K.F_RW_CAM_EXTR, np.array([[0, 1]], np.int32), None, np.full((1, 6), 3.0))
    e.finalize()
    for kind in (K.F_RW_CAM_INTR, K.F_RW_CAM_EXTR):
        got = e.factor_errors(kind)
        assert np.all(got["raw"] == 0.0) and got["sq_unweighted"][0] == 0.0 and got["cost"][0] == 0.0
        for which in (K.ERR_UNWEIGHTED, K.ERR_WEIGHTED):
            assert e.error_histogram(kind, which, [0.0, 0.3, 0.6])["counts"].tolist() == [[0, 1, 0, 0]]
            assert e.error_histogram(kind, which, [0.1, 0.3, 0.6])["counts"].tolist() == [[1, 0, 0, 0]]


# ---------------------------------------------------------------- 4. the LM state stays as it is
@pytest.mark.parametrize("precision", PRECISIONS)
def test_report_leaves_the_lm_state_untouched(precision):
    """linearize -> damp_factor_solve, then apply_step -> cost(True) with and without every report call in
    between: variables bitwise equal, CostStats exact, cost within 1e-12.

    Two separately linearized engines cannot show this: the linearization and the factorization add with fp64
    atomics (summation order), so two engines that never call the report already differ -- measured
    on miniB: largest step ratio 5.9e-13 relative, printed below as the control.  So the
    two runs share ONE linearization and solve: the step is applied and undone (backup / restore) once before
    and once after the report calls.  Whatever the report changed of the step, the cost cache (the comparable
    cost reads it), the scalar slots or the variables would show as a bit."""
    p = problem()
    a, b, c = (synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p) for _ in range(3))
    for x in (a, b, c):
        x.linearize(True, False)
        x.damp_factor_solve(1e-5)

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
    for k in range(K.NUM_FACTOR_KINDS):
        a.factor_errors(k)
        a.error_histogram(k, K.ERR_WEIGHTED, R.weighted_histogram().edges)
        a.error_histogram(k, K.ERR_UNWEIGHTED, R.pixel_histogram().edges, np.zeros(a.num_factors(k), np.int32), 2)
        if k in IMU_KINDS:
            a.error_histogram(k, K.ERR_ROT_DEG, R.rot_histogram().edges)
    state1, after = same_state(a), stepped(a)
    for s0, s1 in zip(state0, state1):
        for u, v in zip(s0, s1):
            assert np.array_equal(u, v)
    assert before[0][0] == after[0][0] and before[2] == after[2]  # largest step ratio, CostStats
    for u, v in zip(before[3], after[3]):
        assert np.array_equal(u, v)
    assert abs(before[1] - after[1]) <= 1e-12 * abs(after[1])
    np.testing.assert_allclose(before[0], after[0], rtol=1e-12)  # the ratio sums are added with atomics
    # control: two engines, neither calls the report
    rb, rc = stepped(b), stepped(c)
    show(f"{precision} run-to-run, no report: largest step ratio, relative", abs(rb[0][0] - rc[0][0]) / rc[0][0])
    show(f"{precision} run-to-run, no report: cost, relative", abs(rb[1] - rc[1]) / rc[1])
    assert rb[2] == rc[2] == after[2]


# ---------------------------------------------------------------- 5. error codes
def code_of(fn):
    from visual_inertial_bundle_adjustment_amd.engine import VbError
    with pytest.raises(VbError) as ex:
        fn()
    return ex.value.code


@pytest.mark.parametrize("precision", PRECISIONS)
def test_error_codes(precision):
    e, p = engine(precision), problem()
    edges = R.weighted_histogram().edges
    n = e.num_factors(K.F_VISUAL)
    ARG, STATE, RANGE, UNSUPPORTED = -1, -2, -5, -6
    assert code_of(lambda: e.factor_errors(14)) == ARG
    assert code_of(lambda: e.factor_errors(-1)) == ARG
    assert code_of(lambda: e.factor_errors(K.F_VISUAL, n, 1)) == ARG
    assert code_of(lambda: e.factor_errors(K.F_VISUAL, -1, 1)) == ARG
    assert code_of(lambda: e.error_histogram(14, K.ERR_WEIGHTED, edges)) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, 5, edges)) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, -1, edges)) == ARG
    for which in (K.ERR_ROT_DEG, K.ERR_VEL_CM_S, K.ERR_POS_CM):
        assert code_of(lambda: e.error_histogram(K.F_VISUAL, which, edges)) == ARG
        assert code_of(lambda: e.error_histogram(K.F_OMEGA_PRIOR, which, edges)) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, [0.0, 1.0, 1.0])) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, [0.0, 2.0, 1.0])) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, [0.0, np.nan])) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, [])) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, np.arange(K.REPORT_MAX_EDGES + 1.0))) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges, None, K.REPORT_MAX_GROUPS + 1)) == ARG
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges, None, 0)) == ARG
    g = np.zeros(n, np.int32)
    g[n // 2] = 2
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges, g, 2)) == ARG
    g[n // 2] = -1
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges, g, 2)) == ARG
    # the caps themselves are accepted
    top = e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, np.arange(K.REPORT_MAX_EDGES) * 0.1, np.arange(n, dtype=np.int32) % 64,
                            K.REPORT_MAX_GROUPS)
    assert top["counts"].shape == (64, 33) and top["n_factors"].sum() == n and top["counts"].sum() == n - 506
    # before vb_finalize
    raw = synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p, finalize=False)
    assert code_of(lambda: raw.factor_errors(K.F_VISUAL)) == STATE
    assert code_of(lambda: raw.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges)) == STATE
    # a landmark shard, a partitioned rank
    raw.set_landmark_shard(0, 100, True)
    raw.finalize()
    assert code_of(lambda: raw.factor_errors(K.F_VISUAL)) == UNSUPPORTED
    assert code_of(lambda: raw.error_histogram(K.F_IMU, K.ERR_WEIGHTED, edges)) == UNSUPPORTED
    part = synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p, finalize=False)
    part.set_partition(0, 2)
    part.finalize()
    assert code_of(lambda: part.factor_errors(K.F_IMU)) == UNSUPPORTED
    assert code_of(lambda: part.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, edges)) == UNSUPPORTED


@pytest.mark.parametrize("precision", PRECISIONS)
def test_out_of_range_rolling_shutter_lookup(precision):
    import copy
    q = copy.copy(problem())
    q.vars = list(q.vars)
    cams = q.vars[4].copy()
    cams[:, 5] *= 100.0  # 100x readout time: rows map far outside the tables (tests/test_parity_gpu.py)
    q.vars[4] = cams
    e = synth.load_into(hip()(imu_calib_options=q.imu_calib_options, precision=precision), q)
    assert code_of(lambda: e.factor_errors(K.F_VISUAL)) == -5
    assert code_of(lambda: e.error_histogram(K.F_VISUAL, K.ERR_WEIGHTED, R.weighted_histogram().edges)) == -5
    assert len(e.factor_errors(K.F_IMU)["cost"]) == e.num_factors(K.F_IMU)  # and the next call starts clean


# ---------------------------------------------------------------- 6. run_session(show_histogram=True)
def test_run_session_logs_two_reports():
    from visual_inertial_bundle_adjustment_amd import adapter
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    lines = []
    e, p, summary = adapter.run_session(os.path.join(HERE, "golden", "session_small"), None,
                                        optimizer_settings=Settings.default(max_num_iterations=8), log=lines.append,
                                        show_histogram=True)
    reports = [s for s in lines if "-~oOo~-" in s]
    assert len(reports) == 2
    after = R.residual_report(e)
    assert reports[1] == after.format()
    shown = set()
    for s in after.sections:
        assert s.n_factors == sum(len(p.fivals[k]) for k in s.kinds)
        shown.update(s.kinds)
    assert K.F_VISUAL in shown and K.F_IMU in shown
    # what the reference's report leaves out (the pose prior) or skips for lack of a main store
    rest = sum(float(e.factor_errors(k)["cost"].sum()) for k in range(K.NUM_FACTOR_KINDS)
               if k not in shown and len(p.fivals[k]))
    assert abs(after.total_cost() + rest - summary.final_cost) <= 1e-8 * abs(summary.final_cost)
    quiet = []
    adapter.run_session(os.path.join(HERE, "golden", "session_small"), None,
                        optimizer_settings=Settings.default(max_num_iterations=1), log=quiet.append)
    assert not any("-~oOo~-" in s for s in quiet)
