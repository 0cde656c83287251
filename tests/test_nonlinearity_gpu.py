"""The non-linearity inspection on the device (vb_factor_expected_delta / vb_inspect_nonlinearities /
vb_set_inspect_iteration: visual_expected_kernel of csrc/visual.hip, small_expected_eval_kernel and small_expected_dot_kernel of
csrc/small.hip, the key / selection kernels and the C-ABI of csrc/inspect.hip), for the fp64 and the mixed build.

Main input: synth.config("miniB") after parity_util.make_failing (the residual report's): 24,491 factors over
all 14 kinds, 506 visual factors failing at x0 and 35 more only at x1.  References: the CPU oracle's eval_factor
with Jacobians (tests/nonlinearity_ref.py, whose preconditions tests/test_nonlinearity.py asserts) along the
DEVICE's step, the 50-digit tests/hp_small_factors.py / tests/hp_reference.py on the micro scenes, and the
array-backed selection (nonlinearity.ArraySource) over the device's own per-factor arrays.

Bounds (the project's: tests/test_small_factor_reference*.py, tests/test_visual_reference*.py, fp64 column; the
same for both builds, the evaluators being fp64 in both): v0 1e-10 relative; grad_norm 1e-10 of max(ref, the
largest |g_s| entry); delta 1e-10 (sum_s |step_s| . |g_s|  +  |w| |J| |step| for the kinds with a precision
matrix) -- delta is a cancelling sum, so its bound scales with the sum of magnitudes; on the scenes with an
ill-conditioned precision the relative whitening term 8 m kappa_2 u of test_small_factor_reference.whitening_term
is added; failing rows exactly (-1, 0, 0), rows beyond the loss cutoff exactly delta = grad_norm = 0.  The
selection is compared exactly (order included) with the array-backed one, v1 bit for bit with factor_errors'
cost, the score bit for bit with the numpy expression.

Measured on an MI355X (worst over the factors of a check; the fp64 and the mixed build give the same figures
to the digits shown): against the oracle on miniB v0 2.0e-12, grad_norm 1.0e-12, delta 9.9e-14 of the sum of
magnitudes (worst kind: visual; the small kinds 2.7e-13 and below), along the sub-step the same; against the
50-digit references v0 1.7e-14 on the micro inertial bundle, 5.6e-12 under the kappa_2 = 1e6 covariance (bound
1.6e-8), 3.3e-15 on the pose-prior scenes (rank4_h included), 4.5e-15 with constant and -1 slots, 1.1e-12 on the
visual micro bundle.  Run-to-run spread of two twins' variables after the step 1.3e-12, the inspected engine
against a twin 1.6e-12; the vb_optimize switch against the manual calls 6e-16 in the score.  No bound was
widened and no kernel changed for a figure.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest

import nonlinearity_ref as NR
import small_factor_scenes as sc
import visual_scenes as vs
from test_small_factor_reference import whitening_term
from visual_inertial_bundle_adjustment_amd import kinds as K
from visual_inertial_bundle_adjustment_amd import synth
from visual_inertial_bundle_adjustment_amd.nonlinearity import ArraySource, nonlinearity_score

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp64", "mixed")
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-10
P_KINDS = NR.IMU_KINDS + (K.F_POSE_PRIOR,)
ARG, STATE, RANGE, UNSUPPORTED = -1, -2, -5, -6
VAR_KINDS = range(K.NUM_VAR_KINDS - 1)


def hip():
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    return HipEngine


def show(what, value):
    print(f"[nonlinearity] {what}: {value:.3e}")
    return value


def prepared(precision, p=None):
    """a fresh engine on the main input with one linearization and solve"""
    p = p or NR.problem()
    e = synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p)
    e.linearize(True, False)
    e.damp_factor_solve(NR.LAMBDA)
    return e


@functools.lru_cache(maxsize=None)
def engine(precision):
    """the shared engine of the tests that leave its variables where they are"""
    return prepared(precision)


def expected(e, which=0):
    return {k: e.factor_expected_delta(k, which=which) for k in range(K.NUM_FACTOR_KINDS)}


def steps_of(e, which=0):
    return [e.get_step(k, which) for k in VAR_KINDS]


def compare(got, ref, kinds_with_p, extra=0.0):
    """worst ratios error / bound of one kind's arrays against with_step's output: (v0, grad_norm, delta)"""
    fail = ref["v0"] < 0
    assert np.array_equal(got["v0"] < 0, fail)
    assert np.all(got["v0"][fail] == -1.0) and np.all(got["delta"][fail] == 0.0) and np.all(got["grad_norm"][fail] == 0.0)
    ok = ~fail
    tol = TOL + extra
    w_v0 = np.abs(got["v0"] - ref["v0"])[ok] / np.maximum(tol * np.abs(ref["v0"][ok]), 1e-300)
    w_gn = np.abs(got["grad_norm"] - ref["grad_norm"])[ok] / np.maximum(tol * np.maximum(ref["grad_norm"], ref["g_max"])[ok], 1e-300)
    bound = ref["sum_abs"] + (ref["wjs"] if kinds_with_p else 0.0)
    w_dl = np.abs(got["delta"] - ref["delta"])[ok] / np.maximum(tol * bound[ok], 1e-300)
    zero = ok & (ref["grad_norm"] == 0.0)
    assert np.all(got["delta"][zero] == 0.0) and np.all(got["grad_norm"][zero] == 0.0)
    return tuple(float(w.max(initial=0.0)) for w in (w_v0, w_gn, w_dl))


# ---------------------------------------------------------------- 1. per-factor values against the oracle
@pytest.mark.parametrize("precision", PRECISIONS)
def test_expected_delta_matches_the_oracle(precision):
    """Worst error / bound per quantity is printed; every one must be <= 1."""
    e = engine(precision)
    ref = NR.oracle_x0()[0].with_step(steps_of(e))
    got = expected(e)
    assert int((got[K.F_VISUAL]["v0"] < 0).sum()) == NR.N_FAIL_X0
    worst = np.zeros(3)
    for k in range(K.NUM_FACTOR_KINDS):
        assert len(got[k]["v0"]) == e.num_factors(k) > 0
        w = compare(got[k], ref[k], k in P_KINDS)
        print(f"[nonlinearity] {precision} kind {k}: error / bound v0 {w[0]:.3e} grad_norm {w[1]:.3e} delta {w[2]:.3e}")
        worst = np.maximum(worst, w)
    vis = got[K.F_VISUAL]
    beyond = (vis["v0"] >= 0) & (vis["grad_norm"] == 0)
    assert int(beyond.sum()) > 10000 and np.all(vis["v0"][beyond] == 2.5)  # 0.5 (2 a k - a^2), a = 1, k = 3
    assert np.all(worst <= 1.0), worst


def small_scenes():
    out = [sc.micro_bundle(), sc.whitening_scene()] + list(sc.pose_prior_cases())
    for free, variants in sc.constant_cases():
        out += [free] + list(variants)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scene", small_scenes(), ids=repr)
def test_small_kinds_match_the_50_digit_reference(scene, precision):
    """kinds with a precision matrix, constant and -1 slots: w = rho' P e and g_s = J_s^T w from
    hp_small_factors (grad per argument), the device's own step"""
    import hp_small_factors as hp
    e = scene.build(hip(), precision=precision)
    e.linearize(True, False)
    e.damp_factor_solve(1.0)
    steps = {k: e.get_step(k) for k in scene.vars if k != hp.GRAVITY}
    d = scene.dense()
    extra = whitening_term(scene)
    row = {}
    worst = np.zeros(3)
    for i in scene.factor_order():
        f, handles = d.factors[i]
        r = row.get(f.kind, 0)
        row[f.kind] = r + 1
        ev = f.evaluate()
        delta = sum_abs = g2 = gmax = 0.0
        for b, (vk, h) in enumerate(zip(f.arg_kinds, handles)):
            if h < 0 or ev["grad"][b] is None or d.tdim[vk][h] == 0:
                continue
            g = np.array([float(x) for x in ev["grad"][b]])
            st = steps[vk][h, :len(g)]
            delta += float(st @ g)
            sum_abs += float(np.abs(st) @ np.abs(g))
            g2 += float(g @ g)
            gmax = max(gmax, float(np.abs(g).max()))
        got = e.factor_expected_delta(f.kind, r, 1)
        tol = TOL + extra
        v0 = float(ev["cost"])
        worst = np.maximum(worst, [abs(got["v0"][0] - v0) / max(tol * v0, 1e-300),
                                   abs(got["grad_norm"][0] - np.sqrt(g2)) / max(tol * max(np.sqrt(g2), gmax), 1e-300),
                                   abs(got["delta"][0] - delta) / max(tol * sum_abs, 1e-300)])
        if sum_abs == 0.0:
            assert got["delta"][0] == 0.0
    print(f"[nonlinearity] {precision} {scene!r}: error / bound v0 {worst[0]:.3e} grad_norm {worst[1]:.3e} delta {worst[2]:.3e}"
          f" (whitening term {extra:.2e})")
    assert np.all(worst <= 1.0), worst


@pytest.mark.parametrize("precision", PRECISIONS)
def test_visual_micro_bundle_matches_the_50_digit_reference(precision):
    mb = vs.micro_bundle()
    e = mb.build(hip(), precision=precision)
    e.linearize(True, False)
    e.damp_factor_solve(1.0)
    steps = {k: e.get_step(k) for k in (0, 1, 5, 4)}
    got = e.factor_expected_delta(K.F_VISUAL)
    worst = np.zeros(3)
    n_cut = 0
    for r, f in enumerate(mb.dense().factors):
        assert f.valid
        delta = sum_abs = g2 = gmax = 0.0
        for vk, h, gb in zip((0, 1, 5, 4), mb.obs[r], f.grad):
            g = np.array([float(x) for x in gb])
            st = steps[vk][h, :len(g)]
            delta += float(st @ g)
            sum_abs += float(np.abs(st) @ np.abs(g))
            g2 += float(g @ g)
            gmax = max(gmax, float(np.abs(g).max()))
        v0 = float(f.cost)
        if float(f.drho) == 0.0:
            n_cut += 1
            assert got["delta"][r] == 0.0 and got["grad_norm"][r] == 0.0
        worst = np.maximum(worst, [abs(got["v0"][r] - v0) / (TOL * v0),
                                   abs(got["grad_norm"][r] - np.sqrt(g2)) / max(TOL * max(np.sqrt(g2), gmax), 1e-300),
                                   abs(got["delta"][r] - delta) / max(TOL * sum_abs, 1e-300)])
    assert n_cut == len(mb.CUTOFF) > 0
    print(f"[nonlinearity] {precision} visual micro bundle: error / bound v0 {worst[0]:.3e} grad_norm {worst[1]:.3e} delta {worst[2]:.3e}")
    assert np.all(worst <= 1.0), worst


# ---------------------------------------------------------------- 2. sub-ranges, the sub-step
@pytest.mark.parametrize("precision", PRECISIONS)
def test_expected_delta_sub_ranges(precision):
    """rows [first, first + n) that start and end inside a wave, the last row, an empty range: the rows of
    the full call, bit for bit (the ranges of test_factor_errors_sub_ranges)"""
    e = engine(precision)
    for k, ranges in ((K.F_VISUAL, ((0, 1), (37, 91), (63, 2), (64, 64), (1000, 777), (23966, 1), (23900, 67), (5, 0))),
                      (K.F_IMU, ((3, 70), (0, 1), (65, 5))), (K.F_IMU_SEC_SPLIT, ((1, 1),)), (K.F_RW_CAM_INTR, ((1, 2),)),
                      (K.F_OMEGA_PRIOR, ((10, 100),))):
        full = e.factor_expected_delta(k)
        for first, n in ranges:
            part = e.factor_expected_delta(k, first, n)
            for key, v in part.items():
                assert len(v) == n and np.array_equal(v, full[key][first:first + n]), (k, first, n, key)
    assert len(e.factor_expected_delta(K.F_VISUAL, 23000)["v0"]) == 967


@pytest.mark.parametrize("precision", PRECISIONS)
def test_expected_delta_along_the_sub_step(precision):
    e = prepared(precision)
    e.backup()
    e.apply_step(0)
    e.gradient_dot_step(False)
    e.solve_with_new_gradient()
    e.restore()
    sub = steps_of(e, 1)
    assert any(np.abs(a - b).max(initial=0.0) > 0 for a, b in zip(sub, steps_of(e, 0)))
    ref = NR.oracle_x0()[0].with_step(sub)
    got = expected(e, which=1)
    worst = np.zeros(3)
    for k in range(K.NUM_FACTOR_KINDS):
        worst = np.maximum(worst, compare(got[k], ref[k], k in P_KINDS))
    print(f"[nonlinearity] {precision} sub-step: error / bound v0 {worst[0]:.3e} grad_norm {worst[1]:.3e} delta {worst[2]:.3e}")
    assert np.all(worst <= 1.0), worst


# ---------------------------------------------------------------- 3. / 4. the selection
CASES = ((64, None), (5, None), (1, None), (64, (K.F_VISUAL,)), (5, (K.F_VISUAL,)), (1, (K.F_VISUAL,)))


@functools.lru_cache(maxsize=None)
def inspected(precision):
    """one engine: the per-factor arrays before the step, every selection case (restore in between: the
    variables come back bitwise, test_state_after_inspection), the costs and the variables after the step"""
    e = prepared(precision)
    before, steps = expected(e), steps_of(e)
    results, after, stepped = {}, None, None
    for k, kinds in CASES:
        results[(k, kinds)] = e.inspect_nonlinearities(k=k, kinds=kinds)
        ms = e.inspect_device_ms()
        if after is None:
            after = {q: e.factor_errors(q) for q in range(K.NUM_FACTOR_KINDS)}
            stepped = [e.get_vars(q) for q in range(K.NUM_VAR_KINDS)]
        e.restore()
    print(f"[nonlinearity] {precision} device ms of the last call: x0 {ms[0]:.3f} x1 {ms[1]:.3f} selection {ms[2]:.3f}")
    return before, steps, results, after, stepped


@pytest.mark.parametrize("precision", PRECISIONS)
def test_selection_is_exact(precision):
    before, _, results, after, _ = inspected(precision)
    per_kind = {k: dict(v0=before[k]["v0"], delta=before[k]["delta"], grad_norm=before[k]["grad_norm"], v1=after[k]["cost"],
                        valid1=after[k]["valid"]) for k in before}
    src = ArraySource(per_kind)
    for (k, kinds), got in results.items():
        want = src.inspect_nonlinearities(k=k, kinds=kinds)
        assert got["n_compared"] == want["n_compared"] == (NR.N_COMPARED if kinds is None else NR.N_VIS_COMPARED)
        assert len(got["row"]) == k
        assert list(zip(got["kind"], got["row"])) == list(zip(want["kind"], want["row"])), (k, kinds)
        for i, (kind, row) in enumerate(zip(got["kind"], got["row"])):
            for key in ("v0", "delta", "grad_norm"):
                assert got[key][i] == before[kind][key][row], (k, kinds, i, key)
            assert got["v1"][i] == after[kind]["cost"][row] and after[kind]["valid"][row]
        score = nonlinearity_score(got["v0"], got["delta"], got["v1"], got["grad_norm"])
        assert np.array_equal(got["score"], score) and np.array_equal(got["score"], want["score"])
        assert np.all(np.diff(got["score"]) <= 0)
    assert set(results[(64, None)]["kind"]) <= {1, 2, 3}


@pytest.mark.parametrize("precision", PRECISIONS)
def test_selection_against_the_oracle(precision):
    """with s_k the oracle's k-th score (its own e, J at x0, the device's step, v1 from an oracle engine at
    the device's stepped variables): every returned factor scores at least s_k (1 - 1e-8) there, and every
    factor scoring above s_k (1 + 1e-8) is returned; the band itself is empty (asserted on the CPU for the
    oracle's own step, tests/test_nonlinearity.py, and here for this run)"""
    _, steps, results, _, stepped = inspected(precision)
    p = NR.problem()
    x1 = NR.costs_at(p, NR.at_variables(p, stepped))
    per_kind = NR.arrays(NR.oracle_x0()[0].with_step(steps), x1)
    for k, kinds in ((5, None), (64, None), (5, (K.F_VISUAL,))):
        scores = NR.all_scores(per_kind, kinds)
        assert len(scores["score"]) == (NR.N_COMPARED if kinds is None else NR.N_VIS_COMPARED)
        assert NR.band_is_empty(scores, k)
        sk = scores["score"][k - 1]
        oracle = {(int(a), int(b)): s for a, b, s in zip(scores["kind"], scores["row"], scores["score"])}
        got = results[(k, kinds)]
        returned = {(int(a), int(b)) for a, b in zip(got["kind"], got["row"])}
        assert all(oracle[f] >= sk * (1 - NR.BAND) for f in returned), (k, kinds)
        assert all(f in returned for f, s in oracle.items() if s > sk * (1 + NR.BAND)), (k, kinds)


# ---------------------------------------------------------------- 5. state
@pytest.mark.parametrize("precision", PRECISIONS)
def test_expected_delta_leaves_the_lm_state_untouched(precision):
    """the pattern of test_report_leaves_the_lm_state_untouched: ONE linearization and solve; the step is
    applied and undone once before and once after vb_factor_expected_delta of every kind"""
    a = prepared(precision)

    def stepped(x):
        x.backup()
        ratios = x.apply_step(0)
        cost, stats = x.cost(True)
        out = (ratios, cost, stats, [x.get_vars(k) for k in range(K.NUM_VAR_KINDS)])
        x.restore()
        return out

    def same_state(x):
        return ([x.get_step(k) for k in VAR_KINDS], [x.get_gradient(k) for k in VAR_KINDS],
                [x.get_vars(k) for k in range(K.NUM_VAR_KINDS)])

    before, state0 = stepped(a), same_state(a)
    for k in range(K.NUM_FACTOR_KINDS):
        a.factor_expected_delta(k)
        a.factor_expected_delta(k, 0, min(3, a.num_factors(k)))
    state1, after = same_state(a), stepped(a)
    for s0, s1 in zip(state0, state1):
        for u, v in zip(s0, s1):
            assert np.array_equal(u, v)
    assert before[0][0] == after[0][0] and before[2] == after[2]  # largest step ratio, CostStats
    for u, v in zip(before[3], after[3]):
        assert np.array_equal(u, v)
    assert abs(before[1] - after[1]) <= 1e-12 * abs(after[1])
    np.testing.assert_allclose(before[0], after[0], rtol=1e-12)  # the ratio sums are added with atomics


@pytest.mark.parametrize("precision", PRECISIONS)
def test_state_after_inspection(precision):
    """after inspect_nonlinearities the variables are those of backup() + apply_step(0): bitwise on the same
    engine (one step, the box-plus adds nothing atomically), and against a twin that shares nothing but the
    same calls within 1e-9 max(1, |x|) (the step's summation order; the spread of two twins is printed);
    restore() brings the linearization point back bitwise, and optimize runs on"""
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    a, b, c = (prepared(precision) for _ in range(3))
    x0 = [a.get_vars(k) for k in range(K.NUM_VAR_KINDS)]
    a.inspect_nonlinearities(k=5)
    x1 = [a.get_vars(k) for k in range(K.NUM_VAR_KINDS)]
    assert any(not np.array_equal(u, v) for u, v in zip(x0, x1))
    a.restore()
    for u, v in zip(x0, (a.get_vars(k) for k in range(K.NUM_VAR_KINDS))):
        assert np.array_equal(u, v)
    a.backup()
    a.apply_step(0)
    for u, v in zip(x1, (a.get_vars(k) for k in range(K.NUM_VAR_KINDS))):
        assert np.array_equal(u, v)
    a.restore()
    spread = twin = 0.0
    for x in (b, c):
        x.backup()
        x.apply_step(0)
    for k in range(K.NUM_VAR_KINDS):
        vb, vc = b.get_vars(k), c.get_vars(k)
        scale = np.maximum(1.0, np.abs(vb))
        spread = max(spread, float((np.abs(vb - vc) / scale).max(initial=0.0)))
        twin = max(twin, float((np.abs(x1[k] - vb) / scale).max(initial=0.0)))
    show(f"{precision} run-to-run, two twins: variables after the step, / max(1, |x|)", spread)
    show(f"{precision} inspected engine against a twin", twin)
    assert twin <= 1e-9
    s = a.optimize(Settings.default(max_num_iterations=2))
    assert s.num_iterations == 2 and s.final_cost < s.initial_cost


# ---------------------------------------------------------------- 6. the vb_optimize switch
def fresh(precision):
    p = NR.problem()
    return synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_optimize_inspects_its_first_iteration(precision):
    """set_inspect_iteration(1) against linearize(True, False) + damp_factor_solve(settings.damping) +
    inspect_nonlinearities on a twin (what vb_optimize's first iteration queues): the same factors in the
    same order; scores within 1e-8 relative (two linearizations differ by their atomics' order, ~1e-12 on
    the step; the five scores are O(1) sums of O(1) terms)"""
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    s = Settings.default(max_num_iterations=4)
    a, b = fresh(precision), fresh(precision)
    a.set_inspect_iteration(1, 5)
    out = a.optimize(s)
    assert (out.num_iterations, out.initial_cost, out.final_cost, out.num_rescaled) == (0, 0.0, 0.0, 0)
    got = a.inspection_result()
    b.linearize(True, False)
    b.damp_factor_solve(s.damping)
    want = b.inspect_nonlinearities(k=5)
    assert len(got["row"]) == 5 and got["n_compared"] == want["n_compared"]
    assert list(zip(got["kind"], got["row"])) == list(zip(want["kind"], want["row"]))
    worst = show(f"{precision} optimize switch against the manual calls: score, relative",
                 float((np.abs(got["score"] - want["score"]) / want["score"]).max()))
    assert worst <= 1e-8
    again = b.inspection_result()
    for key in got:
        assert np.array_equal(again[key], want[key])


@pytest.mark.parametrize("precision", PRECISIONS)
def test_optimize_inspects_a_later_iteration_and_the_switch_turns_off(precision):
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    s = Settings.default(max_num_iterations=4)
    a, b, c = fresh(precision), fresh(precision), fresh(precision)
    a.set_inspect_iteration(3, 7)
    out = a.optimize(s)
    assert (out.num_iterations, out.initial_cost, out.final_cost) == (0, 0.0, 0.0)
    got = a.inspection_result()
    assert len(got["row"]) == 7 and got["n_compared"] > 20000 and np.all(np.diff(got["score"]) <= 0)
    a.set_inspect_iteration(0)
    a.restore()
    assert a.optimize(s).num_iterations > 0
    # set and cleared before any run: as an engine that never set it
    b.set_inspect_iteration(3, 7)
    b.set_inspect_iteration(0)
    sb, sc_ = b.optimize(s), c.optimize(s)
    assert sb.num_iterations == sc_.num_iterations == 4 and sb.num_rescaled == sc_.num_rescaled
    assert abs(sb.initial_cost - sc_.initial_cost) <= 1e-9 * sc_.initial_cost
    assert abs(sb.final_cost - sc_.final_cost) <= 1e-9 * sc_.final_cost


def test_run_session_trigger_debugging_of_nonlinearities(tmp_path):
    from visual_inertial_bundle_adjustment_amd import adapter
    from visual_inertial_bundle_adjustment_amd.engine import Settings
    from visual_inertial_bundle_adjustment_amd.nonlinearity import format_nonlinearities
    lines = []
    out_dir = tmp_path / "out"
    e, p, summary = adapter.run_session(os.path.join(HERE, "golden", "session_small"), str(out_dir),
                                        optimizer_settings=Settings.default(max_num_iterations=8), log=lines.append,
                                        show_histogram=True, trigger_debugging_of_nonlinearities=2, inspect_k=6)
    assert summary is None
    assert lines[-1] == "Exiting... happy debugging!"
    assert lines[-2].count("Factor: ") == 6 and lines[-2].count("Non-linearity score..: ") == 6
    assert lines[-2] == format_nonlinearities(e.inspection_result())
    assert len([s for s in lines if "-~oOo~-" in s]) == 1  # the histogram before optimize only
    assert not any("[ark] optimize" in s for s in lines)
    assert not out_dir.exists() or not os.listdir(out_dir)


# ---------------------------------------------------------------- 7. error codes
def code_of(fn):
    from visual_inertial_bundle_adjustment_amd.engine import VbError
    with pytest.raises(VbError) as ex:
        fn()
    return ex.value.code


@pytest.mark.parametrize("precision", PRECISIONS)
def test_error_codes(precision):
    e, p = engine(precision), NR.problem()
    n = e.num_factors(K.F_VISUAL)
    assert code_of(lambda: e.factor_expected_delta(14)) == ARG
    assert code_of(lambda: e.factor_expected_delta(-1)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL, n, 1)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL, -1, 1)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_IMU, 0, e.num_factors(K.F_IMU) + 1)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL, which=2)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL, which=-1)) == ARG
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL, which=1)) == STATE  # no sub-step yet
    x0 = e.get_vars(K.VAR_POSE)
    assert code_of(lambda: e.inspect_nonlinearities(k=0)) == ARG
    assert code_of(lambda: e.inspect_nonlinearities(k=K.INSPECT_MAX_K + 1)) == ARG
    assert code_of(lambda: e.inspect_nonlinearities(kinds=())) == ARG
    assert code_of(lambda: e.inspect_nonlinearities(kinds=(14,))) == ARG
    assert code_of(lambda: e.inspect_nonlinearities(which=2)) == ARG
    assert code_of(lambda: e.inspect_nonlinearities(which=1)) == STATE
    assert code_of(lambda: e.set_inspect_iteration(1, 0)) == ARG
    assert code_of(lambda: e.set_inspect_iteration(1, K.INSPECT_MAX_K + 1)) == ARG
    assert np.array_equal(x0, e.get_vars(K.VAR_POSE))  # a refused call takes no step
    # before vb_finalize; finalized, but no step yet
    raw = synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p, finalize=False)
    assert code_of(lambda: raw.factor_expected_delta(K.F_VISUAL)) == STATE
    assert code_of(lambda: raw.inspect_nonlinearities()) == STATE
    assert raw.inspection_result()["n_compared"] == 0 and len(raw.inspection_result()["row"]) == 0
    nostep = fresh(precision)
    assert code_of(lambda: nostep.factor_expected_delta(K.F_IMU)) == STATE
    assert code_of(lambda: nostep.inspect_nonlinearities()) == STATE
    nostep.linearize(True, False)
    assert code_of(lambda: nostep.factor_expected_delta(K.F_IMU)) == STATE
    # a landmark shard, a partitioned rank
    raw.set_landmark_shard(0, 100, True)
    raw.finalize()
    assert code_of(lambda: raw.factor_expected_delta(K.F_VISUAL)) == UNSUPPORTED
    assert code_of(lambda: raw.inspect_nonlinearities()) == UNSUPPORTED
    part = synth.load_into(hip()(imu_calib_options=p.imu_calib_options, precision=precision), p, finalize=False)
    part.set_partition(0, 2)
    part.finalize()
    assert code_of(lambda: part.factor_expected_delta(K.F_IMU)) == UNSUPPORTED
    assert code_of(lambda: part.inspect_nonlinearities()) == UNSUPPORTED


@pytest.mark.parametrize("precision", PRECISIONS)
def test_out_of_range_rolling_shutter_lookup(precision):
    """the 100x readout-time input of the residual report's test.  Its linearization reports the lookups too,
    so the step is taken the way the multi-process controllers do: the deferred linearization queues without
    reading the error word, and damp_factor_solve clears it (an out-of-range factor counts as failing)."""
    import copy
    q = copy.copy(NR.problem())
    q.vars = list(q.vars)
    cams = q.vars[4].copy()
    cams[:, 5] *= 100.0
    q.vars[4] = cams
    e = synth.load_into(hip()(imu_calib_options=q.imu_calib_options, precision=precision), q)
    e.set_deferred(True)
    e.linearize(True, False)
    e.set_deferred(False)
    e.damp_factor_solve(1.0)
    x0 = [e.get_vars(k) for k in range(K.NUM_VAR_KINDS)]
    assert code_of(lambda: e.factor_expected_delta(K.F_VISUAL)) == RANGE
    assert code_of(lambda: e.inspect_nonlinearities()) == RANGE
    for u, v in zip(x0, (e.get_vars(k) for k in range(K.NUM_VAR_KINDS))):
        assert np.array_equal(u, v)  # found at the linearization point: no step taken
    assert len(e.factor_expected_delta(K.F_IMU)["v0"]) == e.num_factors(K.F_IMU)  # and the next call starts clean
