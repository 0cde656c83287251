"""The CPU oracle's 13 non-visual factor kinds (inertial primary / secondary-common / secondary-split, omega
prior, four random walks, five priors) against the independent 50-digit reference of
tests/hp_small_factors.py, on the scenes of tests/small_factor_scenes.py: one-factor problems at the branch
edges under two residual placements, the IMU loss zones, the whitening of an ill-conditioned covariance (as
given, and as the preintegration path derives it), constant arguments, the factor-count edges of the
small-factor kernels and one assembled and solved micro inertial bundle.

This is how the reference is shown to be right before the HIP engine is held against it
(tests/test_small_factor_reference_gpu.py); it runs without a GPU.  Outcome: the oracle (ref_factors.hpp) and
the reference agree on every case; neither needed a fix.

Compared per scene (`check_scene`): linearize()'s cost and cost(False); get_gradient of every variable;
damp_factor_solve(1.0) + get_step; apply_step + get_vars of every kind (the box-plus, the IMU calibration's
renormalised non-orthogonality diagonals included).  The Hessian pin of every one-factor scene (constant-
argument and loss scenes included) is compute_covariances of ONE joint block of all free variables at damping
1 against the inverse of the reference's damped Hessian (d (1 + lambda) + lambda, tests/test_covariances.py):
an inverse determines the matrix.  No scene's structure rules that API out, so the two-lambda step pin is not
used.  The count scenes and the micro bundle are pinned through cost, gradient, step and variables.

Bounds (none taken from the code under test; u = 2^-52):
  cost        1e-10 relative;  gradient  1e-10 of the variable's max|ref|;  step 1e-8 of the kind's max|ref|;
  variables after the step 1e-12 of the kind's max|ref|;  joint covariance 1e-7 of max|ref|
  whitening   cost and gradient gain 8 m kappa_2 u relative, m = 9 with kappa_2 of the factor's rvpCov
              (inertial kinds), m = 6 with kappa_2 of H (pose prior with a full-rank H); numpy on the input
              matrix.  The rank-4 H of constrainPositionAndYaw has no finite kappa_2 and gets no term.
  series      the engines follow Sophus: SO3::leftJacobian(w) is I + hat(w) / 2 for |w|^2 < 1e-10, which is
              the spec.  The first neglected term is hat(w)^2 / 6, so column t of the inertial calibration
              Jacobian's rotation rows, dLog Jl(-corr) J_top[:, t], is off by at most
              |dLog| (theta^2 / 6) |J_top[:, t]| with theta = |corr[0:3]|; with |dLog| |Jl^-1 dLog^-1| <= 2
              (rotation errors below 1 rad) the calibration gradient entry t gains
              2 (theta^2 / 6) |J_ref[0:3, t]| |(P e)[0:3]| rho' (at most 1.7e-11 relative to the column).  The
              same series is the V of SE3::exp in the box-plus: a step with |omega|^2 < 1e-10 adds
              (|omega|^2 / 6) |upsilon| to the translation after the step.  The other series (the 1/12 of
              leftJacobianInverse below 1e-10: next term theta^4 / 720 < 2e-23; the three coefficients of the
              SE3 Q block below theta^2 = 1e-4: next terms theta^6 / 362880 and smaller, < 3e-18) are below u
              and add nothing.

  sharp       the SE3 scenes with theta just under 1e-5 also run check_series_coefficient (1024 u on the cost
              and the translation gradient; derivation in its docstring): a wrong second-order coefficient
              of the small-angle branch moves a result by theta^2 / 12 < 1e-11, below the bounds above.

Measured here (oracle, worst over the scenes): cost 2.0e-14, gradient 3.5e-14 (3.3e-12 with
|corr[0:3]| = 0.9e-5, where the two-term left Jacobian is in use), step 6.4e-12, variables 9.5e-14, joint
covariance 1.9e-11 (the last three on the rank-4 pose prior); sharp check cost 1.3e-15, translation gradient
8.4e-16; whitening scene (kappa_2 1e6) cost 3.9e-13, gradient 9.9e-12 against 1.6e-8; recomputed
preintegration (kappa_2 1.2e3) cost 5.6e-15, gradient 8.9e-15; micro bundle (order 164, lambda 1, cond 5.1e4)
gradient 3.8e-14, step 2.9e-14, variables 1.6e-15.

Teeth: each mutation made by hand on a scratch copy of the oracle; failing tests of the 83 of this file:
  two entries of the gyro non-orthogonality order swapped (box-plus and box-minus alike)      21
  dt dropped from the previous-velocity position rows of the inertial Jacobian                24
  sign of the extrinsics term of SecondaryState's composeJacobians flipped                     6
  1/6 for the 1/12 of the small-angle leftJacobianInverse                                      4 (sharp check)
  c[j] for sqrt(c[32 + j]) in the IMU prior                                                    6
  non-orthogonality diagonals left un-renormalised in the calibration box-plus               26
  whitening factor transposed (the oracle weights by P itself, so P = L L^T was replaced by
  L^T L, which is what a transposed square root amounts to)                                  24
"""
from __future__ import annotations

import numpy as np
import pytest

import hp_small_factors as hp
import small_factor_scenes as sc
from oracle.refcpu import RefEngine

U = sc.EPS
COST_TOL, GRAD_TOL, STEP_TOL, VARS_TOL, COV_TOL = 1e-10, 1e-10, 1e-8, 1e-12, 1e-7
LAMBDA = 1.0
INERTIAL = (hp.F_IMU, hp.F_IMU_SEC_COMMON, hp.F_IMU_SEC_SPLIT)
_worst = {}


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.0), float(v))


def report(prefix=""):
    print(f"worst so far: { {k: f'{v:.3e}' for k, v in sorted(_worst.items()) if k.startswith(prefix)} }")


def grouped(scenes):
    """[(base name, [placements])] of a scene list whose names end in /p0, /p1"""
    out = {}
    for s in scenes:
        out.setdefault(s.name.split("/")[0], []).append(s)
    return list(out.items())


def ids(groups):
    return [g[0] for g in groups]


# ------------------------------------------------------------------ additive terms, from the inputs alone
def whitening_term(scene):
    """8 m kappa_2 u of the worst-conditioned precision the scene's factors whiten (relative)"""
    t = 0.0
    for kind, _, c in scene.factors:
        if kind in INERTIAL:
            t = max(t, 8 * 9 * np.linalg.cond(c[218:299].reshape(9, 9)) * U)
        elif kind == hp.F_POSE_PRIOR:
            H = c[7:43].reshape(6, 6)
            if np.linalg.matrix_rank(H) == 6:
                t = max(t, 8 * 6 * np.linalg.cond(H) * U)
    return t


def series_terms(scene):
    """{(IMU_CALIB, handle): absolute gradient term} of the two-term left Jacobian (module docstring)"""
    out = {}
    for f, handles in scene.dense().factors:
        if f.kind not in INERTIAL:
            continue
        corr = hp.to_float(f.correction())
        th2 = float(corr[:3] @ corr[:3])
        if 0.0 < th2 < 1e-10:
            assert th2 / 6 < 1e-9
            ev = f.evaluate()
            J = np.array([[float(ev["J"][0][r, t]) for t in range(f.tdims[0])] for r in range(3)])
            Pe = hp.to_float(list(ev["P"] * ev["e"]))[:3]
            term = 2 * (th2 / 6) * np.linalg.norm(J, axis=0).max() * np.linalg.norm(Pe) * float(ev["drho"])
            key = (hp.IMU_CALIB, handles[0])
            out[key] = out.get(key, 0.0) + term
    return out


# ------------------------------------------------------------------ the checks (shared with the GPU file)
def _close(got, want, rel_tol, what, scene, tag, key, abs_term=0.0):
    got, want = np.asarray(got, float), np.asarray(want, float)
    assert got.shape == want.shape, (scene, what, got.shape, want.shape)
    scale = np.abs(want).max(initial=0.0)
    err = np.abs(got - want).max(initial=0.0)
    if scale == 0.0:
        assert err == 0.0, (scene, what, got)
        return
    _note(f"{tag} {key}", err / scale)
    assert err <= rel_tol * scale + abs_term, (scene, what, err / scale, got, want)


def check_cost_and_gradient(engine, scene, tag, key_suffix="", extra=None):
    d = scene.dense()
    extra = whitening_term(scene) if extra is None else extra
    series = series_terms(scene)
    cost = float(d.cost)
    c_lin = engine.linearize(True, False)
    c_pass = engine.cost(False)[0]
    for c in (c_lin, c_pass):
        _note(f"{tag} cost{key_suffix}", abs(c - cost) / cost)
        assert abs(c - cost) <= (COST_TOL + extra) * cost, (scene, c, cost)
    for k in scene.vars:
        if k == hp.GRAVITY:
            continue
        g, gr = engine.get_gradient(k), d.split(d.g, k)
        assert g.shape == gr.shape
        for h in range(len(gr)):  # per variable: its own max|ref|
            if d.tdim[k][h] == 0:
                assert np.all(g[h] == 0.0), (scene, "constant variable", k, h, g[h])
                continue
            _close(g[h], gr[h], GRAD_TOL + extra, f"gradient kind {k} var {h}", scene, tag, "gradient" + key_suffix,
                   series.get((k, h), 0.0))


def check_step_and_vars(engine, scene, tag):
    """after check_cost_and_gradient on the same engine"""
    d = scene.dense()
    step = d.step(LAMBDA)
    engine.damp_factor_solve(LAMBDA)
    for k in scene.vars:
        if k != hp.GRAVITY:
            _close(engine.get_step(k), d.split(step, k), STEP_TOL, f"step kind {k}", scene, tag, "step")
    engine.apply_step(0)
    after = d.vars_after(step)
    for k in scene.vars:
        if k == hp.GRAVITY:
            assert np.array_equal(engine.get_vars(k), scene.vars[k])
            continue
        term = 0.0
        if k in hp.SE3_KINDS:  # V of SE3::exp is I + hat(omega) / 2 below |omega|^2 = 1e-10
            s = d.split(step, k)
            w2 = (s[:, 3:6] ** 2).sum(axis=1)
            small = w2 < 1e-10
            term = float((w2[small] / 6 * np.linalg.norm(s[small, :3], axis=1)).max(initial=0.0))
        _close(engine.get_vars(k), after[k], VARS_TOL, f"variables kind {k}", scene, tag, "vars", term)


def check_covariance(engine, scene, tag):
    """the Hessian, entry by entry: the joint covariance of every free variable at damping 1 (a fresh engine:
    the call invalidates the LM state)"""
    d = scene.dense()
    (cov,), used = engine.compute_covariances([d.free_vars()], LAMBDA)
    assert used == LAMBDA
    _close(cov, d.covariance(LAMBDA), COV_TOL, "joint covariance", scene, tag, "covariance")


SHARP = 2.0 ** -42  # 1024 u


def check_series_coefficient(engine, scene, tag):
    """The second-order coefficient of the small-angle branch (the 1/12 of leftJacobianInverse below
    theta^2 = 1e-10) changes a result by theta^2 / 12 < 1e-11, below every bound above; the SE3 random walks
    and priors with theta just under the threshold get this sharper check of what the coefficient enters
    most: the translation residual upsilon = Jl^-1(omega) t (through the cost) and the translation columns
    of the gradient.  Bound from the arithmetic alone: the error transform is a product of unit quaternions
    and an O(0.1) translation, off by <= 8 u in the rotation and <= u in the translation; the translation
    residual components are >= 0.005, so they carry <= ~200 u relative, the cost (dominated by them: the
    rotation terms are 1e-7 of it) <= ~500 u, the translation gradient entries w^2 e likewise; 1024 u."""
    d = scene.dense()
    cost = float(d.cost)
    c = engine.linearize(True, False)
    _note(f"{tag} cost (theta < 1e-5)", abs(c - cost) / cost)
    assert abs(c - cost) <= SHARP * cost, (scene, c, cost)
    for k in scene.vars:
        g, gr = engine.get_gradient(k)[:, :3], d.split(d.g, k)[:, :3]
        for h in range(len(gr)):
            _close(g[h], gr[h], SHARP, f"translation gradient kind {k} var {h}", scene, tag, "gradient (theta < 1e-5)")


def check_scene(build, scene, tag, covariance=True):
    """build(scene) -> a fresh engine"""
    e = build(scene)
    check_cost_and_gradient(e, scene, tag)
    check_step_and_vars(e, scene, tag)
    if covariance:
        check_covariance(build(scene), scene, tag)


def assert_placed(scene):
    """the scene sits where it was aimed, judged on the reference alone"""
    d = scene.dense()
    f = d.factors[0][0]
    e = hp.to_float(f.residual())
    assert np.all(e != 0.0), (scene, e)
    t = scene.tags
    if "target" in t:
        assert np.abs(e - t["target"]).max() < 1e-12, (scene, e)
    if "rot_norm" in t:
        assert (float(e[:3] @ e[:3]) < 1e-10) == (t["rot_norm"] < 1e-5)
    if "corr_norm" in t:
        c = hp.to_float(f.correction())
        c2 = float(c[:3] @ c[:3])
        assert c2 == 0.0 if t["corr_norm"] == 0 else (c2 < 1e-10) == (t["corr_norm"] < 1e-5) and c2 > 0
    if "theta" in t:
        w2 = float(e[3:6] @ e[3:6])
        assert abs(np.sqrt(w2) - t["theta"]) < 1e-9 * t["theta"]
        assert (w2 < 1e-10) == (t["theta"] < 1e-5) and (w2 < 1e-4) == (t["theta"] < 1e-2)
    if "tdim" in t:
        assert d.n == t["tdim"] * len(scene.vars[hp.CAM_INTR])


def ref_build(scene):
    return scene.build(RefEngine)


ONE_FACTOR = [(name, group) for which in ("primary_cases", "secondary_cases", "omega_cases", "imu_calib_cases",
                                          "cam_intr_cases", "se3_cases", "pose_prior_cases")
              for name, group in grouped(sc.cases(which))]


def run_one_factor(build, group, tag):
    assert len(group) >= 2  # at least two residual placements
    for scene in group:
        assert len(scene.factors) == 1
        assert_placed(scene)
        check_scene(build, scene, tag)
        if scene.tags.get("theta", 1.0) < 1e-5:
            check_series_coefficient(build(scene), scene, tag)


def run_constant_arguments(build, tag):
    for free, variants in sc.cases("constant_cases"):
        check_scene(build, free, tag)
        df = free.dense()
        assert len(variants) == len(free.factors[0][1]) - 1  # every argument but gravity
        for v in variants:
            k, h = v.tags["const_var"]
            d = v.dense()
            assert d.tdim[k][h] == 0 and d.n == df.n - df.tdim[k][h]
            for kk in v.vars:  # the reference's other blocks are the all-free ones
                if kk != hp.GRAVITY:
                    want = df.split(df.g, kk)
                    if kk == k:
                        want[h] = 0.0
                    assert np.array_equal(d.split(d.g, kk), want)
            check_scene(build, v, tag)  # own block exactly 0, the others to the gradient bound


def run_loss_zones(build, tag):
    for scene, zone in sc.cases("loss_cases"):
        ev = scene.dense().factors[0][0].evaluate()
        a, k = scene.imu_loss
        if zone == "quadratic":
            assert ev["drho"] == 1 and float(ev["cost"]) == pytest.approx(float(ev["s"]) / 2, rel=1e-15)
        elif zone == "linear":
            assert 0 < float(ev["drho"]) < 1 and not np.isfinite(k)
        else:
            assert ev["drho"] == 0 and float(ev["cost"]) == pytest.approx(0.5 * (2 * a * k - a * a), rel=1e-15)
        check_scene(build, scene, tag)


def run_whitening(build, tag):
    scene = sc.cases("whitening_scene")
    kappa = np.linalg.cond(scene.tags["cov_input"])
    assert 0.9e6 < kappa < 1.1e6
    term = whitening_term(scene)
    assert term == 8 * 9 * kappa * U
    check_cost_and_gradient(build(scene), scene, tag, " (kappa 1e6)")
    print(f"{tag} whitening: kappa_2 {kappa:.3g}, additive term {term:.2e}")


def preint_problem():
    """the first primary inertial row of miniB (the stream tests/test_preint.py uses) as a one-factor
    problem whose preintegration is recomputed by the engine"""
    from visual_inertial_bundle_adjustment_amd import synth
    if "preint" not in sc._MEMO:
        p = synth.generate(synth.config("miniB"))
        fv = p.fvars[1][0]
        rows = [p.vars[6][fv[0]], p.vars[1][fv[1]], p.vars[2][fv[2]], p.vars[1][fv[3]], p.vars[2][fv[4]], p.vars[8][fv[5]]]
        # the stream around the interval only: the engines copy it
        t0, t1 = int(p.rs_mid[fv[1]]), int(p.rs_mid[fv[3]])
        keep = (p.imu_t >= (t0 - 20_000) * 1000) & (p.imu_t <= (t1 + 20_000) * 1000)
        sc._MEMO["preint"] = (p.imu_calib_options, rows, p.fconsts[1][0].copy(), (p.imu_t[keep], p.imu_gyro[keep], p.imu_accel[keep]),
                              t0, t1)
    return sc._MEMO["preint"]


def run_preint_whitening(engine_cls, tag, **kw):
    """set_preint_sources -> update_preintegrations; the constants are read back and the reference is formed
    from them: the covariance is input, the whitening derived from it and the factor are under test"""
    mask, rows, consts, stream, t0, t1 = preint_problem()
    # move the next state so that the residual is far from zero in every row
    rows = list(rows)
    rows[3] = sc.moved(rows[3], [2e-3, -1e-3, 1.5e-3, 1e-3, -2e-3, 1.5e-3])
    rows[4] = rows[4] + np.array([3e-3, -2e-3, 1e-3])
    scene = sc.Scene("preint-whitening", {6: [rows[0]], 1: [rows[1], rows[3]], 2: [rows[2], rows[4]], 8: [rows[5]]},
                     [(hp.F_IMU, (0, 0, 0, 1, 1, 0), consts)], mask=mask)
    e = engine_cls(imu_calib_options=mask, **kw)
    for k, v in scene.vars.items():
        e.set_vars(k, v, np.ones(len(v), np.uint8) if k == hp.GRAVITY else None)
    e.set_imu_measurements(*stream)
    e.add_factors(hp.F_IMU, np.array([[0, 0, 0, 1, 1, 0]], np.int32), None, consts[None])
    e.set_preint_sources(hp.F_IMU, [0], [t0], [t1])
    e.finalize()
    e.update_preintegrations()
    got = e.get_factor_consts(hp.F_IMU, 0)
    assert not np.array_equal(got[218:299], consts[218:299])  # recomputed, not the generator's row
    assert np.array_equal(got[299:331], rows[0])              # evaluated at the factor's calibration
    ref = sc.Scene("preint-whitening", scene.vars, [(hp.F_IMU, (0, 0, 0, 1, 1, 0), got)], mask=mask)
    kappa = np.linalg.cond(got[218:299].reshape(9, 9))
    check_cost_and_gradient(e, ref, tag, " (preint)")
    print(f"{tag} preintegration whitening: kappa_2 {kappa:.3g}, additive term {whitening_term(ref):.2e}, "
          f"cost {float(ref.dense().cost):.4g}")


def run_counts(build, scene, tag):
    kinds = {k for k, _, _ in scene.factors}
    assert len(kinds) == 1
    check_scene(build, scene, tag, covariance=False)


def run_micro_bundle(build, tag):
    scene = sc.cases("micro_bundle")
    d = scene.dense()
    kinds = sorted(k for k, _, _ in scene.factors)
    assert kinds == [1, 1, 2, 3, 4, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13]
    assert len(scene.vars[1]) == 3 and hp.POSE not in scene.const
    print(f"micro inertial bundle: {len(scene.factors)} factors, order {d.n}, lambda {LAMBDA:g}, "
          f"cond {d.cond(LAMBDA):.3g}")
    check_scene(build, scene, tag + " micro", covariance=False)


# ------------------------------------------------------------------ the oracle
@pytest.mark.parametrize("name,group", ONE_FACTOR, ids=ids(ONE_FACTOR))
def test_oracle_one_factor_matches_reference(name, group):
    run_one_factor(ref_build, group, "oracle")
    report("oracle")


def test_oracle_constant_arguments():
    run_constant_arguments(ref_build, "oracle")


def test_oracle_imu_loss_zones():
    run_loss_zones(ref_build, "oracle")


def test_oracle_whitening_of_an_ill_conditioned_covariance():
    run_whitening(ref_build, "oracle")
    report("oracle")


def test_oracle_whitening_of_a_recomputed_preintegration():
    run_preint_whitening(RefEngine, "oracle")
    report("oracle")


@pytest.mark.parametrize("scene", sc.cases("count_cases"), ids=repr)
def test_oracle_factor_counts(scene):
    run_counts(ref_build, scene, "oracle")


def test_oracle_micro_inertial_bundle():
    run_micro_bundle(ref_build, "oracle")
    report("oracle")
