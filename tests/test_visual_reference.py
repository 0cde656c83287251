"""The CPU oracle's global-shutter visual factor against the independent 50-digit reference
(tests/hp_reference.py): validity, residual, every Jacobian block, the loss, cost and gradient of
one-factor problems, and one assembled and solved micro bundle.

This is how the reference is shown to be right before the HIP engine is held against it
(tests/test_visual_reference_gpu.py); it runs without a GPU.  Outcome: the oracle (ref_factors.hpp) and
the reference agree on every case, so neither needed a fix.  The reference has teeth (checked once by
hand on a scratch copy of the oracle): with the thin-prism coefficients s0 and s1 swapped in
ref_factors.hpp's project(), every valid fisheye case at r >= 2e-3, four loss cases and the micro bundle
fail here (16 tests); with the on-axis limit g = 1 replaced by 1 + k0, fisheye-axis-r0 and fisheye-r5e-9
fail.  (The limit g'(r)/r = 2 (k0 - 1/3) multiplies x^2 <= 1e-16 inside its branch, so its value cannot
show in any result; the limit of g can.)

Bounds (none taken from the oracle's output; rounding unit u = 2^-52):
  residual       64 u |sqrtH| (|uv| + |z|): a handful of operations on pixel-sized numbers
  Jacobian       1e-10 of the block's max|ref| (the project's fp64 gradient figure)
  cost           1e-10 relative;   gradient  1e-10 of the block's max|ref|
  z = 2e-6 case  the result is ill-conditioned in the inputs (d uv / d p_c ~ f / z): the camera-frame
                 point composed from stored doubles is off by delta_p = 8 u (|X| + |t_bw| + |t_cb|), so the
                 residual bound gains b_e = |d e / d p_c| delta_p, the cost |e| b_e and a gradient block
                 2 max|J| b_e; nothing else is added (the Jacobian stays at 1e-10)
  micro bundle   step 1e-8, variables after the step 1e-12, at a damping chosen so that
                 cond(H) 64 u < 1e-8 on the reference's own matrix
Measured here: residual <= 5.3e-13 (2.8e-9 at z = 2e-6, bound 1.5e-8), Jacobian <= 2.1e-15
(5.1e-11 at z = 2e-6), cost <= 1.4e-12, gradient <= 2.1e-12 (z = 2e-6: cost off by 1.6e-9 against a bound
of 2.2e-7, gradient blocks by 0.40 against 89, both from the one conditioning term), micro bundle gradient 3.6e-14, step 4.5e-14,
variables 5.3e-16.
"""
from __future__ import annotations

import numpy as np
import pytest

import hp_reference as hp
import visual_scenes as sc
from oracle.refcpu import RefEngine

U = sc.EPS
CASES = sc.geometric_cases()
_worst = {}


def _note(key, v):
    _worst[key] = max(_worst.get(key, 0.0), float(v))


def case_bounds(case, ref, consts):
    """(residual bound, relative Jacobian bound, cost bound, per-block gradient bounds) of one valid
    probe, from the reference's own numbers"""
    S = np.abs(consts[2:6]).max()
    uv = hp.to_float(hp.projection(case.args(consts)))
    e_tol = 64 * U * 2 * S * (np.abs(uv).max() + np.abs(consts[:2]).max())
    j_rel = 1e-10
    e = hp.to_float(ref.e)
    cost = float(ref.cost)
    Jmax = [np.abs(hp.to_float(Jb)).max() for Jb in ref.J]
    gmax = [np.abs(hp.to_float(g)).max() for g in ref.grad]
    cost_tol = 1e-10 * cost
    g_tol = [1e-10 * g for g in gmax]
    if case.illcond:
        dp, _ = case.conditioning()
        b_e = np.linalg.norm(hp.to_float(ref.J[0]), 2) * dp  # |J_point|_2 = |d e / d p_c|_2 (rotations)
        e_tol += b_e
        cost_tol += np.linalg.norm(e) * b_e + 0.5 * b_e * b_e  # d cost = e . d e
        g_tol = [g + jm * 2 * b_e for g, jm in zip(g_tol, Jmax)]  # d (J^T e) through d e: two residual rows
    return e_tol, j_rel, cost_tol, g_tol


def check_engine_against_reference(engine, case, ref, consts, bounds, tag, grad_rel=None):
    """linearize cost, cost(False) and the gradient blocks of a one-factor problem against the reference;
    grad_rel overrides the per-block gradient bound by a relative one (the mixed build)"""
    _, _, cost_tol, g_tol = bounds
    tag += " (z=2e-6)" if case.illcond else ""
    c_lin = engine.linearize(True, False)
    c_pass, stats = engine.cost(False)
    assert tuple(stats) == (1, 0, 0), (case, stats)
    for c in (c_lin, c_pass):
        _note(f"{tag} cost", abs(c - float(ref.cost)) / float(ref.cost))
        assert abs(c - float(ref.cost)) <= cost_tol, (case, c, float(ref.cost))
    for b, kind in enumerate(sc.BLOCK_KINDS):
        g = engine.get_gradient(kind)
        assert g.shape[0] == 1
        td = ref.tdims[b]
        gr = hp.to_float(ref.grad[b])
        if b == 3:  # camera: the columns of the readout time / time offset and those beyond the tangent
            n = int(case.cam[1])
            assert np.all(g[0, n:] == 0.0), (case, g)
            assert np.all(gr[n:] == 0.0)
        if case.const[b]:
            assert np.all(g == 0.0), (case, sc.BLOCK_NAMES[b], g)
            continue
        tol = g_tol[b] if grad_rel is None else max(g_tol[b], grad_rel * np.abs(gr).max())
        d = np.abs(g[0, :td] - gr).max()
        _note(f"{tag} gradient", d / np.abs(gr).max())
        assert d <= tol, (case, sc.BLOCK_NAMES[b], g[0, :td], gr)


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_oracle_factor_matches_reference(case):
    for probe, target in enumerate(sc.E_TARGETS):
        consts = case.consts_for(target)
        ref = case.reference(consts)
        assert ref.valid == case.expect_valid
        eng = case.build(RefEngine, consts)
        m, e, J = eng.eval_factor(0, 0)
        if not ref.valid:
            assert m == 0
            assert eng.linearize(True, False) == 0.0
            assert all(np.all(eng.get_gradient(k) == 0.0) for k in sc.BLOCK_KINDS)
            assert eng.cost(False) == (0.0, (1, 1, 1))  # invalid now, and invalid in the cache
            continue
        assert m == 2
        bounds = case_bounds(case, ref, consts)
        e_tol, j_rel = bounds[:2]
        er = hp.to_float(ref.e)
        assert np.abs(er - target).max() < 1e-6 or case.illcond  # the probe sits where it was aimed
        _note("residual" + (" (z=2e-6)" if case.illcond else ""), np.abs(e - er).max())
        assert np.abs(e - er).max() <= e_tol, (case, e, er)
        off = 0
        for b, td in enumerate(ref.tdims):
            Ja = J[off:off + 2 * td].reshape(td, 2).T
            off += 2 * td
            Jr = hp.to_float(ref.J[b])
            d = np.abs(Ja - Jr).max() / np.abs(Jr).max()
            _note("jacobian" + (" (z=2e-6)" if case.illcond else ""), d)
            assert d <= j_rel, (case, sc.BLOCK_NAMES[b], Ja, Jr)
            if b == 3:
                assert td == hp.cam_tangent_dim(case.cam) and np.all(Jr[:, int(case.cam[1]):] == 0.0)
        check_engine_against_reference(eng, case, ref, consts, bounds, "oracle")
    print(f"worst so far: { {k: f'{v:.1e}' for k, v in _worst.items()} }")


def test_constant_arguments_leave_the_other_blocks_unchanged():
    by_name = {c.name: c for c in CASES}
    consts = by_name["fisheye-free"].consts_for(sc.E_TARGETS[0])
    free = by_name["fisheye-free"].build(RefEngine, consts)
    free.linearize(True, False)
    for name, blk in (("fisheye-const-point", 0), ("fisheye-const-extr", 2), ("fisheye-const-intr", 3)):
        e = by_name[name].build(RefEngine, consts)
        e.linearize(True, False)
        for b, kind in enumerate(sc.BLOCK_KINDS):
            if b != blk:
                assert np.array_equal(e.get_gradient(kind), free.get_gradient(kind)), (name, b)


def loss_probe(name, reproj_loss, s):
    """the loss geometry with the measurement placed at whitened |e|^2 = s"""
    case = sc.loss_case_geometry()
    r = np.sqrt(s)
    consts = case.consts_for((0.8 * r, -0.6 * r))
    ref = case.reference(consts, reproj_loss)
    assert abs(float(ref.s) - s) < 1e-9 * s
    return case, consts, ref


def check_loss(engine, name, ref, grad_tol=1e-10):
    c_lin = engine.linearize(True, False)
    c_pass, _ = engine.cost(False)
    for c in (c_lin, c_pass):
        assert abs(c - float(ref.cost)) <= 1e-10 * float(ref.cost), (name, c, float(ref.cost))
    for b, kind in enumerate(sc.BLOCK_KINDS):
        g = engine.get_gradient(kind)[0, :ref.tdims[b]]
        gr = hp.to_float(ref.grad[b])
        if name.startswith("cutoff"):
            assert np.all(g == 0.0) and np.all(gr == 0.0)
        else:
            assert np.abs(g - gr).max() <= grad_tol * np.abs(gr).max(), (name, sc.BLOCK_NAMES[b])


@pytest.mark.parametrize("name,reproj_loss,s", sc.LOSS_CASES, ids=[c[0] for c in sc.LOSS_CASES])
def test_oracle_loss_zones(name, reproj_loss, s):
    case, consts, ref = loss_probe(name, reproj_loss, s)
    a, k = reproj_loss
    if name.startswith("cutoff"):
        assert float(ref.cost) == pytest.approx(0.5 * (2 * a * k - a * a), rel=1e-15) and ref.drho == 0
    elif name.startswith("huber"):
        assert 0 < float(ref.drho) < 1
    else:
        assert ref.drho == 1 and float(ref.cost) == pytest.approx(0.5 * s, rel=1e-9)
    check_loss(case.build(RefEngine, consts, reproj_loss=reproj_loss), name, ref)


# ------------------------------------------------------------------ micro bundle
STEP_TOL, VARS_TOL = 1e-8, 1e-12


def check_micro_bundle(engine, tag, cost_tol=1e-10, grad_tol=1e-10, step_tol=STEP_TOL, vars_tol=VARS_TOL):
    mb = sc.micro_bundle()
    d = mb.dense()
    assert len(mb.obs) >= 32 and np.bincount(mb.obs[:, 0]).min() >= 4
    zones = [float(f.drho) for f in d.factors]
    assert all(0 < zones[j] < 1 for j in mb.HUBER) and all(zones[j] == 0 for j in mb.CUTOFF)
    assert sum(z == 1 for z in zones) == len(zones) - 3
    lam, cond = mb.pick_lambda(STEP_TOL)
    print(f"micro bundle: {len(mb.obs)} observations, order {d.n}, lambda {lam:g}, cond {cond:.3g}")
    assert cond * sc.EPS * 64 < STEP_TOL  # on the reference alone: a mismatch is not conditioning
    step = d.step(lam)
    cost = engine.linearize(True, False)
    assert abs(cost - float(d.cost)) <= cost_tol * float(d.cost)
    engine.damp_factor_solve(lam)
    worst = {"gradient": 0.0, "step": 0.0, "vars1": 0.0}
    for b, kind in enumerate(sc.BLOCK_KINDS):
        for what, got, want, tol in (("gradient", engine.get_gradient(kind), d.split(d.g, b), grad_tol),
                                     ("step", engine.get_step(kind), d.split(step, b), step_tol)):
            err = np.abs(got - want).max() / np.abs(want).max()
            worst[what] = max(worst[what], err)
            assert err < tol, (what, sc.BLOCK_NAMES[b], err)
    engine.apply_step(0)
    after = d.vars_after(step)
    if vars_tol is not None:
        for b, kind in enumerate(sc.BLOCK_KINDS):
            err = np.abs(engine.get_vars(kind) - after[b]).max() / np.abs(after[b]).max()
            worst["vars1"] = max(worst["vars1"], err)
            assert err < vars_tol, ("vars1", sc.BLOCK_NAMES[b], err)
    print(f"{tag} micro bundle vs 50-digit reference: { {k: f'{v:.1e}' for k, v in worst.items()} }")


def test_oracle_micro_bundle():
    check_micro_bundle(sc.micro_bundle().build(RefEngine), "oracle")
