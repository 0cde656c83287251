"""The HIP engine's global-shutter visual factor (visual_lin_kernel, visual_cost_kernel, the landmark
kernels; csrc/device_math.hpp) against the independent 50-digit reference of tests/hp_reference.py,
on the one-factor problems and the micro bundle (tests/visual_scenes.py) that tests/test_visual_reference.py holds the CPU
oracle to.

The engine exposes no per-factor Jacobian, so it is recovered through the gradient rho' J^T e: every
geometric case runs with two measurements whose whitened residuals (0.6, 0.1) and (-0.2, 0.7) are
linearly independent and inside the quadratic zone of the loss, so an error in any single Jacobian
entry changes at least one compared gradient entry.

Bounds, fp64 build: cost 1e-10 relative, gradient 1e-10 of the block's max|ref|, step 1e-8, variables
after the step 1e-12; the z = 2e-6 case adds the conditioning term of its inputs (case_bounds in
test_visual_reference.py).  Mixed build (fp32 Jacobian records): cost 1e-10, gradient 1e-6, step 1e-3.

Measured on an MI355X (worst over the cases): fp64 cost 1.9e-12, gradient 2.0e-12 (z = 2e-6: 8.2e-9 and
8.7e-9, inside its conditioning bound); mixed cost 1.9e-12, gradient 9.8e-8; micro bundle (lambda 1,
cond 1.6e5) fp64 gradient 3.2e-14, step 5.0e-14, variables 5.3e-16; mixed gradient 4.0e-8, step 1.4e-7.
The loss cases run on both builds as well (mixed gradient bound 1e-6).
No mismatch: device_math.hpp agrees with the reference on every case.
"""
from __future__ import annotations

import numpy as np
import pytest

import hp_reference as hp
import visual_scenes as sc
from oracle.refcpu import RefEngine
from test_visual_reference import (_worst, case_bounds, check_engine_against_reference, check_loss,
                                   check_micro_bundle, loss_probe)

pytestmark = pytest.mark.gpu

CASES = sc.geometric_cases()
PRECISIONS = ("fp64", "mixed")
GRAD_REL = {"fp64": None, "mixed": 1e-6}


def hip():
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    return HipEngine


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("case", CASES, ids=repr)
def test_hip_factor_matches_reference(case, precision):
    for target in sc.E_TARGETS:
        consts = case.consts_for(target)
        ref = case.reference(consts)
        assert ref.valid == case.expect_valid
        eng = case.build(hip(), consts, precision=precision)
        if not ref.valid:  # what the oracle reports on the same problem, and no gradient at all
            orc = case.build(RefEngine, consts)
            assert eng.linearize(True, False) == orc.linearize(True, False) == 0.0
            assert eng.cost(False) == orc.cost(False)
            assert eng.cost(True) == orc.cost(True)
            assert all(np.all(eng.get_gradient(k) == 0.0) for k in sc.BLOCK_KINDS)
            continue
        check_engine_against_reference(eng, case, ref, consts, case_bounds(case, ref, consts), f"hip {precision}",
                                       grad_rel=GRAD_REL[precision])
    print(f"worst so far: { {k: f'{v:.1e}' for k, v in _worst.items() if k.startswith('hip')} }")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_constant_arguments_leave_the_other_blocks_unchanged(precision):
    """a constant point, extrinsics or intrinsics: its own gradient is zero (checked per case above) and
    the other blocks are those of the all-free problem, to the gradient bound (a constant point's
    observation takes another kernel path, so not bit for bit)"""
    by_name = {c.name: c for c in CASES}
    consts = by_name["fisheye-free"].consts_for(sc.E_TARGETS[1])
    free = by_name["fisheye-free"].build(hip(), consts, precision=precision)
    free.linearize(True, False)
    tol = 1e-10 if precision == "fp64" else 1e-6
    for name, blk in (("fisheye-const-point", 0), ("fisheye-const-extr", 2), ("fisheye-const-intr", 3)):
        e = by_name[name].build(hip(), consts, precision=precision)
        e.linearize(True, False)
        for b, kind in enumerate(sc.BLOCK_KINDS):
            g, gf = e.get_gradient(kind), free.get_gradient(kind)
            if b == blk:
                assert np.all(g == 0.0)
            else:
                assert np.abs(g - gf).max() <= tol * np.abs(gf).max(), (name, sc.BLOCK_NAMES[b])


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,reproj_loss,s", sc.LOSS_CASES, ids=[c[0] for c in sc.LOSS_CASES])
def test_hip_loss_zones(name, reproj_loss, s, precision):
    case, consts, ref = loss_probe(name, reproj_loss, s)
    check_loss(case.build(hip(), consts, reproj_loss=reproj_loss, precision=precision), name, ref,
               grad_tol=1e-10 if precision == "fp64" else 1e-6)


def test_hip_micro_bundle_fp64():
    check_micro_bundle(sc.micro_bundle().build(hip()), "hip fp64")


def test_hip_micro_bundle_mixed():
    check_micro_bundle(sc.micro_bundle().build(hip(), precision="mixed"), "hip mixed", cost_tol=1e-10, grad_tol=1e-6,
                       step_tol=1e-3, vars_tol=None)
