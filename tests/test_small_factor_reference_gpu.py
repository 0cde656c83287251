"""The HIP engine's 13 non-visual factor kinds (small_kernel and small_assemble_kernel of csrc/small.hip,
boxplus_reduced_kernel of csrc/step.hip, the whitening of csrc/host.hpp and preint_whiten_kernel of
csrc/preint.hip) against the independent 50-digit reference of tests/hp_small_factors.py, on the scenes of
tests/small_factor_scenes.py, for the fp64 and the mixed build.  The checks are those of
tests/test_small_factor_reference.py, which holds the CPU oracle to the same reference: cost (linearize and
the cost pass), the gradient of every variable, the step at lambda 1, the variables after it, and on every
one-factor scene the Hessian entry by entry through the joint covariance of all free variables at damping 1.

Bounds: the fp64 ones of that file (cost 1e-10, gradient 1e-10, step 1e-8, variables 1e-12, joint covariance
1e-7, plus the whitening and series terms computed from the inputs), for BOTH builds: the small factors store
nothing in fp32, so the mixed build is held to the same figures.

Measured on an MI355X (worst over the scenes; the fp64 and the mixed build give the same figures to the
digits shown, as expected of code that stores nothing in fp32): cost 2.0e-14, gradient 3.5e-14 (3.3e-12 with
|corr[0:3]| = 0.9e-5, where the two-term left Jacobian is in use), step 6.4e-12 and joint
covariance 1.9e-11 (the same scenes), variables after the step 9.5e-14; sharp small-angle check (1024 u =
2.3e-13) cost 1.3e-15, translation gradient 9.4e-16; whitening of the kappa_2 = 1e6 covariance cost 2.8e-13,
gradient 1.1e-11 against 1.6e-8; recomputed preintegration (preint_whiten_kernel, kappa_2 1.2e3) cost 7.4e-15,
gradient 9.2e-15; micro bundle (order 164, lambda 1, cond 5.1e4) gradient 3.5e-14, step 2.8e-14, variables
1.8e-15.  No mismatch: small.hip, step.hip, host.hpp and preint.hip agree with the reference on every
scene, so no bound was widened and no kernel changed.
"""
from __future__ import annotations

import pytest

import small_factor_scenes as sc
from test_small_factor_reference import (ONE_FACTOR, ids, report, run_constant_arguments, run_counts, run_loss_zones,
                                         run_micro_bundle, run_one_factor, run_preint_whitening, run_whitening)

pytestmark = pytest.mark.gpu

PRECISIONS = ("fp64", "mixed")


def hip():
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    return HipEngine


def builder(precision):
    return lambda scene: scene.build(hip(), precision=precision)


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name,group", ONE_FACTOR, ids=ids(ONE_FACTOR))
def test_hip_one_factor_matches_reference(name, group, precision):
    run_one_factor(builder(precision), group, f"hip {precision}")
    report(f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_constant_arguments(precision):
    run_constant_arguments(builder(precision), f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_imu_loss_zones(precision):
    run_loss_zones(builder(precision), f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_whitening_of_an_ill_conditioned_covariance(precision):
    run_whitening(builder(precision), f"hip {precision}")
    report(f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_whitening_of_a_recomputed_preintegration(precision):
    run_preint_whitening(hip(), f"hip {precision}", precision=precision)
    report(f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("scene", sc.cases("count_cases"), ids=repr)
def test_hip_factor_counts(scene, precision):
    run_counts(builder(precision), scene, f"hip {precision}")


@pytest.mark.parametrize("precision", PRECISIONS)
def test_hip_micro_inertial_bundle(precision):
    run_micro_bundle(builder(precision), f"hip {precision}")
    report(f"hip {precision}")
