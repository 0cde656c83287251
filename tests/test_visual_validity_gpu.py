"""The consumers of a visual residual agree on which observations fail.  The linearization, the cost pass,
the residual report and the expected delta (visual_lin_kernel, visual_cost_kernel, visual_report_kernel,
visual_expected_kernel of csrc/visual.hip) evaluate an observation through one function, vis_obs_eval of
csrc/factor_eval.hpp, each with its own bookkeeping around it; the point refinement, the fifth consumer, has
tests of its own.  On visual_scenes.ValidityScene (200 observations over a global- and a rolling-shutter
camera: a full two-wave block, a full wave and an 8-lane partial wave of the linearization; 24 points behind
their camera) the four must report the same failing observations, compared exactly:

  per observation  valid of the report rows, v0 == -1 of the expected-delta rows: the same set, the one the
                   scene was built with
  as counts        the C-ABI exposes the ResultCache and the cost pass through CostStats alone: the cost
                   pass after the linearization counts the cache's -1 entries (numPrevInvalid) and its own
                   failures (numInvalid); both equal the size of that set, and no rolling-shutter lookup was
                   out of range (the calls would fail with VB_E_RANGE)

Cost values are pinned by tests/test_visual_reference_gpu.py and tests/test_residual_report_gpu.py.
"""
from __future__ import annotations

import numpy as np
import pytest

import visual_scenes as vs
from visual_inertial_bundle_adjustment_amd import kinds as K

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("precision", ("fp64", "mixed"))
def test_visual_consumers_agree_on_the_failing_observations(precision):
    from visual_inertial_bundle_adjustment_amd.engine import HipEngine
    sc = vs.ValidityScene()
    rs = sc.table >= 0
    assert len(sc.obs) == 200 and rs.sum() == 100
    assert (sc.invalid & rs).sum() == 12 and (sc.invalid & ~rs).sum() == 12
    e = sc.build(HipEngine, precision=precision)
    e.linearize(True, False)  # fills the ResultCache
    e.damp_factor_solve(1.0)  # a step for the expected delta; the variables stay where they are
    _, (n_total, n_invalid, n_prev_invalid) = e.cost(False)
    rows = e.factor_errors(K.F_VISUAL)
    exp = e.factor_expected_delta(K.F_VISUAL)
    report_invalid, expected_invalid = ~rows["valid"], exp["v0"] == -1.0
    print(f"[validity] {precision}: report {report_invalid.sum()} expected-delta {expected_invalid.sum()} "
          f"cost pass {n_invalid} of {n_total}, cache {n_prev_invalid}")
    assert np.array_equal(report_invalid, sc.invalid)
    assert np.array_equal(expected_invalid, sc.invalid)
    assert (n_total, n_invalid, n_prev_invalid) == (200, 24, 24)
