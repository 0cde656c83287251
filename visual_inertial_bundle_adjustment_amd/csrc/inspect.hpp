// Non-linearity inspection (vb_factor_expected_delta / vb_inspect_nonlinearities): what the expected-delta
// kernels of visual.hip / small.hip (beside the factor evaluations) and inspect.hip (score, selection, the C-ABI)
// share.
#pragma once
#include "engine.hpp"

namespace viba {

// rows [first, first + n) of a kind, or (visual kind, posOfRow == nullptr) positions [first, first + n) of
// obCostOrder: singleExpectedDelta (Factor.h:470-540) along the step (stepRed / stepPt) into v0 / delta /
// gnorm at t = item - first
struct InsRows {
  int64_t first = 0, n = 0;
  const double *stepRed = nullptr, *stepPt = nullptr;
  double *v0 = nullptr, *delta = nullptr, *gnorm = nullptr;
};

// the inspection's own staging of the small kinds' evaluation with Jacobians (the layout of Dev::sJ / sE /
// sMeta, engine.hpp), `cap` slots: the last linearization's staging is not touched
struct InsStage {
  double *sJ = nullptr, *sE = nullptr;
  int32_t* sMeta = nullptr;
  int64_t cap = 0;
};

// visual.hip / small.hip
// visual kind; err: bit 1 = a rolling-shutter lookup out of range
void launch_visual_expected(const Dev& d, const int32_t* posOfRow, const InsRows& R, int32_t* err, hipStream_t st);
// small kinds 1..13, R.n <= S.cap
void launch_small_expected(const Dev& d, int fk, const InsRows& R, const InsStage& S, hipStream_t st);

}  // namespace viba
