// The Levenberg-Marquardt decisions of Optimizer::optimize (Optimizer.cpp:834-1097), stated once for the
// package: the accept / reject test, the step-rescaling loop with its sub-step, the dontRetryFailed latch,
// the damping updates, the troubled-sequence bookkeeping and the three stop tests.  Host code only (no HIP,
// no handle): vb_optimize (optimize.hip) supplies the device-queueing primitives, the multi-process
// controllers (distributed.py, through vb_lm_run) the collective ones; tests/cpp/lm_check.cpp drives it with
// scripted ones.  The order of evaluation is the reference's.
#pragma once

#include <algorithm>

#include "../../include/viba_hip.h"

namespace viba_lm {

// Ops: the members of vb_lm_ops (include/viba_hip.h) without `user`.  Every member returns 0 or a VB_E_* code;
// a non-zero code ends the run, is returned unchanged, and no further member is called -- undoing a
// half-applied step is the caller's business.
template <class Ops>
int lmRun(const vb_settings& s, Ops& ops, vb_summary* out) {
  double damping = s.damping;
  int it = 0, lastImpr = 0, lastTroubled = -10;
  double initialCost = 0, finalCost = 0, troubledStartDamping = damping;
  int troubledStart = 0, nTroubled = 0, largestTroubled = 0, nRescaled = 0;
  int dontRetry = 0;
  auto acceptable = [](const vb_cost_stats& st) {
    const double rate = st.num_invalid / (st.num_total + 1.0);
    return rate < 0.03 && (st.num_invalid < st.num_prev_invalid * 2.0 + 50);
  };
  int rc;
  while (true) {
    vb_lm_iteration r;
    if ((rc = ops.iteration(it, damping, dontRetry, &r))) return rc;
    const double prevCost = r.prev_cost, modelRed = r.model_reduction;
    double newCost = r.new_cost;
    vb_cost_stats st = r.stats;
    finalCost = prevCost;
    if (it == 0) initialCost = prevCost;
    if (modelRed < 0) {
      // Optimizer.cpp:835-854: the reference re-linearizes into `hess` at the same point (the caches
      // and the gradient it recomputes are the ones it has) and raises the damping, keeping the old
      // step.  Its re-linearization also overwrites the factor in `hess`, so a later sub-step solve
      // of that iteration runs BaSpaCho's triangular solves on an unfactored matrix; that value is
      // defined by BaSpaCho's storage layout and is not reproduced: here the sub-step uses the
      // factor (tests/test_parity_configs.py forces this branch).
      damping *= s.damping_adjust_on_fail;
    }
    double costRed = prevCost - newCost;
    const double ratioRedToCost = costRed / newCost;
    double ratioRedToExp = costRed / modelRed;
    double applied = 1.0;
    bool okRate = acceptable(st);
    bool rescaled = false;
    if (s.max_step_factor_attempts > 0 && (ratioRedToExp < s.min_relative_cost_reduction || !okRate)) {
      rescaled = true, nRescaled++;
      double backRed;
      if ((rc = ops.gradient_dot_step(dontRetry, &backRed))) return rc;
      double sf = backRed > 0 ? modelRed / (modelRed + backRed) : s.step_factor_decrease;
      for (int i = 0; i < s.max_step_factor_attempts; i++) {
        applied *= sf;
        if ((rc = ops.scale_step(sf)) || (rc = ops.restore())) return rc;
        if ((rc = ops.apply_step(0))) return rc;  // (its ratios are discarded, Optimizer.cpp:927)
        vb_cost_stats stF;
        double costF;
        if ((rc = ops.cost(&costF, &stF))) return rc;
        const double redF = prevCost - newCost;  // Optimizer.cpp:935 (reference uses the full-step cost)
        const double rF = redF / (modelRed * applied);
        if (rF >= s.min_relative_cost_reduction && acceptable(stF)) {
          newCost = costF, st = stF, costRed = redF, ratioRedToExp = rF, okRate = true;
          break;
        }
        if (s.try_sub_step) {
          double br;
          if ((rc = ops.gradient_dot_step(dontRetry, &br))) return rc;
          if ((rc = ops.solve_with_new_gradient())) return rc;
          if ((rc = ops.apply_step(1))) return rc;  // (Optimizer.cpp:972)
          vb_cost_stats stS;
          double costS;
          if ((rc = ops.cost(&costS, &stS))) return rc;
          const double redS = prevCost - costS;
          const double rS = redS / (modelRed * applied);
          if (rS >= s.min_relative_cost_reduction && acceptable(stS)) {
            newCost = costS, st = stS, costRed = redS, ratioRedToExp = rS, okRate = true;
            break;
          }
        }
        dontRetry = 1;
        sf = s.step_factor_decrease;
      }
    }
    // (the variable tolerance reads the full step's ratio, Optimizer.cpp:886, 1017)
    const char* tol = ratioRedToCost < s.relative_cost_tolerance     ? "relative cost"
                      : costRed < s.absolute_cost_tolerance          ? "absolute cost"
                      : r.step_rms_ratio < s.variables_tolerance     ? "variable"
                                                                     : nullptr;
    const bool rejected = newCost > prevCost || !okRate;
    if ((rc = ops.step_outcome(rejected, rescaled))) return rc;
    if (rejected) {
      if (lastTroubled != it - 1) troubledStartDamping = damping, troubledStart = it;
      damping *= s.damping_adjust_on_fail;
      if ((rc = ops.restore())) return rc;
      if (damping > s.damping_max) break;
      lastTroubled = it;
    } else {
      if (lastTroubled == it - 1)
        if (troubledStartDamping < 1e1 && damping > 1e-3) {
          nTroubled++;
          largestTroubled = std::max(largestTroubled, it - troubledStart);
        }
      if (ratioRedToExp >= s.min_relative_cost_reduction && applied > s.min_step_factor_for_good)
        damping = std::max(damping * s.damping_adjust_on_good_step, s.damping_min);
      else
        damping *= s.damping_adjust_on_average_step;
      finalCost = newCost;
    }
    it++;
    if ((rc = ops.iteration_done(it, prevCost, newCost, damping, rescaled))) return rc;
    if (!tol) lastImpr = it;
    if (it >= lastImpr + s.stop_if_no_improvement_for && it >= lastTroubled + s.distance_from_troubled_iteration) break;
    if (it >= s.max_num_iterations) break;
  }
  if (out) {
    out->initial_cost = initialCost, out->final_cost = finalCost;
    out->num_troubled_seqs = nTroubled, out->largest_troubled_seq = largestTroubled, out->num_iterations = it;
    out->num_rescaled = nRescaled;
  }
  return 0;
}

// vb_lm_run: the plain-C table (include/viba_hip.h) as an Ops
struct TableOps {
  const vb_lm_ops* o;
  void* user;
  int iteration(int it, double damping, int dontRetry, vb_lm_iteration* out) {
    return o->iteration(user, it, damping, dontRetry, out);
  }
  int gradient_dot_step(int dontRetry, double* backRed) { return o->gradient_dot_step(user, dontRetry, backRed); }
  int scale_step(double f) { return o->scale_step(user, f); }
  int restore() { return o->restore(user); }
  int apply_step(int which) { return o->apply_step(user, which); }
  int cost(double* cost, vb_cost_stats* stats) { return o->cost(user, cost, stats); }
  int solve_with_new_gradient() { return o->solve_with_new_gradient(user); }
  int step_outcome(int rejected, int rescaled) {
    return o->step_outcome ? o->step_outcome(user, rejected, rescaled) : 0;
  }
  int iteration_done(int it, double prevCost, double newCost, double damping, int rescaled) {
    return o->iteration_done ? o->iteration_done(user, it, prevCost, newCost, damping, rescaled) : 0;
  }
};

inline int lmRunTable(const vb_settings& s, const vb_lm_ops* o, void* user, vb_summary* out) {
  if (!o || !o->iteration || !o->gradient_dot_step || !o->scale_step || !o->restore || !o->apply_step || !o->cost ||
      !o->solve_with_new_gradient)
    return VB_E_ARG;
  TableOps ops{o, user};
  return lmRun(s, ops, out);
}

}  // namespace viba_lm
