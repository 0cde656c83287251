// vb_optimize (≙ Optimizer::optimize, Optimizer.cpp:768-1106): the device-queueing half of the
// Levenberg-Marquardt loop -- one queued iteration with its speculative linearization of the next, read by
// the host once -- under the decisions of lm_controller.hpp, and vb_lm_run, the same decisions over a
// caller's primitives.
#include "host.hpp"
#include "lm_controller.hpp"

extern "C" {
// ---- vb_optimize's speculative linearization of the next iteration (SpecState, host.hpp)
// The spare tile store (nTiles x 32 KB: 2.2 GB at config C), ResultCache, gradient and rolling-shutter
// tables of the speculative linearization, allocated at the first vb_optimize that speculates.  Returns
// false when any of it cannot be had: the caller then runs the plain controller (no speculation), as
// before the speculative path existed, instead of failing a problem that fits without it.
bool specPrepare(vb_handle h) {
  if (h->spec) return true;
  const Dev& d = h->fin->d;
  // base-map factors keep one cost cache and no spare one: no speculation (the plain controller takes the
  // same decisions, so the trajectory is the same)
  if (d.bm.n > 0) return false;
  auto s = std::make_unique<SpecState>();
  DevOwner& m = s->mem;
  bool ok = !m.zeroed(&s->tilesAlt, (size_t)d.nTiles * TS * TS) && !m.zeroed(&s->cacheAlt, d.nObs) &&
            !m.zeroed(&s->gRedAlt, (size_t)d.nT * TS) && !h->tune.specFailDebug;
  if (ok && h->prob.rsDevice) {
    const int64_t nRS = h->prob.nRS, ns = h->fin->rsOff[nRS];
    ok = !m.zeroed(&s->rsSAlt, ns * 11) && !m.zeroed(&s->rsIAlt, (ns - nRS) * 9) && !m.zeroed(&s->rsGAlt, (size_t)nRS * 3) &&
         !m.zeroed(&s->rsNAlt, nRS);
  }
  for (auto& row : s->evS)
    for (hipEvent_t& e : row) ok = ok && !m.event(&e);
  ok = ok && !m.event(&s->evCost, hipEventDisableTiming) && !m.stream(&s->stR) && !m.pinned(&s->hostRed, 32);
  // a failure gives back what was had before it, with s (nothing has been swapped into Finalized::d then);
  // once installed the group stays to the handle's end (SpecState, host.hpp)
  if (ok) h->spec = std::move(s);
  else (void)hipGetLastError();
  return ok;
}
// the buffers the speculative work writes instead of Finalized::d's
Dev specDev(vb_handle h) {
  Dev ds = h->fin->d;
  ds.tiles = h->spec->tilesAlt, ds.cacheW = h->spec->cacheAlt, ds.gRed = h->spec->gRedAlt;
  ds.red = h->fin->d.red + 48, ds.err = h->fin->d.err + 4;
  ds.redS = h->fin->d.redS + 64 * 8;  // own stripes: the fused cost pass adds into the handle's (costS)
  if (h->prob.rsDevice) ds.rsS = h->spec->rsSAlt, ds.rsI = h->spec->rsIAlt, ds.rsG = h->spec->rsGAlt, ds.rsN = h->spec->rsNAlt;
  return ds;
}
// ark_vi_ba's preStepCallback (the rolling-shutter rebuild at the accepted variables) and the
// linearization of the next iteration, queued behind this iteration's cost pass; event set p
// With early set, specEarly queued the small factors' evaluation and the clear beside the cost pass.
// rsDone: vb_optimize already cleared the speculative slots and queued the rebuild on stF (evRs), beside
// the cost pass; the main stream only waits for it.
int specEnqueue(vb_handle h, int dontRetry, int p, bool early, bool rsDone, bool fuseCost) {
  Dev ds = specDev(h);
  if (fuseCost) ds.costS = h->fin->d.redS;
  if (!early && !rsDone) {
    HIPCHK(hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->str.st));
    HIPCHK(hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->str.st));
  }
  if (rsDone) {
    HIPCHK(hipStreamWaitEvent(h->str.st, h->str.evRs, 0));
  } else {
    HIPCHK(hipEventRecord(h->spec->evS[p][0], h->str.st));
    if (h->prob.rsDevice) launch_rs_build(ds, h->str.st);
    HIPCHK(hipEventRecord(h->spec->evS[p][1], h->str.st));
  }
  return linearizeBody(h, ds, 1, dontRetry, h->spec->evS[p][2], h->spec->evS[p][3], early);
}
// The part of the speculative linearization that needs only the stepped variables, queued on stZ after
// the box-plus so it runs beside the cost pass (which leaves the HBM and most CUs idle): the small
// factors' evaluation into the staging slots and the clear of the spare tile store and gradient.  The
// staging slots are free there (the iteration's assembly is joined, and vb_gradient_dot_step's
// evaluation forks from the main stream after the speculative linearization's join).
int specEarly(vb_handle h, bool cleared, bool storeCleared) {
  if (!smallHere(h, 0)) return 0;
  const Dev ds = specDev(h);
  if (!cleared) {
    HIPCHK(hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->str.st));
    HIPCHK(hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->str.st));
  }
  HIPCHK(hipEventRecord(h->str.evFork, h->str.st));
  HIPCHK(hipStreamWaitEvent(h->str.stZ, h->str.evFork, 0));
  if (storeCleared && h->run.clearOnF) HIPCHK(hipStreamWaitEvent(h->str.stZ, h->str.evClrDone, 0));
  launch_small_eval(ds, 0, ds.gRed, h->str.stZ);
  // (storeCleared: the factorization queued the clear on stZ already, factorSeqSn)
  return storeCleared ? 0 : clearReduced(h, ds, h->str.stZ);
}
// the step was accepted at full size: the speculative buffers become the handle's
void specCommit(vb_handle h) {
  Dev& d = h->fin->d;
  std::swap(d.tiles, h->spec->tilesAlt);
  std::swap(d.cache, h->spec->cacheAlt);
  d.cacheW = d.cache;
  std::swap(d.gRed, h->spec->gRedAlt);
  if (h->prob.rsDevice) {
    std::swap(d.rsS, h->spec->rsSAlt), std::swap(d.rsI, h->spec->rsIAlt);
    std::swap(d.rsG, h->spec->rsGAlt), std::swap(d.rsN, h->spec->rsNAlt);
  }
  h->fin->tileSet ^= 1;
  launch_spec_commit(d, h->str.st);
}
// the iteration's scalars red[0, n) and error words, read on the readback stream once the cost pass
// (evCost) is done, while whatever was queued behind it runs
int readIterScalars(vb_handle h, double* out, int n) {
  HIPCHK(hipStreamWaitEvent(h->spec->stR, h->spec->evCost, 0));
  HIPCHK(hipMemcpyAsync(h->spec->hostRed, h->fin->d.red, n * sizeof(double), hipMemcpyDeviceToHost, h->spec->stR));
  HIPCHK(hipMemcpyAsync(h->spec->hostRed + 24, h->fin->d.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->spec->stR));
  HIPCHK(hipStreamSynchronize(h->spec->stR));
  std::copy(h->spec->hostRed, h->spec->hostRed + n, out);
  h->prof.done = h->prof.atCost;
  int32_t ee[2];
  std::memcpy(ee, h->spec->hostRed + 24, sizeof(ee));
  return errFromWords(h, ee);
}

// vb_optimize's primitives for lmRun.  Per iteration the linearization, damp + eliminate + factor + solve,
// backup, box-plus and cost pass are queued back to back and the host reads their scalars once.  Unless a
// prestep callback or --recompute-preint needs the host between iterations, the next iteration's
// rolling-shutter rebuild and linearization are queued speculatively behind the cost pass (into second
// buffers, specEnqueue), so the device works while the host decides; they are used when the step is accepted
// at full size, the common case.
struct OptimizeOps {
  vb_handle h;
  int maxIt;  // (no speculation behind the last iteration: its work would only be discarded)
  bool verbose;
  vb_log_cb log;
  vb_prestep_cb pre;
  void* user;
  bool preint, speculate;
  bool specQueued = false;  // the current iteration's rebuild + linearization were queued speculatively
  int specSet = 0;
  bool backedUp = false;  // this iteration's backup was taken: an error restores it (vb_optimize)
  std::chrono::steady_clock::time_point t0;

  int iteration(int it, double damping, int dontRetry, vb_lm_iteration* out) {
    int rc;
    t0 = std::chrono::steady_clock::now();
    backedUp = false;
    if (specQueued) {
      specCommit(h);
    } else {
      // ark_vi_ba's preStepCallback (main_AriaKit_ViBa.cpp:95-101): updateRollingShutterData
      // and, under --recompute-preint, the preintegrations from the IMU streams (InertialFactors.cpp:19-70)
      if ((h->prob.rsDevice || preint) && (rc = rsUpdateAsync(h, h->prob.rsDevice, preint))) return rc;
      if (pre) pre(it, user);
      if ((rc = linearizeEnqueue(h, 1, dontRetry))) return rc;
    }
    // (the iteration before it queued no speculative linearization: inspectNext below)
    if (h->run.inspectIt > 0 && it + 1 == h->run.inspectIt) return inspectIteration(damping);
    // damp + eliminate + factor + solve, backup, box-plus and the cost pass queued back to back; the host
    // reads their scalars (costs, CostStats, model reduction, step ratios) and errors once, after the cost
    // pass: none of them changes what the queued work does
    // no speculative linearization in flight across an inspected iteration (vb_set_inspect_iteration)
    const bool inspectNext = h->run.inspectIt > 0 && it + 2 == h->run.inspectIt;
    const bool specNext = speculate && it + 1 < maxIt && !inspectNext;
    const bool early = specNext && smallHere(h, 0) && h->tune.specEarly;
    h->run.clearWanted = early && h->tune.clearInFactor, h->run.clearQueued = false;
    rc = dampFactorSolveEnqueue(h, damping, false);
    const bool storeCleared = h->run.clearQueued;
    h->run.clearWanted = h->run.clearQueued = false;
    if (rc) return rc;
    if ((rc = vb_backup(h))) return rc;
    backedUp = true;
    if ((rc = applyStepEnqueue(h, 0, 10, 11))) return rc;
    // the next iteration's rolling-shutter rebuild (a few latency-bound waves) on stF beside the cost pass
    // instead of after it on the main stream: the speculative slots are cleared first (the rebuild sets
    // error bits), and the main stream waits for it (evRs) before the linearization -- and so before
    // anything the host queues after its read, e.g. a restore of the variables the rebuild reads
    bool rsSide = false;
    if (specNext && h->prob.rsDevice) {
      const Dev ds = specDev(h);
      const int p = specSet ^ 1;
      if (hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->str.st) != hipSuccess ||
          hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->str.st) != hipSuccess ||
          hipEventRecord(h->str.evStep, h->str.st) != hipSuccess || hipStreamWaitEvent(h->str.stF, h->str.evStep, 0) != hipSuccess ||
          hipEventRecord(h->spec->evS[p][0], h->str.stF) != hipSuccess)
        return fail(VB_E_HIP, "speculative rebuild fork");
      launch_rs_build(ds, h->str.stF);
      if (hipEventRecord(h->spec->evS[p][1], h->str.stF) != hipSuccess || hipEventRecord(h->str.evRs, h->str.stF) != hipSuccess)
        return fail(VB_E_HIP, "speculative rebuild join");
      rsSide = true;
    }
    if (early && (rc = specEarly(h, rsSide, storeCleared))) return rc;
    // the global-shutter part of the cost pass inside the speculative linearization (every observation
    // evaluated there: not under dontRetry)
    const bool fuseCost = specNext && h->tune.costFuse && !dontRetry;
    if ((rc = fuseCost ? costFusedEnqueue(h) : costEnqueue(h, 1, false))) return rc;
    const bool wasSpec = specQueued;
    const int wasSet = specSet;
    specQueued = false;
    if (speculate) {
      if (!fuseCost) {  // (fused: recorded after the speculative visual linearization)
        if (hipEventRecord(h->spec->evCost, h->str.st) != hipSuccess) return fail(VB_E_HIP, "hipEventRecord");
        h->prof.atCost = h->prof.used;
      }
      // the next iteration's rebuild + linearization, assuming this step is accepted at full size
      if (specNext) {
        specSet ^= 1;
        if ((rc = specEnqueue(h, dontRetry, specSet, early, rsSide, fuseCost))) return rc;
        specQueued = true;
      }
    }
    profHarvestPrefix(h, h->prof.done);  // the previous iteration's event times, read while this one runs
    double r[17];
    if ((rc = speculate ? readIterScalars(h, r, 17) : readRedErr(h, r, 17))) return rc;
    if (it == h->run.faultFailIt) return fail(VB_E_NUMERIC, "reduced system Cholesky breakdown (injected)");
    out->prev_cost = r[0], out->model_reduction = 0.5 * r[16];
    if (it == h->run.faultNegModelRedIt) out->model_reduction = -out->model_reduction;  // test fault injection
    const double n = (double)std::max<int64_t>(1, h->fin->nParams);
    out->step_rms_ratio = std::sqrt(r[9] / n);
    costStats(h, r + 1, &out->new_cost, &out->stats);
    if (wasSpec) {
      h->run.times.linearize_ms = elapsed(h->spec->evS[wasSet][2], h->spec->evS[wasSet][3]);
      if (h->prob.rsDevice) h->run.times.rs_update_ms = elapsed(h->spec->evS[wasSet][0], h->spec->evS[wasSet][1]);
    } else {
      h->run.times.linearize_ms = elapsed(h->str.ev[0], h->str.ev[1]);
      if (h->run.rsTimed) h->run.times.rs_update_ms = elapsed(h->str.ev[8], h->str.ev[9]), h->run.rsTimed = false;
    }
    h->run.times.schur_ms = elapsed(h->str.ev[2], h->str.ev[3]);
    h->run.times.factor_ms = elapsed(h->str.ev[3], h->str.ev[4]);
    h->run.times.solve_ms = elapsed(h->str.ev[4], h->str.ev[5]);
    h->run.times.step_ms = elapsed(h->str.ev[10], h->str.ev[11]);
    h->run.times.cost_ms = elapsed(h->str.ev[6], h->str.ev[7]);
    h->run.linearized = false, h->run.factored = true, h->run.haveStep = true;
    return 0;
  }
  // Optimizer.cpp:861-883 (Settings::triggerDebuggingOfNonlinearities): after this iteration's linearization
  // and solve, the inspection in place of backup / applyStep / cost; kInspectStop ends lmRun (vb_optimize
  // turns it into success with a zeroed summary, the reference's `return {}`).  No speculative work is queued.
  int inspectIteration(double damping) {
    int rc;
    if ((rc = dampFactorSolveEnqueue(h, damping, false))) return rc;
    double r[17];
    if ((rc = readRedErr(h, r, 17))) return rc;
    h->run.linearized = false, h->run.factored = true, h->run.haveStep = true;
    if ((rc = inspectRun(h, 0, (1u << 14) - 1, h->run.inspectK))) return rc;
    return kInspectStop;
  }
  int gradient_dot_step(int dontRetry, double* backRed) { return vb_gradient_dot_step(h, dontRetry, backRed); }
  int scale_step(double f) { return vb_scale_step(h, f); }
  int restore() { return vb_restore(h); }
  int apply_step(int which) {
    double ratios[3];
    return vb_apply_step(h, which, ratios);
  }
  int cost(double* cost, vb_cost_stats* stats) { return vb_cost(h, 1, cost, stats); }
  int solve_with_new_gradient() { return vb_solve_with_new_gradient(h); }
  // the speculative linearization assumed the full step stays applied
  int step_outcome(int rejected, int rescaled) {
    if (rejected || rescaled) specQueued = false;
    return 0;
  }
  int iteration_done(int it, double prevCost, double newCost, double damping, int) {
    h->run.times.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (log && verbose) {
      char buf[512];
      snprintf(buf, sizeof(buf),
               "it %d cost %.12g -> %.12g lambda %.3g (t %.2f ms: lin %.2f schur %.2f factor %.2f solve %.2f)", it,
               prevCost, newCost, damping, h->run.times.total_ms, h->run.times.linearize_ms, h->run.times.schur_ms,
               h->run.times.factor_ms, h->run.times.solve_ms);
      log(buf, user);
    }
    return 0;
  }
};

// Optimizer::optimize (Optimizer.cpp:768-1106).  An error after an iteration's backup restores the variables
// of that iteration's linearization point before returning.
int vb_optimize(vb_handle h, const vb_settings* sp, vb_log_cb log, vb_prestep_cb pre, void* user, vb_summary* out) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_optimize before vb_finalize");
  vb_settings s;
  if (sp) s = *sp;
  else vb_default_settings(&s);
  const bool preint = h->prob.recomputePreint && h->fin->pi.n > 0;
  // (no memory for the spare buffers: the plain controller, which needs none)
  const bool speculate = !pre && !preint && !h->prob.sharded && !h->prob.partSet && specPrepare(h);
  OptimizeOps ops{h, s.max_num_iterations, s.verbose != 0, log, pre, user, preint, speculate};
  if (h->run.inspectIt > 0 && h->ins) h->ins->nFound = 0, h->ins->nCompared = 0;
  if (const int rc = viba_lm::lmRun(s, ops, out)) {
    if (rc == kInspectStop) {  // the inspected iteration ended the run: the reference's `return {}`
      if (out) *out = vb_summary{};
      HIPCHK(hipStreamSynchronize(h->str.st));
      return 0;
    }
    if (ops.backedUp && vb_restore(h) == 0) (void)hipStreamSynchronize(h->str.st);
    (void)hipStreamSynchronize(h->str.st);
    return rc;
  }
  // (a speculative linearization left queued by a convergence stop is never committed; its buffers are
  // the spare ones)
  HIPCHK(hipStreamSynchronize(h->str.st));
  return 0;
}

// Optimizer.cpp:834-1097 over the caller's primitives (include/viba_hip.h); no handle, no HIP
int vb_lm_run(const vb_settings* sp, const vb_lm_ops* ops, void* user, vb_summary* out) {
  vb_settings s;
  if (sp) s = *sp;
  else vb_default_settings(&s);
  return viba_lm::lmRunTable(s, ops, user, out);
}

}  // extern "C"
