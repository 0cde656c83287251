// vb_optimize (≙ Optimizer::optimize, Optimizer.cpp:768-1106): the device-queueing half of the
// Levenberg-Marquardt loop -- one queued iteration with its speculative linearization of the next, read by
// the host once -- under the decisions of lm_controller.hpp, and vb_lm_run, the same decisions over a
// caller's primitives.
#include "host.hpp"
#include "lm_controller.hpp"

extern "C" {
// ---- vb_optimize's speculative linearization of the next iteration (vb_handle_s::tilesAlt ..)
// The spare tile store (nTiles x 32 KB: 2.2 GB at config C), ResultCache, gradient and rolling-shutter
// tables of the speculative linearization, allocated at the first vb_optimize that speculates.  Returns
// false when any of it cannot be had: the caller then runs the plain controller (no speculation), as
// before the speculative path existed, instead of failing a problem that fits without it.
bool specPrepare(vb_handle h) {
  if (h->specReady) return true;
  Dev& d = h->d;
  DevOwner& m = h->spec;
  bool ok = !m.zeroed(&h->tilesAlt, (size_t)d.nTiles * TS * TS) && !m.zeroed(&h->cacheAlt, d.nObs) &&
            !m.zeroed(&h->gRedAlt, (size_t)d.nT * TS) && !h->specFailDebug;
  if (ok && h->rsDevice) {
    const int64_t ns = h->rsOff[h->nRS];
    ok = !m.zeroed(&h->rsSAlt, ns * 11) && !m.zeroed(&h->rsIAlt, (ns - h->nRS) * 9) &&
         !m.zeroed(&h->rsGAlt, (size_t)h->nRS * 3) && !m.zeroed(&h->rsNAlt, h->nRS);
  }
  for (auto& row : h->evS)
    for (hipEvent_t& e : row) ok = ok && !m.event(&e);
  ok = ok && !m.event(&h->evCost, hipEventDisableTiming) && !m.stream(&h->stR) && !m.pinned(&h->hostRed, 32);
  if (!ok) {  // give back what was had before the failure (nothing has been swapped into h->d then)
    m.release();
    h->tilesAlt = h->cacheAlt = h->gRedAlt = h->rsSAlt = h->rsIAlt = h->rsGAlt = h->hostRed = nullptr;
    h->rsNAlt = nullptr, h->evCost = nullptr, h->stR = nullptr;
    for (auto& row : h->evS)
      for (hipEvent_t& e : row) e = nullptr;
    (void)hipGetLastError();
  }
  h->specReady = ok;
  return ok;
}
// the buffers the speculative work writes instead of h->d's
Dev specDev(vb_handle h) {
  Dev ds = h->d;
  ds.tiles = h->tilesAlt, ds.cacheW = h->cacheAlt, ds.gRed = h->gRedAlt;
  ds.red = h->d.red + 48, ds.err = h->d.err + 4;
  ds.redS = h->d.redS + 64 * 8;  // own stripes: the fused cost pass adds into the handle's (costS)
  if (h->rsDevice) ds.rsS = h->rsSAlt, ds.rsI = h->rsIAlt, ds.rsG = h->rsGAlt, ds.rsN = h->rsNAlt;
  return ds;
}
// ark_vi_ba's preStepCallback (the rolling-shutter rebuild at the accepted variables) and the
// linearization of the next iteration, queued behind this iteration's cost pass; event set p
// With early set, specEarly queued the small factors' evaluation and the clear beside the cost pass.
// rsDone: vb_optimize already cleared the speculative slots and queued the rebuild on stF (evRs), beside
// the cost pass; the main stream only waits for it.
int specEnqueue(vb_handle h, int dontRetry, int p, bool early, bool rsDone, bool fuseCost) {
  Dev ds = specDev(h);
  if (fuseCost) ds.costS = h->d.redS;
  if (!early && !rsDone) {
    HIPCHK(hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->st));
    HIPCHK(hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->st));
  }
  if (rsDone) {
    HIPCHK(hipStreamWaitEvent(h->st, h->evRs, 0));
  } else {
    HIPCHK(hipEventRecord(h->evS[p][0], h->st));
    if (h->rsDevice) launch_rs_build(ds, h->st);
    HIPCHK(hipEventRecord(h->evS[p][1], h->st));
  }
  return linearizeBody(h, ds, 1, dontRetry, h->evS[p][2], h->evS[p][3], early);
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
    HIPCHK(hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->st));
    HIPCHK(hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->st));
  }
  HIPCHK(hipEventRecord(h->evFork, h->st));
  HIPCHK(hipStreamWaitEvent(h->stZ, h->evFork, 0));
  if (storeCleared && h->clearOnF) HIPCHK(hipStreamWaitEvent(h->stZ, h->evClrDone, 0));
  launch_small_eval(ds, 0, ds.gRed, h->stZ);
  // (storeCleared: the factorization queued the clear on stZ already, factorSeqSn)
  return storeCleared ? 0 : clearReduced(h, ds, h->stZ);
}
// the step was accepted at full size: the speculative buffers become the handle's
void specCommit(vb_handle h) {
  Dev& d = h->d;
  std::swap(d.tiles, h->tilesAlt);
  std::swap(d.cache, h->cacheAlt);
  d.cacheW = d.cache;
  std::swap(d.gRed, h->gRedAlt);
  if (h->rsDevice) {
    std::swap(d.rsS, h->rsSAlt), std::swap(d.rsI, h->rsIAlt);
    std::swap(d.rsG, h->rsGAlt), std::swap(d.rsN, h->rsNAlt);
  }
  h->tileSet ^= 1;
  launch_spec_commit(d, h->st);
}
// the iteration's scalars red[0, n) and error words, read on the readback stream once the cost pass
// (evCost) is done, while whatever was queued behind it runs
int readIterScalars(vb_handle h, double* out, int n) {
  HIPCHK(hipStreamWaitEvent(h->stR, h->evCost, 0));
  HIPCHK(hipMemcpyAsync(h->hostRed, h->d.red, n * sizeof(double), hipMemcpyDeviceToHost, h->stR));
  HIPCHK(hipMemcpyAsync(h->hostRed + 24, h->d.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->stR));
  HIPCHK(hipStreamSynchronize(h->stR));
  std::copy(h->hostRed, h->hostRed + n, out);
  h->profDone = h->profAtCost;
  int32_t ee[2];
  std::memcpy(ee, h->hostRed + 24, sizeof(ee));
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
      if ((h->rsDevice || preint) && (rc = rsUpdateAsync(h, h->rsDevice, preint))) return rc;
      if (pre) pre(it, user);
      if ((rc = linearizeEnqueue(h, 1, dontRetry))) return rc;
    }
    // damp + eliminate + factor + solve, backup, box-plus and the cost pass queued back to back; the host
    // reads their scalars (costs, CostStats, model reduction, step ratios) and errors once, after the cost
    // pass: none of them changes what the queued work does
    const bool specNext = speculate && it + 1 < maxIt;
    const bool early = specNext && smallHere(h, 0) && h->specEarly;
    h->clearWanted = early && h->clearInFactor, h->clearQueued = false;
    rc = dampFactorSolveEnqueue(h, damping, false);
    const bool storeCleared = h->clearQueued;
    h->clearWanted = h->clearQueued = false;
    if (rc) return rc;
    if ((rc = vb_backup(h))) return rc;
    backedUp = true;
    if ((rc = applyStepEnqueue(h, 0, 10, 11))) return rc;
    // the next iteration's rolling-shutter rebuild (a few latency-bound waves) on stF beside the cost pass
    // instead of after it on the main stream: the speculative slots are cleared first (the rebuild sets
    // error bits), and the main stream waits for it (evRs) before the linearization -- and so before
    // anything the host queues after its read, e.g. a restore of the variables the rebuild reads
    bool rsSide = false;
    if (specNext && h->rsDevice) {
      const Dev ds = specDev(h);
      const int p = specSet ^ 1;
      if (hipMemsetAsync(ds.red, 0, 16 * sizeof(double), h->st) != hipSuccess ||
          hipMemsetAsync(ds.err, 0, 2 * sizeof(int32_t), h->st) != hipSuccess ||
          hipEventRecord(h->evStep, h->st) != hipSuccess || hipStreamWaitEvent(h->stF, h->evStep, 0) != hipSuccess ||
          hipEventRecord(h->evS[p][0], h->stF) != hipSuccess)
        return fail(VB_E_HIP, "speculative rebuild fork");
      launch_rs_build(ds, h->stF);
      if (hipEventRecord(h->evS[p][1], h->stF) != hipSuccess || hipEventRecord(h->evRs, h->stF) != hipSuccess)
        return fail(VB_E_HIP, "speculative rebuild join");
      rsSide = true;
    }
    if (early && (rc = specEarly(h, rsSide, storeCleared))) return rc;
    // the global-shutter part of the cost pass inside the speculative linearization (every observation
    // evaluated there: not under dontRetry)
    const bool fuseCost = specNext && h->costFuse && !dontRetry;
    if ((rc = fuseCost ? costFusedEnqueue(h) : costEnqueue(h, 1, false))) return rc;
    const bool wasSpec = specQueued;
    const int wasSet = specSet;
    specQueued = false;
    if (speculate) {
      if (!fuseCost) {  // (fused: recorded after the speculative visual linearization)
        if (hipEventRecord(h->evCost, h->st) != hipSuccess) return fail(VB_E_HIP, "hipEventRecord");
        h->profAtCost = h->profUsed;
      }
      // the next iteration's rebuild + linearization, assuming this step is accepted at full size
      if (specNext) {
        specSet ^= 1;
        if ((rc = specEnqueue(h, dontRetry, specSet, early, rsSide, fuseCost))) return rc;
        specQueued = true;
      }
    }
    profHarvestPrefix(h, h->profDone);  // the previous iteration's event times, read while this one runs
    double r[17];
    if ((rc = speculate ? readIterScalars(h, r, 17) : readRedErr(h, r, 17))) return rc;
    if (it == h->faultFailIt) return fail(VB_E_NUMERIC, "reduced system Cholesky breakdown (injected)");
    out->prev_cost = r[0], out->model_reduction = 0.5 * r[16];
    if (it == h->faultNegModelRedIt) out->model_reduction = -out->model_reduction;  // test fault injection
    const double n = (double)std::max<int64_t>(1, h->nParams);
    out->step_rms_ratio = std::sqrt(r[9] / n);
    costStats(h, r + 1, &out->new_cost, &out->stats);
    if (wasSpec) {
      h->times.linearize_ms = elapsed(h->evS[wasSet][2], h->evS[wasSet][3]);
      if (h->rsDevice) h->times.rs_update_ms = elapsed(h->evS[wasSet][0], h->evS[wasSet][1]);
    } else {
      h->times.linearize_ms = elapsed(h->ev[0], h->ev[1]);
      if (h->rsTimed) h->times.rs_update_ms = elapsed(h->ev[8], h->ev[9]), h->rsTimed = false;
    }
    h->times.schur_ms = elapsed(h->ev[2], h->ev[3]);
    h->times.factor_ms = elapsed(h->ev[3], h->ev[4]);
    h->times.solve_ms = elapsed(h->ev[4], h->ev[5]);
    h->times.step_ms = elapsed(h->ev[10], h->ev[11]);
    h->times.cost_ms = elapsed(h->ev[6], h->ev[7]);
    h->linearized = false, h->factored = true;
    return 0;
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
    h->times.total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (log && verbose) {
      char buf[512];
      snprintf(buf, sizeof(buf),
               "it %d cost %.12g -> %.12g lambda %.3g (t %.2f ms: lin %.2f schur %.2f factor %.2f solve %.2f)", it,
               prevCost, newCost, damping, h->times.total_ms, h->times.linearize_ms, h->times.schur_ms,
               h->times.factor_ms, h->times.solve_ms);
      log(buf, user);
    }
    return 0;
  }
};

// Optimizer::optimize (Optimizer.cpp:768-1106).  An error after an iteration's backup restores the variables
// of that iteration's linearization point before returning.
int vb_optimize(vb_handle h, const vb_settings* sp, vb_log_cb log, vb_prestep_cb pre, void* user, vb_summary* out) {
  if (!h || !h->finalized) return fail(VB_E_STATE, "vb_optimize before vb_finalize");
  vb_settings s;
  if (sp) s = *sp;
  else vb_default_settings(&s);
  const bool preint = h->recomputePreint && h->pi.n > 0;
  // (no memory for the spare buffers: the plain controller, which needs none)
  const bool speculate = !pre && !preint && !h->sharded && !h->partSet && specPrepare(h);
  OptimizeOps ops{h, s.max_num_iterations, s.verbose != 0, log, pre, user, preint, speculate};
  if (const int rc = viba_lm::lmRun(s, ops, out)) {
    if (ops.backedUp && vb_restore(h) == 0) (void)hipStreamSynchronize(h->st);
    (void)hipStreamSynchronize(h->st);
    return rc;
  }
  // (a speculative linearization left queued by a convergence stop is never committed; its buffers are
  // the spare ones)
  HIPCHK(hipStreamSynchronize(h->st));
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
