// Host drivers of the reduced system's factorization and solves over Finalized (host.hpp): the tile Cholesky by
// the column schedule or the two-column supernode schedule, its graphs, the fan-out solves, the back-substitution.
#include "host.hpp"

namespace viba_host {

// vb_damp_factor_solve's forward solve runs inside the factorization (potrf_forward / trsm_kernel)
bool fwdFused(vb_handle h) { return !h->prob.partSet && !h->prob.sharded; }

void factorSeq(vb_handle h, const Sched& S) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  // the forward solve of rhsWork into yvec, fused (schedule 0 of a single handle only)
  const bool fwd = fwdFused(h) && &S == &f.sch[0] && !h->run.factorOnly;
  double* fb = fwd ? f.rhsWork : nullptr;
  double* fy = fwd ? f.yvec : nullptr;
  for (int32_t L = 0; L < S.nLevels; L++) {
    const int64_t p0 = S.lvP[L], t0 = S.lvT[L], u0 = S.lvU[L];
    profBegin(h, KF_GEMM);
    launch_fanin(d, S.updD + 4 * u0, S.fanPairsD, (int)(S.lvU[L + 1] - u0), h->str.st);
    profEnd(h, KF_GEMM);
    if (S.lvPF[L + 1] > S.lvPF[L]) {  // potrf + trsm in one launch
      profBegin(h, KF_POTRF);
      launch_potrf_trsm(d, S.ptfD + 5 * S.lvPF[L], (int)(S.lvPF[L + 1] - S.lvPF[L]), f.lscr, f.dinv, h->str.st, fb, fy);
      profEnd(h, KF_POTRF);
      continue;
    }
    profBegin(h, KF_POTRF);
    launch_potrf(d, S.potrfTileD + p0, S.potrfColD + p0, (int)(S.lvP[L + 1] - p0), f.dinv, h->str.st, fb, fy);
    profEnd(h, KF_POTRF);
    profBegin(h, KF_TRSM);
    launch_trsm(d, S.trsmDiagD + t0, S.trsmTargetD + t0, S.trsmColD + t0, (int)(S.lvT[L + 1] - t0), f.dinv, h->str.st,
                S.trsmRowD + t0, fy, fb);
    profEnd(h, KF_TRSM);
  }
  if (S.nPtfDiag) launch_copy_diag(d, S.ptfDiagD, (int)S.nPtfDiag, f.lscr, h->str.st);
  launch_diag_inverse(d, S.potrfColD, S.lvP[S.nLevels], f.linv, h->str.st);
}

// the two-column supernode schedule (SnSched): per segment (a level of one stream) the fan-in of its
// targets, the supernodes' diagonal blocks, their rows; then the diagonal-tile inverses of the solves
// (every column).  Streams (nGroups > 1): stream g on snStream(g), forked from the main stream and joined
// back at the end; segments queued level by level, a segment after the streams it depends on (segDep)
// record their progress (one event per stream and level: everything they have queued so far is of
// earlier levels).  A profiled factor family runs the same schedule, eagerly (per-launch events).
void factorSeqSn(vb_handle h, int which) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  const SnSched& S = f.sn[which];
  const bool fwd = fwdFused(h) && which == 0 && !h->run.factorOnly;
  double* fb = fwd ? f.rhsWork : nullptr;
  double* fy = fwd ? f.yvec : nullptr;
  const bool forked = S.nGroups > 1;
  const int G = forked ? S.nGroups : 1;
  auto stOf = [&](int g) -> hipStream_t {
    if (!forked) return h->str.st;
    return g == 0 ? h->str.st : g == 1 ? h->str.st2 : g == 2 ? h->str.stZ : h->str.stF;
  };
  if (forked) {
    (void)hipEventRecord(h->str.evSnFork, h->str.st);
    for (int g = 1; g < G; g++) (void)hipStreamWaitEvent(stOf(g), h->str.evSnFork, 0);
  }
  const int nSeg = (int)S.segG.size();
  // the top separators' chain: the trailing run of levels with one segment each
  int chain0 = 0;
  for (int i = 1; i < nSeg; i++)
    if (S.segL[i] == S.segL[i - 1]) chain0 = i + 1;
  // (on a stream the schedule leaves free: stZ at G = 2, stF at G = 3; stZ then waits for it, evClrDone)
  const bool clearHere = h->run.clearWanted && which == 0 && (S.nGroups == 2 || S.nGroups == 3) && !h->run.factorOnly;
  hipStream_t cs = S.nGroups == 2 ? h->str.stZ : h->str.stF;
  // the diagonal-tile inverses of the columns factored before the chain, on the same free stream while the
  // chain runs (a few latency-bound waves per level: the chip has room), instead of after the join
  const bool invEarly = which == 0 && (S.nGroups == 2 || S.nGroups == 3) && S.nInvEarly > 0 && chain0 > 0;
  bool invQueued = false;
  for (int i0 = 0; i0 < nSeg;) {
    int i1 = i0;
    while (i1 < nSeg && S.segL[i1] == S.segL[i0]) i1++;
    if (invEarly && i0 == chain0) {  // every stream's levels so far are done: the tiles before the chain are final
      for (int q = 0; q < G; q++) {
        (void)hipEventRecord(h->str.evInvAt[q], stOf(q));
        (void)hipStreamWaitEvent(cs, h->str.evInvAt[q], 0);
      }
      launch_diag_inverse(d, S.invEarlyD, S.nInvEarly, f.linv, cs);
      (void)hipEventRecord(h->str.evInvDone, cs);
      invQueued = true;
    }
    if (clearHere && i0 == chain0) {  // vb_optimize's clear of the spare tile store
      (void)hipEventRecord(h->str.evClr, stOf(S.segG[i0]));
      (void)hipStreamWaitEvent(cs, h->str.evClr, 0);
      if (clearReduced(h, specDev(h), cs) == 0) h->run.clearQueued = true;
      // (stF: specEarly makes stZ wait for it -- not here, where stZ is a factor stream the join waits for)
      h->run.clearOnF = cs != h->str.stZ;
      if (h->run.clearOnF) (void)hipEventRecord(h->str.evClrDone, cs);
      h->run.clearWanted = false;
    }
    if (forked) {  // the level's cross-stream dependencies, recorded before any of its launches
      uint32_t need = 0;
      for (int i = i0; i < i1; i++) need |= (uint32_t)S.segDep[i];
      for (int q = 0; q < G; q++)
        if (need >> q & 1) (void)hipEventRecord(h->str.evSnLvl[q], stOf(q));
    }
    for (int i = i0; i < i1; i++) {
      hipStream_t st = stOf(S.segG[i]);
      if (forked)
        for (int q = 0; q < G; q++)
          if ((uint32_t)S.segDep[i] >> q & 1) (void)hipStreamWaitEvent(st, h->str.evSnLvl[q], 0);
      const int64_t u0 = S.lvU[i], s0 = S.lvS[i], r0 = S.lvR[i];
      profBegin(h, KF_GEMM);
      launch_fanin(d, S.updD + 4 * u0, S.fanPairsD, (int)(S.lvU[i + 1] - u0), st);
      profEnd(h, KF_GEMM);
      profBegin(h, KF_POTRF);
      if (S.lvF[i + 1] > S.lvF[i])
        launch_snpotrf_trsm(d, S.fusD + 8 * S.lvF[i], (int)(S.lvF[i + 1] - S.lvF[i]), f.lscrSn, f.dinv, st, fb, fy);
      launch_snpotrf(d, S.potD + 4 * s0, (int)(S.lvS[i + 1] - s0), f.dinv, st, fb, fy);
      profEnd(h, KF_POTRF);
      profBegin(h, KF_TRSM);
      launch_sntrsm(d, S.rowD + 8 * r0, (int)(S.lvR[i + 1] - r0), f.dinv, st, fy, fb);
      profEnd(h, KF_TRSM);
    }
    i0 = i1;
  }
  if (forked)
    for (int q = 1; q < G; q++) {
      (void)hipEventRecord(h->str.evSnLvl[q], stOf(q));
      (void)hipStreamWaitEvent(h->str.st, h->str.evSnLvl[q], 0);
    }
  if (S.nCopy) launch_copy_diag(d, S.copyD, (int)S.nCopy, f.lscrSn, h->str.st);
  if (invQueued) {
    launch_diag_inverse(d, S.invLateD, S.nInvLate, f.linv, h->str.st);
    (void)hipStreamWaitEvent(h->str.st, h->str.evInvDone, 0);
    return;
  }
  const Sched& C = f.sch[which];
  launch_diag_inverse(d, C.potrfColD, C.lvP[C.nLevels], f.linv, h->str.st);
}

// launch sequences are fixed by the symbolic structure: capture them once into HIP graphs
// (unless one of their kernel families is being profiled, which needs per-launch events)
int captureGraph(vb_handle h, const Sched& S, hipGraphExec_t* out, bool sn = false, int which = 0) {
  hipGraph_t g;
  HIPCHK(hipStreamBeginCapture(h->str.st, hipStreamCaptureModeThreadLocal));
  if (sn) factorSeqSn(h, which);
  else factorSeq(h, S);
  HIPCHK(hipStreamEndCapture(h->str.st, &g));
  HIPCHK(hipGraphInstantiate(out, g, nullptr, nullptr, 0));
  HIPCHK(hipGraphDestroy(g));
  return 0;
}

// factor the columns of schedule `which` (0: all, or this rank's subtree in partition mode; 1: ROOT)
int factorReduced(vb_handle h, int which) {
  Sched& S = h->fin->sch[which];
  if (!S.built) return fail(VB_E_STATE, "no factorization schedule here (partition root on rank 0 only)");
  const bool prof = h->prof.family == KF_POTRF || h->prof.family == KF_GEMM || h->prof.family == KF_TRSM;
  // (a profiled family runs launch by launch: its per-launch events, recorded as event nodes inside
  // a graph, cost as much as the graph saves -- measured)
  const bool sn = h->fin->sn[which].built;
  if (!h->tune.useGraphs || prof || h->run.factorOnly || (sn && h->fin->sn[which].nGroups > 1)) {
    if (sn) factorSeqSn(h, which);
    else factorSeq(h, S);
    return 0;
  }
  hipGraphExec_t& g = sn ? h->fin->sn[which].graph[h->fin->tileSet] : S.graph[h->fin->tileSet];
  if (!g)
    if (int rc = captureGraph(h, S, &g, sn, which)) return rc;
  HIPCHK(hipGraphLaunch(g, h->str.st));
  return 0;
}

// solves with rhsWork as right-hand side, result in xRed (schedule `which`, phases bit 0 forward,
// bit 1 backward; a partitioned backward pass takes the ROOT rows of xRed as given)
int solveReduced(vb_handle h, int which, int phases) {
  Finalized& f = *h->fin;
  Sched& S = f.sch[which];
  if (!S.built) return fail(VB_E_STATE, "no solve schedule here (partition root on rank 0 only)");
  Dev& d = f.d;
  // one persistent workgroup per CU (every launched workgroup must be resident at once)
  profBegin(h, KF_FWD);
  launch_solve_fanout(d, S.tasksFD, S.nF, S.tasksBD, S.nB, S.expFD, S.expBD, f.colTilesD, f.colRowsD, f.rowTilesD,
                      f.rowColD, f.linv, f.rhsWork, f.yvec, d.xRed, f.solveFlags, h->tune.numCUs, h->str.st, phases,
                      S.preReadyD, S.nPreReady);
  profEnd(h, KF_FWD);
  return 0;
}

// x_red (xRed) -> points of this shard (x_p = L^-T (z - Y x_c)), step = -x (which 0) or sub-step
// (which 1), and the partial model-cost dot into red[16] (x_red . g_red partial + shard points)
void backSubstitute(vb_handle h, int which) {
  Dev& d = h->fin->d;
  const int64_t p0 = d.lmB * 3, np = (d.lmE - d.lmB) * 3;
  profBegin(h, KF_BACKSUB);
  launch_backsub(d, which, d.lmB, d.lmE, d.xRed, d.xp, h->str.st);
  profEnd(h, KF_BACKSUB);
  if (which == 0) {
    (void)hipMemsetAsync(d.red + 16, 0, 8 * sizeof(double), h->str.st);
    launch_dot(d.xRed, d.gRed, d.nRed, d.red + 16, h->str.st);
    launch_dot(d.xp + p0, d.gp + p0, np, d.red + 16, h->str.st);
  }
  launch_axpby(which ? d.subRed : d.stepRed, d.xRed, -1.0, 0.0, d.nRed, h->str.st);
  launch_axpby((which ? d.subPt : d.stepPt) + p0, d.xp + p0, -1.0, 0.0, np, h->str.st);
}

}  // namespace viba_host
