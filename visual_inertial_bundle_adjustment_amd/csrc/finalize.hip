// vb_finalize: run the host-only symbolic analysis (symbolic.hip) on the handle's Problem, upload its results
// through a local Finalized (host.hpp), move the host-side results it keeps into it, and install it in the
// handle.  No ordering, pattern or schedule logic lives here.
#include "host.hpp"

namespace viba_host {
namespace {

Knobs readKnobs(const vb_handle_s& h) {
  Knobs k;
  // VIBA_ND_CUTWIN=0: the round-1 order, the median cut with left separators (tests/test_ordering_gpu.py)
  if (const char* e = getenv("VIBA_ND_CUTWIN")) k.cutWin = std::max(0.0, std::min(0.45, atof(e)));
  if (const char* e = getenv("VIBA_ND_LEAF")) k.leafDims = std::max<int64_t>(64, atoll(e));
  // VIBA_ND_KINDS=0: every part in plain time order, the order before the class order (tests/test_kind_order_gpu.py)
  if (const char* e = getenv("VIBA_ND_KINDS")) k.kindOrder = atoi(e) != 0;
  k.stats = getenv("VIBA_STATS") != nullptr;
  k.ptFuseMax = h.tune.ptFuseMax, k.useSn = h.tune.useSn, k.snStreams = h.tune.snStreams;
  return k;
}

int uploadSched(DevOwner& m, const SchedHost& H, Sched& S) {
  static_cast<SchedShape&>(S) = H;
  const bool bad = m.put(&S.potrfTileD, H.potrfTile) || m.put(&S.potrfColD, H.potrfCol) || m.put(&S.trsmDiagD, H.trsmDiag) ||
                   m.put(&S.trsmTargetD, H.trsmTarget) || m.put(&S.trsmColD, H.trsmCol) || m.put(&S.trsmRowD, H.trsmRow) ||
                   m.put(&S.updD, H.upd) || m.put(&S.fanPairsD, H.fanPairs) || m.put(&S.tasksFD, H.tasksF) ||
                   m.put(&S.tasksBD, H.tasksB) || m.put(&S.expFD, H.expF) || m.put(&S.expBD, H.expB) ||
                   m.put(&S.preReadyD, H.preReady) || m.put(&S.ptfD, H.ptf) || m.put(&S.ptfDiagD, H.ptfDiag);
  return bad ? VB_E_HIP : 0;
}

int uploadSnSched(DevOwner& m, const SnSchedHost& H, SnSched& S) {
  static_cast<SnSchedShape&>(S) = H;
  const bool bad = m.put(&S.updD, H.upd) || m.put(&S.fanPairsD, H.fanPairs) || m.put(&S.potD, H.pot) ||
                   m.put(&S.rowD, H.row) || m.put(&S.fusD, H.fus) || m.put(&S.copyD, H.copy) ||
                   m.put(&S.invEarlyD, H.invEarly) || m.put(&S.invLateD, H.invLate);
  return bad ? VB_E_HIP : 0;
}

// the Dev scalars and the counts of the analysis
void setScalars(const vb_handle_s& h, const Symbolic& A, Finalized& f) {
  const Problem& P = h.prob;
  Dev& d = f.d;
  d.jac = makeJac(h.cfg.imu_calib_options);
  d.reproj = makeLoss(h.cfg.reproj_loss_radius, h.cfg.reproj_loss_cutoff);
  d.imu = makeLoss(h.cfg.imu_loss_radius, h.cfg.imu_loss_cutoff);
  d.T = TS;
  for (int k = 0; k < 9; k++) d.nvar[k] = A.reg.nvar[k];
  const int64_t nPts = A.reg.nPts;
  d.nRV = A.lay.nRV, d.nRed = A.lay.nRed, d.nPts = nPts, d.nT = A.lay.nT, d.nTiles = A.pat.nTiles;
  d.nObs = A.obs.nObs, d.nObsPad = A.obs.nObsPad, d.nYcol = A.pan.nYcol;
  d.nLxChunk = (int64_t)A.pan.lxChunk.size() / 3;
  d.lmB = A.shard.lmBegin, d.lmE = A.shard.lmEnd, d.root = A.shard.isRoot ? 1 : 0;
  d.nLmSmall = A.shard.nLmSmall, d.nLmBig = A.shard.nLmBig, d.lmBigCols = A.shard.lmBigCols;
  d.obB = A.shard.obB, d.obE = A.shard.obE, d.obFree = A.shard.obFree, d.fB = A.shard.fB, d.fE = A.shard.fE;
  d.nGroups = (int64_t)A.schur.grpRed.size() / 4;
  d.nTileWorks = (int64_t)A.schur.works.size();
  for (int fk = 1; fk < 14; fk++) {
    SmallFactors& sf = d.sf[fk];
    sf.nv = kNumVars[fk], sf.n = (int64_t)P.fint[fk].size(), sf.nc = A.small.nc[fk], sf.stage = A.small.stage[fk];
  }
  d.nSmallStage = A.small.nSmallStage;
  d.myRank = P.partRank, d.world = P.partWorld;
  d.nRS = P.nRS;

  f.nParams = nPts + A.lay.nRV, f.order = nPts * 3 + A.lay.nRedReal;
  f.nClear = (int64_t)A.schur.clearTiles.size(), f.nTileEnt = (int64_t)A.schur.ents.size();
  f.tileFirst = A.schur.tileFirst, f.tileCount = A.schur.tileCount;
  f.nLevels = A.pat.nLevels, f.nPairs = A.sch[0].nPairs + A.sch[1].nPairs;
  f.costRsB[0] = A.cost.rsBegin[0], f.costRsB[1] = A.cost.rsBegin[1];
}

// the host-side results read after vb_finalize, moved out of the analysis (the large lists nobody reads
// again -- tileIdx, the Schur entries and works, the observation arrays -- go with it)
void keepResults(Symbolic& A, Finalized& f) {
  f.visRowOfPos.resize(A.cost.order.size());
  for (size_t i = 0; i < A.cost.order.size(); i++) f.visRowOfPos[i] = (int32_t)A.obs.perm[A.cost.order[i]];
  f.lay = std::move(A.lay), f.shard = std::move(A.shard), f.part = std::move(A.part);
  f.lmOfPoint = std::move(A.reg.lmOfPoint);
  f.tileFill = std::move(A.pat.tileFill);
  f.colStart = std::move(A.pat.colStart), f.colTilesH = std::move(A.pat.colTiles), f.colRowsH = std::move(A.pat.colRows);
  f.rowStart = std::move(A.pat.rowStart), f.rowColH = std::move(A.pat.rowCol);
  f.shardTiles = std::move(A.schur.shardTiles);
  if (A.preint.present) f.piNoise = std::move(A.preint.noise);
  f.bmRowOfPos = std::move(A.bm.rowOfPos);
  f.loneLm = f.shard.loneList;
}

// the rolling-shutter tables: rebuilt on the device (capacities from the IMU stream), or as given
int uploadRsTables(const Problem& P, Finalized& f) {
  Dev& d = f.d;
  DevOwner& m = f.mem;
  if (P.rsDevice) {
    f.rsOff.assign(P.nRS + 1, 0);
    for (int32_t t = 0; t < P.nRS; t++)
      f.rsOff[t + 1] = f.rsOff[t] + rsTableCapacity(P.imuT.data(), (int64_t)P.imuT.size(), P.rsMid[t], P.rsHalf[t]);
    const int64_t ns = f.rsOff[P.nRS];
    std::vector<int32_t> zeroN(P.nRS, 0);
    if (m.put(&d.rsOff, f.rsOff) || m.zeroed(&d.rsS, ns * 11) || m.zeroed(&d.rsI, (ns - P.nRS) * 9) ||
        m.zeroed(&d.rsG, (size_t)P.nRS * 3) || m.put(&d.rsN, zeroN) || m.put(&d.imuT, P.imuT) ||
        m.put(&d.imuV, P.imuV) || m.put(&d.rsMid, P.rsMid) || m.put(&d.rsHalf, P.rsHalf) ||
        m.put(&d.rsCalib, P.rsCalib))
      return VB_E_HIP;
    d.nImu = (int64_t)P.imuT.size();
    d.rsGravVar = P.rsGravVar;
    return 0;
  }
  f.rsOff = P.rsOff;
  std::vector<int32_t> cnt(P.nRS);
  for (int32_t t = 0; t < P.nRS; t++) cnt[t] = (int32_t)(f.rsOff[t + 1] - f.rsOff[t]);
  if (f.rsOff.empty()) f.rsOff.assign(1, 0);
  if (m.put(&d.rsOff, f.rsOff) || m.put(&d.rsS, P.rsS) || m.put(&d.rsI, P.rsI) || m.put(&d.rsG, P.rsG) ||
      m.put(&d.rsN, cnt))
    return VB_E_HIP;
  return 0;
}

// the base map's tables, its factors gathered in sorted order, their cache, records and per-landmark sums:
// nothing is allocated on a handle without base-map factors
int uploadBaseMap(const Problem& P, const Symbolic& A, Finalized& f) {
  const BaseMapOrder& B = A.bm;
  if (B.n == 0) return 0;
  BaseMapDev& b = f.d.bm;
  DevOwner& m = f.mem;
  std::vector<int32_t> pt(B.n), cam(B.n);
  std::vector<double> C((size_t)B.n * 6);
  for (int64_t i = 0; i < B.n; i++) {
    const int64_t r = B.rowOfPos[i];
    pt[i] = P.bmPoint[r], cam[i] = P.bmCamera[r];
    std::copy(&P.bmConst[r * 6], &P.bmConst[r * 6] + 6, &C[i * 6]);
  }
  b.n = B.n, b.nFree = B.nFree, b.nLmWith = (int64_t)B.lmWith.size(), b.nLone = (int64_t)A.shard.loneList.size();
  if (m.put(&b.rig, P.bmRig) || m.put(&b.camT, P.bmCamT) || m.put(&b.cam, P.bmCam) || m.put(&b.camRig, P.bmCamRig) ||
      m.put(&b.pt, pt) || m.put(&b.camOf, cam) || m.put(&b.C, C) || m.put(&b.posOfRow, B.posOfRow) ||
      m.put(&b.start, B.start) || m.put(&b.lmWith, B.lmWith) || m.put(&b.lone, A.shard.loneList) ||
      m.zeroed(&b.cache, B.n) || m.zeroed(&b.rec, (size_t)B.n * 8) || m.zeroed(&b.Vg, (size_t)A.reg.nPts * 9))
    return VB_E_HIP;
  return 0;
}

// every device buffer of vb_finalize, owned by f.mem
int uploadAll(const Problem& P, const Symbolic& A, Finalized& f) {
  Dev& d = f.d;
  DevOwner& m = f.mem;
  const int64_t nPts = A.reg.nPts, nObs = A.obs.nObs, nTiles = A.pat.nTiles;
  const int32_t nT = A.lay.nT;
  // variables and the reduced layout
  for (int k = 0; k < 9; k++)
    if (m.put(&d.var[k], P.data[k]) || m.zeroed(&d.varBak[k], P.data[k].size()) || m.put(&d.redOf[k], A.lay.redOf[k]))
      return VB_E_HIP;
  if (m.put(&d.rvKind, A.lay.rvKind) || m.put(&d.rvHandle, A.lay.rvHandle) || m.put(&d.rvDim, A.lay.rvDim) ||
      m.put(&d.rvOff, A.lay.rvOff) || m.put(&d.rvRowEnd, A.pat.rowEnd) || m.put(&f.padRowsD, A.lay.padRows))
    return VB_E_HIP;
  if (m.put(&d.colOwner, A.lay.colOwner)) return VB_E_HIP;
  // observations
  if (m.put(&d.obCostOrder, A.cost.order) || m.put(&d.obPack, A.cost.pack) || m.put(&d.obCP, A.cost.cp) ||
      m.put(&d.obPose, A.obs.obPose) || m.put(&d.obExtr, A.obs.obExtr) || m.put(&d.obIntr, A.obs.obIntr) ||
      m.put(&d.obVel, A.obs.obVel) || m.put(&d.obRS, A.obs.obRS) || m.put(&d.obPt, A.obs.obPt) ||
      m.put(&d.obRed, A.obs.obRed) || m.put(&d.obCol, A.pan.obCol) || m.put(&d.obC, A.obs.obC) ||
      m.zeroed(&d.cache, nObs) || m.zeroed(&d.Jt, (size_t)kJPlanes * d.nObsPad))
    return VB_E_HIP;
  d.cacheW = d.cache;
  // landmarks
  if (m.put(&d.lmList, A.shard.lmList) || m.put(&d.lmObs, A.obs.lmObs) || m.put(&d.lmY, A.pan.lmY) ||
      m.put(&d.lmBlk, A.pan.lmBlk) || m.put(&d.blkRed, A.pan.blkRed) || m.put(&d.blkCol, A.pan.blkCol) ||
      m.put(&d.ptLm, A.reg.lmOfPoint) || m.put(&d.pcRow, A.pan.pcRow) || m.put(&d.pcBlk, A.pan.pcBlk) ||
      m.put(&d.bxStart, A.pan.bxStart) || m.put(&d.bxEnt, A.pan.bxEnt))
    return VB_E_HIP;
  if (m.zeroed(&d.Vchol, nPts * 6) || m.zeroed(&d.gp, nPts * 3) || m.zeroed(&d.z, nPts * 3) || m.zeroed(&d.xp, nPts * 3) ||
      m.zeroed(&d.Y, A.pan.lmY[nPts] + 128) || m.zeroed(&d.yZero, 256) ||  // + the over-read of the Schur gathers
      m.zeroed(&d.gpNew, nPts * 3) || m.zeroed(&d.zNew, nPts * 3))
    return VB_E_HIP;
  if (m.put(&d.oxStart, A.pan.oxStart) || m.put(&d.oxObs, A.pan.oxObs) || m.put(&d.oxSlot, A.pan.oxSlot) ||
      m.put(&d.lxStart, A.pan.lxStart) || m.put(&d.lxLm, A.pan.lxLm) || m.put(&d.lxCol, A.pan.lxCol) ||
      m.put(&d.lxChunk, A.pan.lxChunk))
    return VB_E_HIP;
  // Schur work
  if (m.put(&d.grpStart, A.schur.grpStart) || m.put(&d.grpObs, A.schur.grpObs) || m.put(&d.grpRed, A.schur.grpRed) ||
      m.put(&d.schurRuns, A.schur.runs) || m.put(&d.schurTasks, A.schur.tasks) || m.put(&d.tileWorks, A.schur.works) ||
      m.put(&d.tileEnts, A.schur.ents))
    return VB_E_HIP;
  if (A.schur.hasClear && m.put(&f.clearTilesD, A.schur.clearTiles)) return VB_E_HIP;
  if (!A.schur.shardTiles.empty() &&
      (m.put(&f.shardTilesD, A.schur.shardTiles) || m.zeroed(&f.shardPack, A.schur.shardTiles.size() * (size_t)TS * TS)))
    return VB_E_HIP;
  // tiles, reduced vectors, pattern
  if (m.put(&d.tileIdx, A.pat.tileIdx) || m.zeroed(&d.tiles, (size_t)nTiles * TS * TS)) return VB_E_HIP;
  const size_t nPad = (size_t)nT * TS;
  if (m.zeroed(&d.gRed, nPad) || m.zeroed(&d.rhs, nPad) || m.zeroed(&d.xRed, nPad) || m.zeroed(&d.gRedNew, nPad) ||
      m.zeroed(&d.stepRed, nPad) || m.zeroed(&d.stepPt, nPts * 3) || m.zeroed(&d.subRed, nPad) ||
      m.zeroed(&d.subPt, nPts * 3) || m.zeroed(&f.yvec, nPad) || m.zeroed(&f.rhsWork, nPad))
    return VB_E_HIP;
  if (m.put(&f.colStartD, A.pat.colStart) || m.put(&f.rowStartD, A.pat.rowStart) || m.zeroed(&f.solveFlags, 4 * (size_t)nT) ||
      m.put(&f.colTilesD, A.pat.colTiles) || m.put(&f.colRowsD, A.pat.colRows) || m.put(&f.rowTilesD, A.pat.rowTiles) ||
      m.put(&f.rowColD, A.pat.rowCol) || m.zeroed(&f.dinv, (size_t)(nT + 1) * 1024) ||
      m.zeroed(&f.linv, (size_t)nT * TS * TS))
    return VB_E_HIP;
  // schedules and their scratch (L_JJ of the fused levels)
  for (int i = 0; i < 2; i++) {
    if (A.sch[i].built && uploadSched(m, A.sch[i], f.sch[i])) return VB_E_HIP;
    if (A.sn[i].built && uploadSnSched(m, A.sn[i], f.sn[i])) return VB_E_HIP;
    if (f.sch[i].nPtfDiag && !f.lscr && m.zeroed(&f.lscr, (size_t)nT * TS * TS)) return VB_E_HIP;
    if (f.sn[i].nCopy && !f.lscrSn && m.zeroed(&f.lscrSn, 2 * (size_t)nT * TS * TS)) return VB_E_HIP;
  }
  if (P.partSet) {
    if (m.put(&f.ownRowsD, A.part.ownRows) || m.zeroed(&f.ownPack, A.part.ownRows.size() * (size_t)TS + 1) ||
        m.put(&f.rootTilesD, A.part.rootTiles) || m.put(&f.rootRowsD, A.part.rootRows) ||
        m.zeroed(&f.rootPack, A.part.rootTiles.size() * (size_t)TS * TS + 1) ||
        m.zeroed(&f.rowPack, A.part.rootRows.size() * (size_t)TS + 1))
      return VB_E_HIP;
  }
  // small factors
  for (int fk = 1; fk < 14; fk++)
    if (m.put(&d.sf[fk].vars, P.fvars[fk]) || m.put(&d.sf[fk].consts, A.small.consts[fk])) return VB_E_HIP;
  if ((A.shard.isRoot || P.partSet) && d.nSmallStage > 0 &&
      (m.zeroed(&d.sJ, (size_t)d.nSmallStage * kSmallJ) || m.zeroed(&d.sE, (size_t)d.nSmallStage * kSmallE) ||
       m.zeroed(&d.sMeta, (size_t)d.nSmallStage * kSmallMeta)))
    return VB_E_HIP;
  // --recompute-preint inputs (preint.hip); PreintArgs holds them as pointers to const
  if (A.preint.present) {
    f.pi.n = (int64_t)P.piSrc.size();
    if (m.put(&f.pi.src, P.piSrc) || m.put(&f.pi.t, A.preint.t) || m.put(&f.pi.v, A.preint.v) ||
        m.put(&f.pi.off, A.preint.off) || m.put(&f.pi.noise, A.preint.noise))
      return VB_E_HIP;
  }
  if (int rc = uploadRsTables(P, f)) return rc;
  if (int rc = uploadBaseMap(P, A, f)) return rc;
  if (m.zeroed(&d.red, 64) || m.zeroed(&d.redS, 2 * 64 * 8) || m.zeroed(&d.err, 8)) return VB_E_HIP;
  return 0;
}

}  // namespace

int doFinalize(vb_handle h) {
  const Problem& P = h->prob;
  const Input in{P.data,     P.cst,     P.fvars,   P.fint,  P.fconst, h->cfg.imu_calib_options,
                 P.nRS,      P.sharded, P.lmBegin, P.lmEnd, P.isRoot, P.partSet,
                 P.partRank, P.partWorld, P.piSrc, P.imuT,  P.imuV,   P.piT,
                 P.piV,      P.piNoise, readKnobs(*h), &P.bmPoint};
  Symbolic A;
  if (const Status e = analyze(in, A)) return fail(e.code, e.msg);
  // built beside the handle and installed whole: a failure drops f with everything it took, and the handle
  // is the created handle it was (a second vb_finalize is legal)
  auto f = std::make_unique<Finalized>();
  setScalars(*h, A, *f);
  if (uploadAll(P, A, *f)) return devFail(f->mem, "vb_finalize: device allocation / copy");
  keepResults(A, *f);
  h->fin = std::move(f);
  return 0;
}

}  // namespace viba_host
