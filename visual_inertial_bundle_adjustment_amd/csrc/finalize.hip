// vb_finalize: run the host-only symbolic analysis (symbolic.hip) on what the handle holds, then copy
// its results into the handle and upload them.  No ordering, pattern or schedule logic lives here.
#include "host.hpp"

namespace viba_host {
namespace {

Knobs readKnobs(const vb_handle_s& h) {
  Knobs k;
  // VIBA_ND_CUTWIN=0: the round-1 order, the median cut with left separators (tests/test_ordering_gpu.py)
  if (const char* e = getenv("VIBA_ND_CUTWIN")) k.cutWin = std::max(0.0, std::min(0.45, atof(e)));
  if (const char* e = getenv("VIBA_ND_LEAF")) k.leafDims = std::max<int64_t>(64, atoll(e));
  k.stats = getenv("VIBA_STATS") != nullptr;
  k.ptFuseMax = h.ptFuseMax, k.useSn = h.useSn, k.snStreams = h.snStreams;
  return k;
}

int uploadSched(DevOwner& m, const SchedHost& H, Sched& S) {
  static_cast<SchedShape&>(S) = H;
  if (m.put(&S.potrfTileD, H.potrfTile) || m.put(&S.potrfColD, H.potrfCol) || m.put(&S.trsmDiagD, H.trsmDiag) ||
      m.put(&S.trsmTargetD, H.trsmTarget) || m.put(&S.trsmColD, H.trsmCol) || m.put(&S.trsmRowD, H.trsmRow) ||
      m.put(&S.updD, H.upd) || m.put(&S.fanPairsD, H.fanPairs) || m.put(&S.tasksFD, H.tasksF) ||
      m.put(&S.tasksBD, H.tasksB) || m.put(&S.expFD, H.expF) || m.put(&S.expBD, H.expB) ||
      m.put(&S.preReadyD, H.preReady) || m.put(&S.ptfD, H.ptf) || m.put(&S.ptfDiagD, H.ptfDiag))
    return VB_E_HIP;
  return 0;
}

int uploadSnSched(DevOwner& m, const SnSchedHost& H, SnSched& S) {
  static_cast<SnSchedShape&>(S) = H;
  if (m.put(&S.updD, H.upd) || m.put(&S.fanPairsD, H.fanPairs) || m.put(&S.potD, H.pot) || m.put(&S.rowD, H.row) ||
      m.put(&S.fusD, H.fus) || m.put(&S.copyD, H.copy) || m.put(&S.invEarlyD, H.invEarly) ||
      m.put(&S.invLateD, H.invLate))
    return VB_E_HIP;
  return 0;
}

// the host-side results the handle keeps, and the Dev scalars
void copyToHandle(vb_handle h, const Symbolic& A) {
  Dev& d = h->d;
  d.jac = makeJac(h->cfg.imu_calib_options);
  d.reproj = makeLoss(h->cfg.reproj_loss_radius, h->cfg.reproj_loss_cutoff);
  d.imu = makeLoss(h->cfg.imu_loss_radius, h->cfg.imu_loss_cutoff);
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
    sf.nv = kNumVars[fk], sf.n = (int64_t)h->fint[fk].size(), sf.nc = A.small.nc[fk], sf.stage = A.small.stage[fk];
  }
  d.nSmallStage = A.small.nSmallStage;
  d.myRank = h->partRank, d.world = h->partWorld;
  d.nRS = h->nRS;

  h->rvKind = A.lay.rvKind, h->rvHandle = A.lay.rvHandle, h->rvDim = A.lay.rvDim, h->rvOff = A.lay.rvOff;
  h->lmOfPoint = A.reg.lmOfPoint;
  h->colOwner = A.lay.colOwner;
  h->nRedReal = A.lay.nRedReal, h->nParts = (int64_t)A.nd.partBegin.size();
  h->nParams = nPts + A.lay.nRV;
  h->order = nPts * 3 + A.lay.nRedReal;
  h->nPadRows = (int64_t)A.lay.padRows.size();
  h->nLmObs = A.obs.lmObs[nPts];
  h->lmBegin = A.shard.lmBegin, h->lmEnd = A.shard.lmEnd, h->isRoot = A.shard.isRoot;
  h->tileFill = A.pat.tileFill;
  h->colStart = A.pat.colStart, h->colTilesH = A.pat.colTiles, h->colRowsH = A.pat.colRows;
  h->rowStart = A.pat.rowStart, h->rowTilesH = A.pat.rowTiles, h->rowColH = A.pat.rowCol;
  h->nClear = (int64_t)A.schur.clearTiles.size();
  h->nTileEnt = (int64_t)A.schur.ents.size(), h->nObEnt = d.nGroups;
  h->tileFirst = A.schur.tileFirst, h->tileCount = A.schur.tileCount;
  h->shardTiles = A.schur.shardTiles;
  h->zeroRuns = A.part.zeroRuns, h->rootTiles = A.part.rootTiles, h->rootRows = A.part.rootRows;
  h->nOwnRows = (int64_t)A.part.ownRows.size();
  h->nLevels = A.pat.nLevels;
  h->nPairs = A.sch[0].nPairs + A.sch[1].nPairs;
  h->costRsB[0] = A.cost.rsBegin[0], h->costRsB[1] = A.cost.rsBegin[1];
  h->visRowOfPos.resize(A.cost.order.size());
  for (size_t i = 0; i < A.cost.order.size(); i++) h->visRowOfPos[i] = (int32_t)A.obs.perm[A.cost.order[i]];
  if (A.preint.present) h->piNoise = A.preint.noise;
}

// the rolling-shutter tables: rebuilt on the device (capacities from the IMU stream), or as given
int uploadRsTables(vb_handle h) {
  Dev& d = h->d;
  DevOwner& m = h->fin;
  if (h->rsDevice) {
    h->rsOff.assign(h->nRS + 1, 0);
    for (int32_t t = 0; t < h->nRS; t++)
      h->rsOff[t + 1] = h->rsOff[t] + rsTableCapacity(h->imuT.data(), (int64_t)h->imuT.size(), h->rsMid[t], h->rsHalf[t]);
    const int64_t ns = h->rsOff[h->nRS];
    std::vector<int32_t> zeroN(h->nRS, 0);
    if (m.put(&d.rsOff, h->rsOff) || m.zeroed(&d.rsS, ns * 11) || m.zeroed(&d.rsI, (ns - h->nRS) * 9) ||
        m.zeroed(&d.rsG, (size_t)h->nRS * 3) || m.put(&d.rsN, zeroN) || m.put(&d.imuT, h->imuT) ||
        m.put(&d.imuV, h->imuV) || m.put(&d.rsMid, h->rsMid) || m.put(&d.rsHalf, h->rsHalf) ||
        m.put(&d.rsCalib, h->rsCalib))
      return VB_E_HIP;
    d.nImu = (int64_t)h->imuT.size();
    d.rsGravVar = h->rsGravVar;
    return 0;
  }
  std::vector<int32_t> cnt(h->nRS);
  for (int32_t t = 0; t < h->nRS; t++) cnt[t] = (int32_t)(h->rsOff[t + 1] - h->rsOff[t]);
  if (h->rsOff.empty()) h->rsOff.assign(1, 0);
  if (m.put(&d.rsOff, h->rsOff) || m.put(&d.rsS, h->rsS) || m.put(&d.rsI, h->rsI) || m.put(&d.rsG, h->rsG) ||
      m.put(&d.rsN, cnt))
    return VB_E_HIP;
  return 0;
}

// every device buffer of vb_finalize, owned by the handle's `fin` group
int uploadAll(vb_handle h, const Symbolic& A) {
  Dev& d = h->d;
  DevOwner& m = h->fin;
  const int64_t nPts = A.reg.nPts, nObs = A.obs.nObs, nTiles = A.pat.nTiles;
  const int32_t nT = A.lay.nT;
  // variables and the reduced layout
  for (int k = 0; k < 9; k++)
    if (m.put(&d.var[k], h->data[k]) || m.zeroed(&d.varBak[k], h->data[k].size()) || m.put(&d.redOf[k], A.lay.redOf[k]))
      return VB_E_HIP;
  if (m.put(&d.rvKind, A.lay.rvKind) || m.put(&d.rvHandle, A.lay.rvHandle) || m.put(&d.rvDim, A.lay.rvDim) ||
      m.put(&d.rvOff, A.lay.rvOff) || m.put(&d.rvRowEnd, A.pat.rowEnd) || m.put(&h->padRowsD, A.lay.padRows))
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
  if (A.schur.hasClear && m.put(&h->clearTilesD, A.schur.clearTiles)) return VB_E_HIP;
  if (!h->shardTiles.empty() &&
      (m.put(&h->shardTilesD, h->shardTiles) || m.zeroed(&h->shardPack, h->shardTiles.size() * (size_t)TS * TS)))
    return VB_E_HIP;
  // tiles, reduced vectors, pattern
  if (m.put(&d.tileIdx, A.pat.tileIdx) || m.zeroed(&d.tiles, (size_t)nTiles * TS * TS)) return VB_E_HIP;
  const size_t nPad = (size_t)nT * TS;
  if (m.zeroed(&d.gRed, nPad) || m.zeroed(&d.rhs, nPad) || m.zeroed(&d.xRed, nPad) || m.zeroed(&d.gRedNew, nPad) ||
      m.zeroed(&d.stepRed, nPad) || m.zeroed(&d.stepPt, nPts * 3) || m.zeroed(&d.subRed, nPad) ||
      m.zeroed(&d.subPt, nPts * 3) || m.zeroed(&h->yvec, nPad) || m.zeroed(&h->rhsWork, nPad))
    return VB_E_HIP;
  if (m.put(&h->colStartD, h->colStart) || m.put(&h->rowStartD, h->rowStart) || m.zeroed(&h->solveFlags, 4 * (size_t)nT) ||
      m.put(&h->colTilesD, h->colTilesH) || m.put(&h->colRowsD, h->colRowsH) || m.put(&h->rowTilesD, h->rowTilesH) ||
      m.put(&h->rowColD, h->rowColH) || m.zeroed(&h->dinv, (size_t)(nT + 1) * 1024) ||
      m.zeroed(&h->linv, (size_t)nT * TS * TS))
    return VB_E_HIP;
  // schedules and their scratch (L_JJ of the fused levels)
  for (int i = 0; i < 2; i++) {
    if (A.sch[i].built && uploadSched(m, A.sch[i], h->sch[i])) return VB_E_HIP;
    if (A.sn[i].built && uploadSnSched(m, A.sn[i], h->sn[i])) return VB_E_HIP;
    if (h->sch[i].nPtfDiag && !h->lscr && m.zeroed(&h->lscr, (size_t)nT * TS * TS)) return VB_E_HIP;
    if (h->sn[i].nCopy && !h->lscrSn && m.zeroed(&h->lscrSn, 2 * (size_t)nT * TS * TS)) return VB_E_HIP;
  }
  if (h->partSet) {
    if (m.put(&h->ownRowsD, A.part.ownRows) || m.zeroed(&h->ownPack, A.part.ownRows.size() * (size_t)TS + 1) ||
        m.put(&h->rootTilesD, h->rootTiles) || m.put(&h->rootRowsD, h->rootRows) ||
        m.zeroed(&h->rootPack, h->rootTiles.size() * (size_t)TS * TS + 1) ||
        m.zeroed(&h->rowPack, h->rootRows.size() * (size_t)TS + 1))
      return VB_E_HIP;
  }
  // small factors
  for (int fk = 1; fk < 14; fk++)
    if (m.put(&d.sf[fk].vars, h->fvars[fk]) || m.put(&d.sf[fk].consts, A.small.consts[fk])) return VB_E_HIP;
  if ((h->isRoot || h->partSet) && d.nSmallStage > 0 &&
      (m.zeroed(&d.sJ, (size_t)d.nSmallStage * kSmallJ) || m.zeroed(&d.sE, (size_t)d.nSmallStage * kSmallE) ||
       m.zeroed(&d.sMeta, (size_t)d.nSmallStage * kSmallMeta)))
    return VB_E_HIP;
  // --recompute-preint inputs (preint.hip); PreintArgs holds them as pointers to const
  if (A.preint.present) {
    h->pi.n = (int64_t)h->piSrc.size();
    if (m.put(&h->pi.src, h->piSrc) || m.put(&h->pi.t, A.preint.t) || m.put(&h->pi.v, A.preint.v) ||
        m.put(&h->pi.off, A.preint.off) || m.put(&h->pi.noise, A.preint.noise))
      return VB_E_HIP;
  }
  if (int rc = uploadRsTables(h)) return rc;
  if (m.zeroed(&d.red, 64) || m.zeroed(&d.redS, 2 * 64 * 8) || m.zeroed(&d.err, 8)) return VB_E_HIP;
  return 0;
}

// what copyToHandle and uploadAll set, back to a created handle's values (the `fin` group released)
void unfinalize(vb_handle h) {
  h->d = Dev();
  h->pi = PreintArgs();
  for (int i = 0; i < 2; i++) h->sch[i] = Sched(), h->sn[i] = SnSched();
  h->padRowsD = nullptr, h->clearTilesD = nullptr, h->shardTilesD = nullptr, h->shardPack = nullptr;
  h->yvec = h->rhsWork = h->dinv = h->linv = h->lscr = h->lscrSn = nullptr;
  h->colStartD = h->rowStartD = nullptr, h->solveFlags = nullptr;
  h->colTilesD = h->colRowsD = h->rowTilesD = h->rowColD = nullptr;
  h->ownRowsD = h->rootTilesD = h->rootRowsD = nullptr, h->ownPack = h->rootPack = h->rowPack = nullptr;
  h->rvKind.clear(), h->rvHandle.clear(), h->rvDim.clear(), h->rvOff.clear(), h->lmOfPoint.clear(), h->colOwner.clear();
  h->nRedReal = h->nParts = h->nParams = h->order = h->nPadRows = h->nLmObs = h->nClear = h->nTileEnt = h->nObEnt = 0;
  h->tileFill.clear(), h->colStart.clear(), h->colTilesH.clear(), h->colRowsH.clear();
  h->rowStart.clear(), h->rowTilesH.clear(), h->rowColH.clear();
  h->tileFirst = h->tileCount = h->nOwnRows = h->nPairs = 0, h->nLevels = 0;
  h->shardTiles.clear(), h->zeroRuns.clear(), h->rootTiles.clear(), h->rootRows.clear(), h->visRowOfPos.clear();
  h->costRsB[0] = h->costRsB[1] = 0;
}
}  // namespace

int doFinalize(vb_handle h) {
  const Input in{h->data,    h->cst,     h->fvars,    h->fint,  h->fconst, h->cfg.imu_calib_options,
                 h->nRS,     h->sharded, h->lmBegin,  h->lmEnd, h->isRoot, h->partSet,
                 h->partRank, h->partWorld, h->piSrc, h->imuT,  h->imuV,   h->piT,
                 h->piV,     h->piNoise, readKnobs(*h)};
  Symbolic A;
  // an error leaves the handle as it was: nothing allocated, no field changed (a second vb_finalize is legal)
  if (const Status e = analyze(in, A)) return fail(e.code, e.msg);
  // the inputs that the results overwrite: the shard as given, the noise and the table offsets
  const int64_t lmBegin = h->lmBegin, lmEnd = h->lmEnd;
  const bool isRoot = h->isRoot;
  const std::vector<double> piNoise = h->piNoise;
  const std::vector<int64_t> rsOff = h->rsOff;
  copyToHandle(h, A);
  if (uploadAll(h, A)) {
    const int rc = devFail(h->fin, "vb_finalize: device allocation / copy");
    h->fin.release();
    unfinalize(h);
    h->lmBegin = lmBegin, h->lmEnd = lmEnd, h->isRoot = isRoot, h->piNoise = piNoise, h->rsOff = rsOff;
    return rc;
  }
  h->finalized = true;
  return 0;
}

}  // namespace viba_host
