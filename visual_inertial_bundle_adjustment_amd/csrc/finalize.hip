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

int uploadSched(const SchedHost& H, Sched& S) {
  static_cast<SchedShape&>(S) = H;
  if (upload(&S.potrfTileD, H.potrfTile) || upload(&S.potrfColD, H.potrfCol) || upload(&S.trsmDiagD, H.trsmDiag) ||
      upload(&S.trsmTargetD, H.trsmTarget) || upload(&S.trsmColD, H.trsmCol) || upload(&S.trsmRowD, H.trsmRow) ||
      upload(&S.updD, H.upd) || upload(&S.fanPairsD, H.fanPairs) || upload(&S.tasksFD, H.tasksF) ||
      upload(&S.tasksBD, H.tasksB) || upload(&S.expFD, H.expF) || upload(&S.expBD, H.expB) ||
      upload(&S.preReadyD, H.preReady) || upload(&S.ptfD, H.ptf) || upload(&S.ptfDiagD, H.ptfDiag))
    return VB_E_HIP;
  return 0;
}

int uploadSnSched(const SnSchedHost& H, SnSched& S) {
  static_cast<SnSchedShape&>(S) = H;
  if (upload(&S.updD, H.upd) || upload(&S.fanPairsD, H.fanPairs) || upload(&S.potD, H.pot) || upload(&S.rowD, H.row) ||
      upload(&S.fusD, H.fus) || upload(&S.copyD, H.copy) || upload(&S.invEarlyD, H.invEarly) ||
      upload(&S.invLateD, H.invLate))
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
  if (h->rsDevice) {
    // table capacity: the IMU samples of [mid - half, mid + half] widened by 20 ms on both sides (the
    // reference-time offsets of the calibration move the gyro boundaries by far less), + 4
    const int64_t kWidenNs = 20000000;
    h->rsOff.assign(h->nRS + 1, 0);
    for (int32_t t = 0; t < h->nRS; t++) {
      const int64_t a = (h->rsMid[t] - h->rsHalf[t]) * 1000 - kWidenNs, b = (h->rsMid[t] + h->rsHalf[t]) * 1000 + kWidenNs;
      const int64_t cnt = std::upper_bound(h->imuT.begin(), h->imuT.end(), b) -
                          std::lower_bound(h->imuT.begin(), h->imuT.end(), a);
      h->rsOff[t + 1] = h->rsOff[t] + cnt + 4;
    }
    const int64_t ns = h->rsOff[h->nRS];
    std::vector<int32_t> zeroN(h->nRS, 0);
    if (upload(&d.rsOff, h->rsOff) || alloc0(&d.rsS, ns * 11) || alloc0(&d.rsI, (ns - h->nRS) * 9) ||
        alloc0(&d.rsG, (size_t)h->nRS * 3) || upload(&d.rsN, zeroN) || upload(&d.imuT, h->imuT) ||
        upload(&d.imuV, h->imuV) || upload(&d.rsMid, h->rsMid) || upload(&d.rsHalf, h->rsHalf) ||
        upload(&d.rsCalib, h->rsCalib))
      return VB_E_HIP;
    d.nImu = (int64_t)h->imuT.size();
    d.rsGravVar = h->rsGravVar;
    return 0;
  }
  std::vector<int32_t> cnt(h->nRS);
  for (int32_t t = 0; t < h->nRS; t++) cnt[t] = (int32_t)(h->rsOff[t + 1] - h->rsOff[t]);
  if (h->rsOff.empty()) h->rsOff.assign(1, 0);
  if (upload(&d.rsOff, h->rsOff) || upload(&d.rsS, h->rsS) || upload(&d.rsI, h->rsI) || upload(&d.rsG, h->rsG) ||
      upload(&d.rsN, cnt))
    return VB_E_HIP;
  return 0;
}

// every device buffer of vb_finalize.  Each pointer lands in the handle as it is made, so vb_destroy
// frees what exists after a failure.
int uploadAll(vb_handle h, const Symbolic& A) {
  Dev& d = h->d;
  const int64_t nPts = A.reg.nPts, nObs = A.obs.nObs, nTiles = A.pat.nTiles;
  const int32_t nT = A.lay.nT;
  // variables and the reduced layout
  for (int k = 0; k < 9; k++)
    if (upload(&d.var[k], h->data[k]) || alloc0(&d.varBak[k], h->data[k].size()) || upload(&d.redOf[k], A.lay.redOf[k]))
      return VB_E_HIP;
  if (upload(&d.rvKind, A.lay.rvKind) || upload(&d.rvHandle, A.lay.rvHandle) || upload(&d.rvDim, A.lay.rvDim) ||
      upload(&d.rvOff, A.lay.rvOff) || upload(&d.rvRowEnd, A.pat.rowEnd) || upload(&h->padRowsD, A.lay.padRows))
    return VB_E_HIP;
  {
    int8_t* co = nullptr;
    if (upload(&co, A.lay.colOwner)) return VB_E_HIP;
    d.colOwner = co;
  }
  // observations
  if (upload(&d.obCostOrder, A.cost.order) || upload(&d.obPack, A.cost.pack) || upload(&d.obCP, A.cost.cp) ||
      upload(&d.obPose, A.obs.obPose) || upload(&d.obExtr, A.obs.obExtr) || upload(&d.obIntr, A.obs.obIntr) ||
      upload(&d.obVel, A.obs.obVel) || upload(&d.obRS, A.obs.obRS) || upload(&d.obPt, A.obs.obPt) ||
      upload(&d.obRed, A.obs.obRed) || upload(&d.obCol, A.pan.obCol) || upload(&d.obC, A.obs.obC) ||
      alloc0(&d.cache, nObs) || alloc0(&d.Jt, (size_t)kJPlanes * d.nObsPad))
    return VB_E_HIP;
  d.cacheW = d.cache;
  // landmarks
  if (upload(&d.lmList, A.shard.lmList) || upload(&d.lmObs, A.obs.lmObs) || upload(&d.lmY, A.pan.lmY) ||
      upload(&d.lmBlk, A.pan.lmBlk) || upload(&d.blkRed, A.pan.blkRed) || upload(&d.blkCol, A.pan.blkCol) ||
      upload(&d.ptLm, A.reg.lmOfPoint) || upload(&d.pcRow, A.pan.pcRow) || upload(&d.pcBlk, A.pan.pcBlk) ||
      upload(&d.bxStart, A.pan.bxStart) || upload(&d.bxEnt, A.pan.bxEnt))
    return VB_E_HIP;
  if (alloc0(&d.Vchol, nPts * 6) || alloc0(&d.gp, nPts * 3) || alloc0(&d.z, nPts * 3) || alloc0(&d.xp, nPts * 3) ||
      alloc0(&d.Y, A.pan.lmY[nPts] + 128) || alloc0(&d.yZero, 256) ||  // + the over-read of the Schur gathers
      alloc0(&d.gpNew, nPts * 3) || alloc0(&d.zNew, nPts * 3))
    return VB_E_HIP;
  if (upload(&d.oxStart, A.pan.oxStart) || upload(&d.oxObs, A.pan.oxObs) || upload(&d.oxSlot, A.pan.oxSlot) ||
      upload(&d.lxStart, A.pan.lxStart) || upload(&d.lxLm, A.pan.lxLm) || upload(&d.lxCol, A.pan.lxCol) ||
      upload(&d.lxChunk, A.pan.lxChunk))
    return VB_E_HIP;
  // Schur work
  if (upload(&d.grpStart, A.schur.grpStart) || upload(&d.grpObs, A.schur.grpObs) || upload(&d.grpRed, A.schur.grpRed) ||
      upload(&d.schurRuns, A.schur.runs) || upload(&d.schurTasks, A.schur.tasks) || upload(&d.tileWorks, A.schur.works) ||
      upload(&d.tileEnts, A.schur.ents))
    return VB_E_HIP;
  if (A.schur.hasClear && upload(&h->clearTilesD, A.schur.clearTiles)) return VB_E_HIP;
  if (!h->shardTiles.empty() &&
      (upload(&h->shardTilesD, h->shardTiles) || alloc0(&h->shardPack, h->shardTiles.size() * (size_t)TS * TS)))
    return VB_E_HIP;
  // tiles, reduced vectors, pattern
  if (upload(&d.tileIdx, A.pat.tileIdx) || alloc0(&d.tiles, (size_t)nTiles * TS * TS)) return VB_E_HIP;
  const size_t nPad = (size_t)nT * TS;
  if (alloc0(&d.gRed, nPad) || alloc0(&d.rhs, nPad) || alloc0(&d.xRed, nPad) || alloc0(&d.gRedNew, nPad) ||
      alloc0(&d.stepRed, nPad) || alloc0(&d.stepPt, nPts * 3) || alloc0(&d.subRed, nPad) ||
      alloc0(&d.subPt, nPts * 3) || alloc0(&h->yvec, nPad) || alloc0(&h->rhsWork, nPad))
    return VB_E_HIP;
  if (upload(&h->colStartD, h->colStart) || upload(&h->rowStartD, h->rowStart) || alloc0(&h->solveFlags, 4 * (size_t)nT) ||
      upload(&h->colTilesD, h->colTilesH) || upload(&h->colRowsD, h->colRowsH) || upload(&h->rowTilesD, h->rowTilesH) ||
      upload(&h->rowColD, h->rowColH) || alloc0(&h->dinv, (size_t)(nT + 1) * 1024) ||
      alloc0(&h->linv, (size_t)nT * TS * TS))
    return VB_E_HIP;
  // schedules and their scratch (L_JJ of the fused levels)
  for (int i = 0; i < 2; i++) {
    if (A.sch[i].built && uploadSched(A.sch[i], h->sch[i])) return VB_E_HIP;
    if (A.sn[i].built && uploadSnSched(A.sn[i], h->sn[i])) return VB_E_HIP;
    if (h->sch[i].nPtfDiag && !h->lscr && alloc0(&h->lscr, (size_t)nT * TS * TS)) return VB_E_HIP;
    if (h->sn[i].nCopy && !h->lscrSn && alloc0(&h->lscrSn, 2 * (size_t)nT * TS * TS)) return VB_E_HIP;
  }
  if (h->partSet) {
    if (upload(&h->ownRowsD, A.part.ownRows) || alloc0(&h->ownPack, A.part.ownRows.size() * (size_t)TS + 1) ||
        upload(&h->rootTilesD, h->rootTiles) || upload(&h->rootRowsD, h->rootRows) ||
        alloc0(&h->rootPack, h->rootTiles.size() * (size_t)TS * TS + 1) ||
        alloc0(&h->rowPack, h->rootRows.size() * (size_t)TS + 1))
      return VB_E_HIP;
  }
  // small factors
  for (int fk = 1; fk < 14; fk++)
    if (upload(&d.sf[fk].vars, h->fvars[fk]) || upload(&d.sf[fk].consts, A.small.consts[fk])) return VB_E_HIP;
  if ((h->isRoot || h->partSet) && d.nSmallStage > 0 &&
      (alloc0(&d.sJ, (size_t)d.nSmallStage * kSmallJ) || alloc0(&d.sE, (size_t)d.nSmallStage * kSmallE) ||
       alloc0(&d.sMeta, (size_t)d.nSmallStage * kSmallMeta)))
    return VB_E_HIP;
  // --recompute-preint inputs (preint.hip); PreintArgs holds them as pointers to const
  if (A.preint.present) {
    h->pi.n = (int64_t)h->piSrc.size();
    if (upload(const_cast<PreintSrc**>(&h->pi.src), h->piSrc) || upload(const_cast<int64_t**>(&h->pi.t), A.preint.t) ||
        upload(const_cast<double**>(&h->pi.v), A.preint.v) || upload(const_cast<int64_t**>(&h->pi.off), A.preint.off) ||
        upload(const_cast<double**>(&h->pi.noise), A.preint.noise))
      return VB_E_HIP;
  }
  if (int rc = uploadRsTables(h)) return rc;
  if (alloc0(&d.red, 64) || alloc0(&d.redS, 2 * 64 * 8) || alloc0(&d.err, 8)) return VB_E_HIP;
  return 0;
}
}  // namespace

int doFinalize(vb_handle h) {
  const Input in{h->data,    h->cst,     h->fvars,    h->fint,  h->fconst, h->cfg.imu_calib_options,
                 h->nRS,     h->sharded, h->lmBegin,  h->lmEnd, h->isRoot, h->partSet,
                 h->partRank, h->partWorld, h->piSrc, h->imuT,  h->imuV,   h->piT,
                 h->piV,     h->piNoise, readKnobs(*h)};
  Symbolic A;
  // an error leaves the handle as it was: nothing allocated, no field changed
  if (const Status e = analyze(in, A)) return fail(e.code, e.msg);
  copyToHandle(h, A);
  if (int rc = uploadAll(h, A)) return rc;
  h->finalized = true;
  return 0;
}

}  // namespace viba_host
