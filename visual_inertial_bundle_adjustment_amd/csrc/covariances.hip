// Covariances (≙ Optimizer::computeJointCovariances / computeCovariances, Optimizer.cpp:503-697): the
// selected inversion of the tile factor (selinv.hip), the per-column solves of off-pattern blocks, and the
// covariances of landmark points from the inversion and the elimination's panels (pointcov.hip).
#include "host.hpp"

// (kind, handle) -> reduced variable
static std::unordered_map<int64_t, int32_t> reducedIndex(vb_handle h) {
  std::unordered_map<int64_t, int32_t> rvOf;
  for (size_t i = 0; i < h->fin->lay.rvKind.size(); i++) rvOf[((int64_t)h->fin->lay.rvKind[i] << 32) | (uint32_t)h->fin->lay.rvHandle[i]] = (int32_t)i;
  return rvOf;
}

// The prologue of both covariance calls (Optimizer.cpp:503-545): linearize at the current variables without
// touching the cost cache, eliminate the points at the damping, assemble and factor the reduced system
// (initDirectSolverData + factor); while the factor breaks down the damping is raised (+1e-9 below 1e-9,
// else x2).  *used = the damping of the factor that succeeded.  Leaves Vchol, the Y panels and the factor.
static int covariancePrologue(vb_handle h, double damping, double* used) {
  Dev& d = h->fin->d;
  double lam = damping;
  for (int attempt = 0;; attempt++) {
    if (int rc = vb_linearize(h, 0, 0, nullptr)) return rc;
    HIPCHK(hipMemsetAsync(d.err, 0, sizeof(int32_t), h->str.st));
    launch_landmark(d, lam, 0, h->str.st);
    HIPCHK(hipMemsetAsync(d.rhs, 0, (size_t)d.nT * TS * sizeof(double), h->str.st));
    launch_schur(d, lam, 1, h->str.st);
    h->run.factorOnly = true;  // (the fused forward solve would run on a stale right-hand side)
    const int frc = factorReduced(h);
    h->run.factorOnly = false;
    if (frc) return frc;
    int32_t e = 0;
    HIPCHK(hipMemcpyAsync(&e, d.err, sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
    HIPCHK(hipStreamSynchronize(h->str.st));
    if (!(e & (2 | 8))) {
      if (int rc = checkErr(h)) return rc;
      break;
    }
    if (attempt > 200) return fail(VB_E_NUMERIC, "covariances: factor keeps breaking down");
    lam = lam < 1e-9 ? lam + 1e-9 : lam * 2.0;
  }
  *used = lam;
  return 0;
}

extern "C" {
int selectedInversion(vb_handle h) {
  Dev& d = h->fin->d;
  const int32_t nT = d.nT;
  std::vector<int32_t> level(nT, 0);
  int32_t nLev = 0;
  for (int32_t J = 0; J < nT; J++) {
    for (int64_t i = h->fin->rowStart[J]; i < h->fin->rowStart[J + 1]; i++) level[J] = std::max(level[J], level[h->fin->rowColH[i]] + 1);
    nLev = std::max(nLev, level[J] + 1);
  }
  std::vector<std::vector<int32_t>> cols(nLev);
  for (int32_t J = 0; J < nT; J++) cols[level[J]].push_back(J);
  // per level: U items (L slot, J), Z items (target slot, I, J, first U of the column), diagonal items
  // (J, first U); U indices restart at 0 every level (one compact scratch of the largest level)
  std::vector<int32_t> uIt, zIt, dIt;
  std::vector<int64_t> lvU(nLev + 1, 0), lvZ(nLev + 1, 0), lvD(nLev + 1, 0);
  int64_t maxU = 1;
  for (int32_t L = nLev - 1, k = 0; L >= 0; L--, k++) {
    int32_t u = 0;
    for (int32_t J : cols[L]) {
      const int64_t c0 = h->fin->colStart[J], n = h->fin->colStart[J + 1] - c0;
      for (int64_t q = 1; q < n; q++) {
        uIt.insert(uIt.end(), {h->fin->colTilesH[c0 + q], J});
        zIt.insert(zIt.end(), {h->fin->colTilesH[c0 + q], h->fin->colRowsH[c0 + q], J, u});
      }
      dIt.insert(dIt.end(), {J, u});
      u += (int32_t)(n - 1);
    }
    maxU = std::max<int64_t>(maxU, u);
    lvU[k + 1] = (int64_t)uIt.size() / 2, lvZ[k + 1] = (int64_t)zIt.size() / 4, lvD[k + 1] = (int64_t)dIt.size() / 2;
  }
  DevOwner m;  // the level lists and the U scratch, freed when the call returns
  int32_t *uD = nullptr, *zD = nullptr, *dD = nullptr;
  double* U = nullptr;
  if (m.put(&uD, uIt) || m.put(&zD, zIt) || m.put(&dD, dIt) || m.get(&U, (size_t)maxU * TS * TS))
    return fail(VB_E_HIP, "selected inversion: device allocation");
  for (int32_t k = 0; k < nLev; k++)
    launch_selinv_level(d.tiles, d.tileIdx, nT, h->fin->colStartD, h->fin->colRowsD, h->fin->colTilesD, h->fin->linv, U,
                        uD + 2 * lvU[k], (int)(lvU[k + 1] - lvU[k]), zD + 4 * lvZ[k], (int)(lvZ[k + 1] - lvZ[k]),
                        dD + 2 * lvD[k], (int)(lvD[k + 1] - lvD[k]), h->str.st);
  if (hipStreamSynchronize(h->str.st) != hipSuccess) return fail(VB_E_HIP, "selected inversion: kernel failure");
  return 0;
}

int vb_compute_covariances(vb_handle h, double damping, int64_t n_blocks, const int64_t* block_start,
                           const int32_t* kinds, const int32_t* handles, double* out, double* used_damping) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_compute_covariances before vb_finalize");
  if (h->prob.partSet || h->prob.sharded) return fail(VB_E_UNSUPPORTED, "covariances run on a single handle");
  if (n_blocks < 0 || (n_blocks > 0 && (!block_start || !kinds || !handles || !out)))
    return fail(VB_E_ARG, "vb_compute_covariances: null argument");
  if (!h->fin->sch[0].built) return fail(VB_E_STATE, "no factorization schedule");
  const std::unordered_map<int64_t, int32_t> rvOf = reducedIndex(h);
  const int64_t nv = n_blocks ? block_start[n_blocks] : 0;
  std::vector<int32_t> rv(nv);
  for (int64_t q = 0; q < n_blocks; q++)
    if (block_start[q + 1] < block_start[q]) return fail(VB_E_ARG, "block_start must be non-decreasing");
  for (int64_t i = 0; i < nv; i++) {
    if (kinds[i] == VB_VAR_POINT) return fail(VB_E_UNSUPPORTED, "covariance of a landmark point (points are eliminated)");
    auto it = rvOf.find(((int64_t)kinds[i] << 32) | (uint32_t)handles[i]);
    if (it == rvOf.end()) return fail(VB_E_ARG, "covariance of a constant or unknown variable");
    rv[i] = it->second;
  }
  Dev& d = h->fin->d;
  double lam = damping;
  if (int rc = covariancePrologue(h, damping, &lam)) return rc;
  if (used_damping) *used_damping = lam;
  // Every element (row ra, column rb of the padded reduced order) of a block whose tiles lie on the
  // factor's pattern comes from the selected inversion.  That covers SingleSessionProblem::
  // computeCovariances' request (SingleSessionProblem.cpp:66-118): a rig's pose, velocity and omega
  // couple directly in S, and a calibration variable is one block.  Blocks off the pattern (joint
  // blocks of uncoupled variables) take one reduced solve per column S x = e, before the inversion
  // consumes the factor.  VIBA_COV_SOLVES=1 sends every block that way (test aid).
  const int32_t nT = d.nT;
  std::vector<int32_t> tix((size_t)nT * nT, -1);
  for (int32_t J = 0; J < nT; J++)
    for (int64_t c = h->fin->colStart[J]; c < h->fin->colStart[J + 1]; c++) tix[(size_t)h->fin->colRowsH[c] * nT + J] = h->fin->colTilesH[c];
  auto elem = [&](int64_t ra, int64_t rb) -> int64_t {  // Z(ra, rb) in the tile store, -1 off the pattern
    if (ra / TS < rb / TS) std::swap(ra, rb);
    const int32_t t = tix[(size_t)(ra / TS) * nT + rb / TS];
    return t < 0 ? -1 : (int64_t)t * TS * TS + (rb % TS) * TS + ra % TS;
  };
  const bool forceSolves = getenv("VIBA_COV_SOLVES") && atoi(getenv("VIBA_COV_SOLVES")) == 1;
  std::vector<int64_t> outOff(n_blocks + 1, 0), gidx;
  std::vector<uint8_t> bySolve(n_blocks, forceSolves ? 1 : 0);
  std::vector<std::vector<int64_t>> offs(n_blocks);
  for (int64_t q = 0; q < n_blocks; q++) {
    const int64_t b = block_start[q], e = block_start[q + 1];
    std::vector<int64_t>& off = offs[q];
    off.assign(e - b + 1, 0);
    for (int64_t i = b; i < e; i++) off[i - b + 1] = off[i - b] + h->fin->lay.rvDim[rv[i]];
    const int64_t n = off.back();
    outOff[q + 1] = outOff[q] + n * n;
    for (int64_t i = b; i < e; i++)
      for (int c = 0; c < h->fin->lay.rvDim[rv[i]]; c++)
        for (int64_t j = b; j < e; j++)
          for (int r = 0; r < h->fin->lay.rvDim[rv[j]]; r++) {
            const int64_t at = elem(h->fin->lay.rvOff[rv[j]] + r, h->fin->lay.rvOff[rv[i]] + c);
            gidx.push_back(at);
            if (at < 0) bySolve[q] = 1;
          }
  }
  const int64_t nPad = (int64_t)nT * TS;
  std::vector<double> rhs(nPad, 0.0), x(nPad);
  bool anyInv = false;
  for (int64_t q = 0; q < n_blocks; q++) {
    if (!bySolve[q]) {
      anyInv = true;
      continue;
    }
    const int64_t b = block_start[q], e = block_start[q + 1], n = offs[q].back();
    double* o = out + outOff[q];
    for (int64_t i = b; i < e; i++)
      for (int c = 0; c < h->fin->lay.rvDim[rv[i]]; c++) {
        const int64_t row = h->fin->lay.rvOff[rv[i]] + c;
        rhs[row] = 1.0;
        HIPCHK(hipMemcpyAsync(h->fin->rhsWork, rhs.data(), nPad * sizeof(double), hipMemcpyHostToDevice, h->str.st));
        rhs[row] = 0.0;
        if (int rc = solveReduced(h)) return rc;
        HIPCHK(hipMemcpyAsync(x.data(), d.xRed, nPad * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
        HIPCHK(hipStreamSynchronize(h->str.st));
        const int64_t col = offs[q][i - b] + c;
        for (int64_t j = b; j < e; j++)
          for (int r = 0; r < h->fin->lay.rvDim[rv[j]]; r++) o[col * n + offs[q][j - b] + r] = x[h->fin->lay.rvOff[rv[j]] + r];
      }
  }
  if (anyInv) {
    if (int rc = selectedInversion(h)) return rc;
    for (int64_t q = 0; q < n_blocks; q++)  // solved blocks: gather anything (their slots are overwritten below)
      if (bySolve[q]) std::fill(gidx.begin() + outOff[q], gidx.begin() + outOff[q + 1], 0);
    const int64_t ng = (int64_t)gidx.size();
    DevOwner m;  // freed at the end of the block, on every path
    int64_t* idxD = nullptr;
    double* valD = nullptr;
    std::vector<double> val(ng);
    if (m.put(&idxD, gidx) || m.get(&valD, ng)) return fail(VB_E_HIP, "covariances: device allocation");
    launch_gather(d.tiles, idxD, ng, valD, h->str.st);
    if (hipMemcpyAsync(val.data(), valD, ng * sizeof(double), hipMemcpyDeviceToHost, h->str.st) != hipSuccess ||
        hipStreamSynchronize(h->str.st) != hipSuccess)
      return fail(VB_E_HIP, "covariances: gather");
    for (int64_t q = 0; q < n_blocks; q++)
      if (!bySolve[q]) std::copy(val.begin() + outOff[q], val.begin() + outOff[q + 1], out + outOff[q]);
  }
  h->run.linearized = false, h->run.factored = false;
  return checkErr(h);
}

int vb_compute_point_covariances(vb_handle h, double damping, int64_t n, const int32_t* points,
                                 const int64_t* with_start, const int32_t* with_kinds, const int32_t* with_handles,
                                 double* out, double* used_damping) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_compute_point_covariances before vb_finalize");
  if (h->prob.partSet || h->prob.sharded) return fail(VB_E_UNSUPPORTED, "covariances run on a single handle");
  if (n < 0 || (n > 0 && (!points || !out))) return fail(VB_E_ARG, "vb_compute_point_covariances: null argument");
  const int64_t nw = (n && with_start) ? with_start[n] : 0;
  if (nw > 0 && (!with_kinds || !with_handles)) return fail(VB_E_ARG, "vb_compute_point_covariances: null argument");
  Dev& d = h->fin->d;
  h->run.pointCovMs[0] = h->run.pointCovMs[1] = h->run.pointCovMs[2] = 0.0;
  if (n == 0) {
    if (used_damping) *used_damping = damping;
    return 0;
  }
  if (!h->fin->sch[0].built) return fail(VB_E_STATE, "no factorization schedule");
  // the requests: landmark of every point, panel columns of the extra variables
  std::vector<int64_t> lmY(d.nPts + 1);
  HIPCHK(hipMemcpy(lmY.data(), d.lmY, lmY.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
  std::vector<int32_t> reqLm(n), xPc;
  std::vector<int64_t> xStart(n + 1, 0), outOff(n + 1, 0);
  for (int64_t q = 0; q < n; q++) {
    if (points[q] < 0 || points[q] >= d.nvar[VB_VAR_POINT]) return fail(VB_E_ARG, "point handle out of range");
    if (h->fin->lmOfPoint[points[q]] < 0) return fail(VB_E_ARG, "covariance of a constant point");
    reqLm[q] = h->fin->lmOfPoint[points[q]];
    if (std::binary_search(h->fin->loneLm.begin(), h->fin->loneLm.end(), reqLm[q]))
      return fail(VB_E_UNSUPPORTED, "covariance of a point that only base-map factors observe");
  }
  if (nw > 0) {
    std::vector<int64_t> lmBlk(d.nPts + 1);
    HIPCHK(hipMemcpy(lmBlk.data(), d.lmBlk, lmBlk.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> blkRed(lmBlk.back()), blkCol(lmBlk.back());
    if (!blkRed.empty()) {
      HIPCHK(hipMemcpy(blkRed.data(), d.blkRed, blkRed.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
      HIPCHK(hipMemcpy(blkCol.data(), d.blkCol, blkCol.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    const std::unordered_map<int64_t, int32_t> rvOf = reducedIndex(h);
    for (int64_t q = 0; q < n; q++) {
      if (with_start[q + 1] < with_start[q] || with_start[q] < 0) return fail(VB_E_ARG, "with_start must be non-decreasing");
      const int64_t l = reqLm[q];
      for (int64_t i = with_start[q]; i < with_start[q + 1]; i++) {
        if (with_kinds[i] == VB_VAR_POINT) return fail(VB_E_ARG, "the extra variables of a point covariance are reduced variables");
        auto it = rvOf.find(((int64_t)with_kinds[i] << 32) | (uint32_t)with_handles[i]);
        if (it == rvOf.end()) return fail(VB_E_ARG, "covariance of a constant or unknown variable");
        // the landmark's blocks are sorted by reduced id
        const auto b0 = blkRed.begin() + lmBlk[l], b1 = blkRed.begin() + lmBlk[l + 1];
        const auto b = std::lower_bound(b0, b1, it->second);
        if (b == b1 || *b != it->second) return fail(VB_E_ARG, "the variable does not observe the point");
        for (int j = 0; j < h->fin->lay.rvDim[it->second]; j++) xPc.push_back(blkCol[b - blkRed.begin()] + j);
      }
      xStart[q + 1] = (int64_t)xPc.size();
    }
  }
  std::vector<int32_t> items, big;
  for (int64_t q = 0; q < n; q++) {
    const int64_t N = 3 + xStart[q + 1] - xStart[q];
    outOff[q + 1] = outOff[q] + N * N;
    const int64_t l = reqLm[q];
    ((lmY[l + 1] - lmY[l]) / 3 <= kLmSmallCols ? items : big).push_back((int32_t)q);
  }
  const int64_t nSmall = (int64_t)items.size(), nBig = (int64_t)big.size();
  items.insert(items.end(), big.begin(), big.end());

  auto now = [] { return std::chrono::steady_clock::now(); };
  auto ms = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
  const auto t0 = now();
  double lam = damping;
  if (int rc = covariancePrologue(h, damping, &lam)) return rc;
  if (used_damping) *used_damping = lam;
  h->run.linearized = false, h->run.factored = false;  // the inversion consumes the factor
  const auto t1 = now();
  if (d.nT > 0)
    if (int rc = selectedInversion(h)) return rc;
  const auto t2 = now();
  {
    DevOwner m;  // freed at the end of the block (inside the third time), on every path
    int32_t *itemsD = nullptr, *reqLmD = nullptr, *xPcD = nullptr;
    int64_t *xStartD = nullptr, *outOffD = nullptr;
    double* outD = nullptr;
    if (m.put(&itemsD, items) || m.put(&reqLmD, reqLm) || m.put(&xPcD, xPc) || m.put(&xStartD, xStart) ||
        m.put(&outOffD, outOff) || m.get(&outD, (size_t)outOff[n]))
      return fail(VB_E_HIP, "point covariances: device allocation");
    launch_pointcov(d, itemsD, nSmall, nBig, reqLmD, xStartD, xPcD, outOffD, outD, h->str.st);
    if (hipMemcpyAsync(out, outD, (size_t)outOff[n] * sizeof(double), hipMemcpyDeviceToHost, h->str.st) != hipSuccess ||
        hipStreamSynchronize(h->str.st) != hipSuccess)
      return fail(VB_E_HIP, "point covariances: kernel failure");
  }
  const auto t3 = now();
  h->run.pointCovMs[0] = ms(t0, t1), h->run.pointCovMs[1] = ms(t1, t2), h->run.pointCovMs[2] = ms(t2, t3);
  return checkErr(h);
}

int vb_point_covariance_times(vb_handle h, double ms[3]) {
  if (!h || !ms) return fail(VB_E_ARG, "vb_point_covariance_times: null argument");
  std::copy(h->run.pointCovMs, h->run.pointCovMs + 3, ms);
  return 0;
}
}  // extern "C"
