// Host driver of the iterative reduced solve (kernels: pcg.hip, lowprec.hip) over its PcgState (host.hpp).
#include "host.hpp"

namespace viba_host {

// ---------------------------------------------------------------- iterative reduced solve
// (Optimizer.cpp:232-331; pcg.hip)
bool pcgMode(vb_handle h) { return h->tune.solverType != VB_SOLVER_DIRECT; }

// device buffers of the PCG path, on first use: the tile list of S x, the five vectors, and the
// preconditioner storage of the selected type
int pcgPrepare(vb_handle h) {
  const Finalized& f = *h->fin;
  const Dev& d = f.d;
  if (h->prob.partSet || h->prob.sharded)
    return fail(VB_E_UNSUPPORTED, "the PCG solvers run on a single handle (no landmark shards, no partition)");
  const int64_t nPad = (int64_t)d.nT * TS;
  // a new group, or the handle's to grow; installed again only when every request succeeded
  std::unique_ptr<PcgState> p = std::move(h->pcg);
  const bool fresh = !p;
  if (fresh) p = std::make_unique<PcgState>();
  DevOwner& m = p->mem;
  bool ok = true;
  if (fresh) {
    std::vector<int32_t> tl, rc;
    for (int32_t J = 0; J < d.nT; J++)
      for (int64_t c = f.colStart[J]; c < f.colStart[J + 1]; c++)
        if (!f.tileFill[f.colTilesH[c]]) tl.push_back(f.colTilesH[c]), rc.push_back(f.colRowsH[c]), rc.push_back(J);
    p->nSymv = (int64_t)tl.size();
    ok = !(m.put(&p->symvTilesD, tl) || m.put(&p->symvRCD, rc) || m.zeroed(&p->pcgR, nPad) || m.zeroed(&p->pcgZ, nPad) ||
           m.zeroed(&p->pcgP, nPad) || m.zeroed(&p->pcgAp, nPad) || m.zeroed(&p->pcgB, nPad));
  }
  if (ok && h->tune.solverType == VB_SOLVER_PCG_JACOBI && !p->jacL) ok = !m.zeroed(&p->jacL, nPad * 32);
  if (ok && h->tune.solverType == VB_SOLVER_PCG_GAUSS_SEIDEL && !p->tilesGS) ok = !m.zeroed(&p->tilesGS, d.nTiles * TS * TS);
  if (ok && h->tune.solverType == VB_SOLVER_PCG_LOWER_PREC && !p->lpTiles)
    ok = !(m.zeroed(&p->lpTiles, d.nTiles * TS * TS) || m.zeroed(&p->lpLinv, (size_t)d.nT * TS * TS) ||
           m.zeroed(&p->lpT, nPad));
  if (!ok) return devFail(m, "PCG buffers");  // (the whole group goes with p: the next call starts over)
  h->pcg = std::move(p);
  return 0;
}

// LowerPrecSolvePrecond::init (Preconditioner.h:180-218): S cast to fp32 and factored by the direct
// solver's tile schedule in fp32 (lowprec.hip); while the fp32 sum of the factor is not finite (a
// non-finite entry, or finite entries whose sum overflows), redo it from S with the diagonal raised:
// epsilon 0, then 1e-8, then x3 per attempt
int lpInit(vb_handle h) {
  Dev& d = h->fin->d;
  PcgState& p = *h->pcg;
  const Sched& S = h->fin->sch[0];
  const int64_t nEl = d.nTiles * TS * TS;
  float eps = 0.0f;
  for (int attempt = 0; attempt < 200; attempt++) {
    launch_lp_cast(d.tiles, p.lpTiles, nEl, h->str.st);
    if (eps > 0) {
      launch_lp_damp(p.lpTiles, d.tileIdx, d.nT, d.rvOff, d.rvDim, d.nRV, eps, h->str.st);
      eps *= 3.0f;
    } else {
      eps = 1e-8f;
    }
    for (int32_t L = 0; L < S.nLevels; L++) {
      const int64_t p0 = S.lvP[L], t0 = S.lvT[L], u0 = S.lvU[L];
      launch_lp_factor_level(p.lpTiles, S.updD + 4 * u0, (int)(S.lvU[L + 1] - u0), S.fanPairsD, S.potrfTileD + p0,
                             S.potrfColD + p0, (int)(S.lvP[L + 1] - p0), S.trsmTargetD + t0, S.trsmColD + t0,
                             (int)(S.lvT[L + 1] - t0), p.lpLinv, h->str.st);
    }
    // err[3]: a non-finite factor entry; err[2] (as fp32): the factor's sum (Preconditioner.h:216-218)
    HIPCHK(hipMemsetAsync(d.err + 2, 0, 2 * sizeof(int32_t), h->str.st));
    launch_lp_nonfinite(p.lpTiles, nEl, d.err + 3, reinterpret_cast<float*>(d.err + 2), h->str.st);
    int32_t w[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(w, d.err + 2, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
    HIPCHK(hipStreamSynchronize(h->str.st));
    float sum;
    std::memcpy(&sum, &w[0], sizeof(float));
    if (!w[1] && std::isfinite(sum)) return 0;
  }
  return fail(VB_E_NUMERIC, "LowerPrecSolvePrecond: the fp32 factor keeps breaking down");
}

// LowerPrecSolvePrecond::operator() (Preconditioner.h:215-237): z = (L L^T)^-1 r in fp32
void lpApply(vb_handle h, const double* r, double* z) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  PcgState& p = *h->pcg;
  const Sched& S = f.sch[0];
  const int64_t n = (int64_t)d.nT * TS;
  launch_lp_cast(r, p.lpT, n, h->str.st);
  for (int32_t L = 0; L < S.nLevels; L++) {
    const int64_t p0 = S.lvP[L], t0 = S.lvT[L];
    launch_lp_fwd_level(p.lpTiles, S.potrfColD + p0, (int)(S.lvP[L + 1] - p0), S.trsmTargetD + t0, S.trsmColD + t0,
                        S.trsmRowD + t0, (int)(S.lvT[L + 1] - t0), p.lpLinv, p.lpT, h->str.st);
  }
  for (int32_t L = S.nLevels - 1; L >= 0; L--) {
    const int64_t p0 = S.lvP[L];
    launch_lp_bwd_level(p.lpTiles, f.colStartD, f.colTilesD, f.colRowsD, S.potrfColD + p0, (int)(S.lvP[L + 1] - p0),
                        p.lpLinv, p.lpT, h->str.st);
  }
  launch_lp_uncast(p.lpT, z, n, h->str.st);
}

// Preconditioner::init on the assembled (damped) S
int precondInit(vb_handle h) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  if (int rc = pcgPrepare(h)) return rc;
  if (h->tune.solverType == VB_SOLVER_PCG_JACOBI) {
    launch_jacobi_init(d, h->pcg->jacL, h->str.st);
  } else if (h->tune.solverType == VB_SOLVER_PCG_GAUSS_SEIDEL) {
    // pseudo-factor (BaSpaCho pseudoFactorFrom, Preconditioner.h:125-133): every diagonal tile
    // factored, every off-diagonal tile times L_JJ^-T, no Schur updates -- so all columns at once
    HIPCHK(hipMemcpyAsync(h->pcg->tilesGS, d.tiles, (size_t)d.nTiles * TS * TS * sizeof(double), hipMemcpyDeviceToDevice,
                          h->str.st));
    Dev g = d;
    g.tiles = h->pcg->tilesGS;
    const Sched& S = f.sch[0];
    launch_potrf(g, S.potrfTileD, S.potrfColD, (int)S.lvP[S.nLevels], f.dinv, h->str.st);
    launch_trsm(g, S.trsmDiagD, S.trsmTargetD, S.trsmColD, (int)S.lvT[S.nLevels], f.dinv, h->str.st);
    launch_diag_inverse(g, S.potrfColD, S.lvP[S.nLevels], f.linv, h->str.st);
  } else if (h->tune.solverType == VB_SOLVER_PCG_LOWER_PREC) {
    return lpInit(h);
  }
  return 0;
}

// z = M^-1 r (Preconditioner::operator())
int precondApply(vb_handle h, const double* r, double* z) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  PcgState& p = *h->pcg;
  const size_t bytes = (size_t)d.nT * TS * sizeof(double);
  if (h->tune.solverType == VB_SOLVER_PCG_GAUSS_SEIDEL) {
    HIPCHK(hipMemcpyAsync(p.pcgB, r, bytes, hipMemcpyDeviceToDevice, h->str.st));
    Dev g = d;
    g.tiles = p.tilesGS;
    const Sched& S = f.sch[0];
    launch_solve_fanout(g, S.tasksFD, S.nF, S.tasksBD, S.nB, S.expFD, S.expBD, f.colTilesD, f.colRowsD, f.rowTilesD,
                        f.rowColD, f.linv, p.pcgB, f.yvec, z, f.solveFlags, h->tune.numCUs, h->str.st, 3,
                        nullptr, 0);
    return 0;
  }
  if (h->tune.solverType == VB_SOLVER_PCG_LOWER_PREC) {
    lpApply(h, r, z);
    return 0;
  }
  HIPCHK(hipMemcpyAsync(z, r, bytes, hipMemcpyDeviceToDevice, h->str.st));
  if (h->tune.solverType == VB_SOLVER_PCG_JACOBI) launch_jacobi_apply(d, p.jacL, r, z, h->str.st);
  return 0;
}

// PCG::solve (PCG.cpp:15-104): S x = rhsWork -> xRed, x_0 = 0; stops when |r_k+1| / |r_0| is below
// pcgDesiredResidual or after pcgMaxIterations products.  alpha, beta and the stop test live on the
// device (red[32] = p.Ap, red[33] = r.r, red[36 + (k & 1)] = z.r of iteration k, red[40..42] the stop
// slot, pcg.hip); the host queues kPcgBatch iterations between reads of the stop slot.  Iterations
// queued after the stop leave x, r and p alone (their products and dots are skipped or discarded).
// z = M^-1 r of the last iteration is computed before the test, one preconditioner application the
// reference does not make (it changes nothing returned).  The Gauss-Seidel preconditioner (two
// fan-out triangular solves) costs more than a host read, so it reads every iteration.
int pcgSolve(vb_handle h) {
  Finalized& f = *h->fin;
  Dev& d = f.d;
  const int64_t n = (int64_t)d.nT * TS;
  const size_t bytes = (size_t)n * sizeof(double);
  double* x = d.xRed;
  double *r = h->pcg->pcgR, *z = h->pcg->pcgZ, *p = h->pcg->pcgP, *Ap = h->pcg->pcgAp;
  const int batch = h->tune.solverType == VB_SOLVER_PCG_GAUSS_SEIDEL ? 1 : 8;
  HIPCHK(hipMemsetAsync(x, 0, bytes, h->str.st));
  HIPCHK(hipMemsetAsync(Ap, 0, bytes, h->str.st));
  HIPCHK(hipMemcpyAsync(r, f.rhsWork, bytes, hipMemcpyDeviceToDevice, h->str.st));
  if (int rc = precondApply(h, r, z)) return rc;
  HIPCHK(hipMemcpyAsync(p, z, bytes, hipMemcpyDeviceToDevice, h->str.st));
  HIPCHK(hipMemsetAsync(d.red + 32, 0, 12 * sizeof(double), h->str.st));
  launch_dot(r, r, n, d.red + 33, h->str.st);
  launch_dot(z, r, n, d.red + 36, h->str.st);
  double r02 = 0;
  if (int rc = readRed(h, &r02, 33, 1)) return rc;
  const double r0 = std::sqrt(r02);
  HIPCHK(hipMemsetAsync(d.red + 33, 0, sizeof(double), h->str.st));
  for (int k = 0;; k++) {
    const int zr = 36 + (k & 1), zrNew = 36 + ((k + 1) & 1);
    profBegin(h, KF_SYMV);
    launch_tile_symv(d.tiles, h->pcg->symvTilesD, h->pcg->symvRCD, h->pcg->nSymv, p, Ap, d.red + 40, h->str.st);
    profEnd(h, KF_SYMV);
    launch_dot(p, Ap, n, d.red + 32, h->str.st);
    launch_pcg_xr(x, r, p, Ap, d.red, zr, 32, n, d.red + 33, h->str.st);
    launch_pcg_check(d.red, r0, h->tune.pcgTol, k, h->tune.pcgMaxIt, zrNew, h->str.st);
    if (int rc = precondApply(h, r, z)) return rc;
    launch_dot(z, r, n, d.red + zrNew, h->str.st);
    launch_pcg_p(p, Ap, z, d.red, zrNew, zr, n, h->str.st);
    if ((k + 1) % batch == 0 || k + 1 >= h->tune.pcgMaxIt) {
      double stop[3];
      if (int rc = readRed(h, stop, 40, 3)) return rc;
      if (stop[0] != 0.0) {
        h->run.pcgIters = (int32_t)stop[1], h->run.pcgRelRes = stop[2];
        return checkErr(h);
      }
      if (k + 1 >= h->tune.pcgMaxIt) return fail(VB_E_HIP, "PCG: no stop after pcgMaxIterations");
    }
  }
}

}  // namespace viba_host
