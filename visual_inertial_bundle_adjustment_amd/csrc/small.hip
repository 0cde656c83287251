// Kernels of the thirteen small (non-visual) factor kinds (gfx950): inertial (InertialFactor.cpp:23-305), omega
// priors (OmegaPriorFactor.cpp), random walks (RandomWalkFactor.cpp) and priors (PriorFactor.cpp).
//   small_eval<FK, Report>        one lane per factor: residual, Jacobian blocks into the factor's staging slot
//   small_kernel<LO, HI>          the LM loop's evaluation of kinds [LO, HI]: linearization (staged) or cost
//   small_assemble_kernel<MM>     one wave per staged factor: whitened by the precision's Cholesky factor,
//                                 gradient and Gauss-Newton block into the reduced tiles with fp64 atomics
//   small_report_kernel           residual report (report.hpp), the evaluate-only instantiation
//   small_expected_eval_kernel,   singleExpectedDelta along a step (inspect.hpp) from a staging of the
//   small_expected_dot_kernel     inspection's own
// and their launchers.  The kernels over kinds pick small_eval's instantiation through small_dispatch.
#include "factor_eval.hpp"
#include "inspect.hpp"
#include "report.hpp"
#include <type_traits>

namespace viba {

constexpr int kMaxM = kSmallRows;
constexpr int kMaxCols = kSmallCols;

// J points into the factor's staging slot (HBM): the evaluation writes its Jacobian blocks there
// directly instead of into a 15 KB per-thread scratch array
struct SmallEval {
  int m = 0;
  int nslot = 0;
  int col[10], dim[10], red[10];
  double e[kMaxM];
  double (*J)[kMaxCols];
};

// InertialFactor::operator() (InertialFactor.cpp:23-123). Jacobian blocks written into E.J at
// columns c[0..4] (calib, Tp, vp, Tn, vn); a column offset < 0 skips that block.
__device__ void inertial_eval(const double* c, const double* calib, const ImuIdx& jac, const se3& Tp, v3 vp,
                              const se3& Tn, v3 vn, v3 g, SmallEval& E, const int cols[5]) {
  const int n = jac.size;
  const double dt = c[10];
  // corr = J_calib * boxMinus(calib, calib at preintegration): the error-state entries in the
  // ImuJacInd order (bias g / a, scale g / a, nonorth g / a, time offsets), enabled blocks only, each
  // consumed as it is formed (a compacted boxMinus array indexed at run time lived in scratch)
  double corr[9];
#pragma unroll
  for (int i = 0; i < 9; i++) corr[i] = 0.0;
  {
    const double* r = c + 11 + 207 + 81;
    const double* Jc = c + 11;
    auto take = [&](double v) {
#pragma unroll
      for (int i = 0; i < 9; i++) corr[i] += Jc[i] * v;
      Jc += 9;
    };
    if (jac.gB >= 0)
#pragma unroll
      for (int i = 0; i < 3; i++) take(calib[6 + i] - r[6 + i]);
    if (jac.aB >= 0)
#pragma unroll
      for (int i = 0; i < 3; i++) take(calib[9 + i] - r[9 + i]);
    if (jac.gS >= 0)
#pragma unroll
      for (int i = 0; i < 3; i++) take(1.0 / calib[i] - 1.0 / r[i]);
    if (jac.aS >= 0)
#pragma unroll
      for (int i = 0; i < 3; i++) take(1.0 / calib[3 + i] - 1.0 / r[3 + i]);
    if (jac.gN >= 0) {
      constexpr int kG[6] = {3, 6, 1, 7, 2, 5};  // col-major (0,1) (0,2) (1,0) (1,2) (2,0) (2,1)
#pragma unroll
      for (int i = 0; i < 6; i++) take(calib[12 + kG[i]] - r[12 + kG[i]]);
    }
    if (jac.aN >= 0) {
      constexpr int kA[3] = {3, 6, 7};  // (0,1) (0,2) (1,2)
#pragma unroll
      for (int i = 0; i < 3; i++) take(calib[21 + kA[i]] - r[21 + kA[i]]);
    }
    if (jac.rT >= 0) take(calib[31] - r[31]);
    if (jac.gaT >= 0) take((calib[30] - calib[31]) - (r[30] - r[31]));
  }
  q4 Rc = qexp(mk(-corr[0], -corr[1], -corr[2]));
  q4 cR = qmul(Rc, qinv(q4{c[0], c[1], c[2], c[3]}));
  q4 Rerr = qmul(qmul(cR, Tp.R), qinv(Tn.R));
  v3 lre = neg(qlog(Rerr));
  v3 dVp = qrot(Tp.R, sub(sub(vn, vp), scl(dt, g)));
  v3 velErr = add(sub(mk(c[4], c[5], c[6]), dVp), mk(corr[3], corr[4], corr[5]));
  q4 Rpn = qmul(Tp.R, qinv(Tn.R));
  v3 dPp = sub(sub(Tp.t, qrot(Rpn, Tn.t)), qrot(Tp.R, add(scl(dt, vp), scl(0.5 * dt * dt, g))));
  v3 posErr = add(sub(mk(c[7], c[8], c[9]), dPp), mk(corr[6], corr[7], corr[8]));
  E.e[0] = lre.x, E.e[1] = lre.y, E.e[2] = lre.z;
  E.e[3] = velErr.x, E.e[4] = velErr.y, E.e[5] = velErr.z;
  E.e[6] = posErr.x, E.e[7] = posErr.y, E.e[8] = posErr.z;
  m3 dL = so3_leftJacInv(neg(lre));
  m3 Rp = qmat(Tp.R);
  if (cols[1] >= 0) {
    const int c0 = cols[1];
    m3 A = mmul(dL, qmat(cR));
    m3 hv = hat(dVp), hp = hat(dPp);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        E.J[i][c0 + j] = 0.0, E.J[i][c0 + 3 + j] = -A.a[i][j];
        E.J[3 + i][c0 + j] = 0.0, E.J[3 + i][c0 + 3 + j] = hv.a[i][j];
        E.J[6 + i][c0 + j] = (i == j) ? -1.0 : 0.0, E.J[6 + i][c0 + 3 + j] = hp.a[i][j];
      }
  }
  if (cols[2] >= 0) {
    const int c0 = cols[2];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        E.J[i][c0 + j] = 0.0;
        E.J[3 + i][c0 + j] = Rp.a[i][j];
        E.J[6 + i][c0 + j] = Rp.a[i][j] * dt;
      }
  }
  if (cols[3] >= 0) {
    const int c0 = cols[3];
    m3 A = mmul(dL, qmat(Rerr));
    m3 Rm = qmat(Rpn);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        E.J[i][c0 + j] = 0.0, E.J[i][c0 + 3 + j] = A.a[i][j];
        E.J[3 + i][c0 + j] = 0.0, E.J[3 + i][c0 + 3 + j] = 0.0;
        E.J[6 + i][c0 + j] = Rm.a[i][j], E.J[6 + i][c0 + 3 + j] = 0.0;
      }
  }
  if (cols[4] >= 0) {
    const int c0 = cols[4];
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        E.J[i][c0 + j] = 0.0;
        E.J[3 + i][c0 + j] = -Rp.a[i][j];
        E.J[6 + i][c0 + j] = 0.0;
      }
  }
  if (cols[0] >= 0) {
    const int c0 = cols[0];
    m3 dR = mmul(dL, so3_leftJac(mk(-corr[0], -corr[1], -corr[2])));
    for (int j = 0; j < n; j++) {
      const double j0 = c[11 + j * 9], j1 = c[11 + j * 9 + 1], j2 = c[11 + j * 9 + 2];
      for (int i = 0; i < 3; i++) E.J[i][c0 + j] = dR.a[i][0] * j0 + dR.a[i][1] * j1 + dR.a[i][2] * j2;
      for (int i = 3; i < 9; i++) E.J[i][c0 + j] = c[11 + j * 9 + i];
    }
  }
}

// SecondaryImuInertialFactor::SecondaryState (InertialFactor.cpp:136-181)
struct SecState {
  v3 t_b_i, v_b, vw;
  q4 R_w_b;
  se3 T_iw;
};
__device__ SecState sec_state(const se3& Tbw, v3 vel, v3 om, const se3& Tib) {
  SecState s;
  s.t_b_i = se3_inv(Tib).t;
  s.v_b = cross(om, s.t_b_i);
  s.R_w_b = qinv(Tbw.R);
  s.T_iw = se3_mul(Tib, Tbw);
  s.vw = add(vel, qrot(s.R_w_b, s.v_b));
  return s;
}
// compose the 9x6 / 9x3 Jacobians at columns (cT, cV) of `J` (wrt imu pose/vel) into the body
// state blocks at columns oT, oV, oO, oE (each < 0 to skip; oE accumulates when addE)
__device__ void sec_compose(const SecState& s, v3 om, const se3& Tib, double (*J)[kMaxCols], int cT, int cV,
                            int oT, int oV, int oO, int oE, bool addE) {
  m3 RA = qmat(s.R_w_b);
  double JT[9][6], Jv[9][3];
  for (int i = 0; i < 9; i++) {
    for (int j = 0; j < 6; j++) JT[i][j] = J[i][cT + j];
    for (int j = 0; j < 3; j++) Jv[i][j] = J[i][cV + j];
  }
  if (oT >= 0) {
    double A[36];
    se3_Adj(Tib, A);
    m3 dv = mmul(RA, hat(s.v_b));  // RA * (-hat(-v_b))
    for (int i = 0; i < 9; i++)
      for (int j = 0; j < 6; j++) {
        double x = 0;
        for (int k = 0; k < 6; k++) x += JT[i][k] * A[k * 6 + j];
        if (j >= 3) x += Jv[i][0] * dv.a[0][j - 3] + Jv[i][1] * dv.a[1][j - 3] + Jv[i][2] * dv.a[2][j - 3];
        J[i][oT + j] = x;
      }
  }
  if (oO >= 0) {
    m3 B = mmul(RA, hat(neg(s.t_b_i)));
    for (int i = 0; i < 9; i++)
      for (int j = 0; j < 3; j++)
        J[i][oO + j] = Jv[i][0] * B.a[0][j] + Jv[i][1] * B.a[1][j] + Jv[i][2] * B.a[2][j];
  }
  if (oE >= 0) {
    m3 B = mmul(mmul(RA, hat(om)), mT(qmat(Tib.R)));  // times -1 below
    for (int i = 0; i < 9; i++)
      for (int j = 0; j < 6; j++) {
        double x = JT[i][j];
        if (j < 3) x -= Jv[i][0] * B.a[0][j] + Jv[i][1] * B.a[1][j] + Jv[i][2] * B.a[2][j];
        J[i][oE + j] = addE ? J[i][oE + j] + x : x;
      }
  }
  if (oV >= 0)
    for (int i = 0; i < 9; i++)
      for (int j = 0; j < 3; j++) J[i][oV + j] = Jv[i][j];
}

struct SmallArgs {
  int64_t n;
  const int32_t* vars;
  const double* consts;
  int nc;
  int mode;  // 0: grad+hess, 1: grad only (into gOut), 2: cost
  double* gOut;
};

__device__ inline int tdim_of(const Dev& d, int kind, int h) {
  switch (kind) {
    case 0: case 2: case 3: return 3;
    case 1: case 5: case 7: return 6;
    case 4: {
      const double* c = d.var[4] + (int64_t)h * 24;
      return (int)c[1] + (c[7] != 0.0 ? 1 : 0) + (c[8] != 0.0 ? 1 : 0);
    }
    case 6: return d.jac.size;
  }
  return 0;
}

__device__ inline double* tile_addr(const Dev& d, int64_t r, int64_t c) {
  const int T = d.T;
  const int32_t ti = d.tileIdx[(r / T) * d.nT + (c / T)];
  return d.tiles + (int64_t)ti * T * T + (c % T) * T + (r % T);
}

// kinds of the factor arguments (reference functor order)
__constant__ int kFK[14][10] = {
    {0, 1, 5, 4, 2}, {6, 1, 2, 1, 2, 8}, {6, 1, 2, 3, 1, 2, 3, 7, 8}, {6, 1, 2, 3, 7, 1, 2, 3, 7, 8},
    {3, 7}, {6, 6}, {4, 4}, {7, 7}, {5, 5}, {1}, {6}, {4}, {5}, {7}};
// their number: the row lengths of kFK
constexpr int small_nv(int fk) { return fk == 0 ? 5 : fk == 1 ? 6 : fk == 2 ? 9 : fk == 3 ? 10 : fk <= 8 ? 2 : 1; }

// evaluation of factor k of kind FK (k >= a.n: nothing); returns this lane's cost term
// Report (the residual report, small_report_kernel): evaluate only -- the residual as the functor returns
// it (rawError, Factor.h:172-232; the calibration kinds' enabled entries compacted, zero-filled), half its
// squared norm, half the squared whitened norm and singleCost go to row k - rep->first of rep; no staging,
// meta or Jacobian is written (a.mode is 2 there).  The other instantiation is untouched by it.
template <int FK, bool Report = false>
__device__ __forceinline__ double small_eval(const Dev& d, const SmallArgs& a, int64_t k, const RepRows* rep = nullptr) {
  double acc[1] = {0.0};
  constexpr int mRows = (FK >= 1 && FK <= 3) ? 9 : FK == 4 ? 3 : (FK == 5 || FK == 10) ? 23 : (FK == 6 || FK == 11) ? 17 : 6;
  constexpr bool kCompact = FK == 5 || FK == 10 || FK == 6 || FK == 11;  // Report: raw rows written in the kind's loop
  if (!Report && a.mode != 2) {
    // the wave's 64 staging slots (consecutive factors) zeroed over their first mRows rows with the
    // lanes on consecutive 16 B: one factor's rows zeroed per lane made every store instruction 64
    // scattered 8-byte writes
    const int lane = threadIdx.x & 63;
    const int64_t k0 = k - lane, ns = a.n - k0 < 64 ? a.n - k0 : 64;
    typedef double zd2 __attribute__((ext_vector_type(2)));
    for (int64_t q = 0; q < ns; q++) {
      zd2* base = (zd2*)(d.sJ + (d.sf[FK].stage + k0 + q) * kSmallJ);
      for (int e = lane; e < mRows * kMaxCols / 2; e += 64) base[e] = zd2{0.0, 0.0};
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");  // before the lanes' own Jacobian stores
    __builtin_amdgcn_wave_barrier();
  }
  if (k < a.n) {
    SmallEval E;
    const int64_t slot = d.sf[FK].stage + k;
    E.J = Report ? nullptr : (double(*)[kMaxCols])(d.sJ + slot * kSmallJ);
    constexpr int nv = small_nv(FK);
    const int32_t* vi = a.vars + k * nv;
    const double* c = a.consts + k * a.nc;
    // column layout: every non-gravity slot gets columns (also constant ones: simpler eval)
    int colc = 0;
    E.nslot = nv;
#pragma unroll
    for (int s = 0; s < nv; s++) {
      const int kind = kFK[FK][s], h = vi[s];
      if (kind == 8 || h < 0) {
        E.col[s] = -1, E.dim[s] = 0, E.red[s] = -1;
        continue;
      }
      E.dim[s] = tdim_of(d, kind, h);
      E.col[s] = colc;
      colc += E.dim[s];
      E.red[s] = d.redOf[kind][h];
    }
    bool whiten = false;
    const double* U = nullptr;
    bool useImuLoss = false;
    if (FK == 1 || FK == 2 || FK == 3) {
      E.m = 9;
      whiten = true;
      U = c + 331;
      useImuLoss = true;
      const double* gd = d.var[8] + (int64_t)vi[nv - 1] * 4;
      v3 g = mk(gd[0], gd[1], gd[2]);
      const double* calib = d.var[6] + (int64_t)vi[0] * 32;
      // the cost pass (mode 2) forms the residual only: every Jacobian block is skipped (a block with
      // column < 0 is not formed), which halves the IMU kinds' serial chain per lane
      const bool wantJ = a.mode != 2;
      if (FK == 1) {
        int cols[5] = {E.col[0], E.col[1], E.col[2], E.col[3], E.col[4]};
        if (!wantJ)
#pragma unroll
          for (int q = 0; q < 5; q++) cols[q] = -1;
        inertial_eval(c, calib, d.jac, se3_load(d.var[1] + (int64_t)vi[1] * 7), mk3(d.var[2], vi[2]),
                      se3_load(d.var[1] + (int64_t)vi[3] * 7), mk3(d.var[2], vi[4]), g, E, cols);
      } else {
        // slots: split  [c, pT, pV, pO, pE, nT, nV, nO, nE, g]
        //        common [c, pT, pV, pO, nT, nV, nO, E, g]
        const bool split = FK == 3;
        const int spT = 1, spV = 2, spO = 3, spE = split ? 4 : 7;
        const int snT = split ? 5 : 4, snV = split ? 6 : 5, snO = split ? 7 : 6, snE = split ? 8 : 7;
        se3 pT = se3_load(d.var[1] + (int64_t)vi[spT] * 7), nT = se3_load(d.var[1] + (int64_t)vi[snT] * 7);
        se3 pE = se3_load(d.var[7] + (int64_t)vi[spE] * 7), nE = se3_load(d.var[7] + (int64_t)vi[snE] * 7);
        v3 pV = mk3(d.var[2], vi[spV]), nV = mk3(d.var[2], vi[snV]);
        v3 pO = mk3(d.var[3], vi[spO]), nO = mk3(d.var[3], vi[snO]);
        SecState ps = sec_state(pT, pV, pO, pE), ns = sec_state(nT, nV, nO, nE);
        // primary-factor blocks in scratch columns after the slot columns
        const int sc = colc;  // pT 6, pV 3, nT 6, nV 3 => 18 scratch columns
        int cols[5] = {E.col[0], sc, sc + 6, sc + 9, sc + 15};
        if (!wantJ)
#pragma unroll
          for (int q = 0; q < 5; q++) cols[q] = -1;
        inertial_eval(c, calib, d.jac, ps.T_iw, ps.vw, ns.T_iw, ns.vw, g, E, cols);
        if (wantJ) {
          sec_compose(ps, pO, pE, E.J, sc, sc + 6, E.col[spT], E.col[spV], E.col[spO], E.col[spE], false);
          sec_compose(ns, nO, nE, E.J, sc + 9, sc + 15, E.col[snT], E.col[snV], E.col[snO], E.col[snE], !split);
        }
      }
    } else if (FK == 4) {  // omega prior
      E.m = 3;
      const double sig = c[3];
      v3 om = mk3(d.var[3], vi[0]);
      v3 wI = mk(c[0], c[1], c[2]);
      v3 r;
      if (vi[1] < 0) {
        r = scl(1.0 / sig, sub(om, wI));
      } else {
        se3 Tib = se3_load(d.var[7] + (int64_t)vi[1] * 7);
        r = scl(1.0 / sig, sub(om, qrot(qinv(Tib.R), wI)));
        // -R^T * (-hat(-w)) / sig = -R^T hat(w) / sig
        if constexpr (!Report) {
          m3 B = mmul(mT(qmat(Tib.R)), hat(wI));
          for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) E.J[i][E.col[1] + j] = 0.0, E.J[i][E.col[1] + 3 + j] = -B.a[i][j] / sig;
        }
      }
      if constexpr (!Report)
        for (int i = 0; i < 3; i++) E.J[i][E.col[0] + i] = 1.0 / sig;
      E.e[0] = r.x, E.e[1] = r.y, E.e[2] = r.z;
    } else if (FK == 5 || FK == 10) {  // imu calib RW / prior (residual padded to 23)
      // rows in the canonical error-state order (a disabled block leaves zero rows: J^T J and J^T e
      // do not depend on the row order), columns / weights at the compact index j -- every register
      // index static (a compacted residual array indexed at run time lived in scratch)
      E.m = 23;
      const double* v = d.var[6] + (int64_t)vi[FK == 5 ? 1 : 0] * 32;
      const double* r = FK == 5 ? d.var[6] + (int64_t)vi[0] * 32 : c;
      const ImuIdx& jc = d.jac;
      const bool on[8] = {jc.gB >= 0, jc.aB >= 0, jc.gS >= 0, jc.aS >= 0, jc.gN >= 0, jc.aN >= 0, jc.rT >= 0, jc.gaT >= 0};
      constexpr int kBlk[23] = {0, 0, 0, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4, 4, 4, 4, 4, 5, 5, 5, 6, 7};
      constexpr int kNo[9] = {3, 6, 1, 7, 2, 5, 3, 6, 7};  // gN (col-major), then aN
      int j = 0;
#pragma unroll
      for (int q = 0; q < 23; q++) {
        E.e[q] = 0.0;
        if (!on[kBlk[q]]) continue;
        double dv;
        if (q < 3) dv = v[6 + q] - r[6 + q];
        else if (q < 6) dv = v[9 + q - 3] - r[9 + q - 3];
        else if (q < 9) dv = 1.0 / v[q - 6] - 1.0 / r[q - 6];
        else if (q < 12) dv = 1.0 / v[3 + q - 9] - 1.0 / r[3 + q - 9];
        else if (q < 18) dv = v[12 + kNo[q - 12]] - r[12 + kNo[q - 12]];
        else if (q < 21) dv = v[21 + kNo[q - 12]] - r[21 + kNo[q - 12]];
        else if (q == 21) dv = v[31] - r[31];
        else dv = (v[30] - v[31]) - (r[30] - r[31]);
        if (FK == 5) {
          E.e[q] = dv * c[j];
          if constexpr (!Report) {
            E.J[q][E.col[0] + j] = -c[j];
            E.J[q][E.col[1] + j] = c[j];
          }
        } else {
          const double sq = sqrt(c[32 + j]);
          E.e[q] = dv * sq;
          if constexpr (!Report) E.J[q][E.col[0] + j] = sq;
        }
        if constexpr (Report)
          if (rep->raw) rep->raw[(k - rep->first) * mRows + j] = E.e[q];
        j++;
      }
      if constexpr (Report)
        if (rep->raw)
          for (; j < mRows; j++) rep->raw[(k - rep->first) * mRows + j] = 0.0;
    } else if (FK == 6 || FK == 11) {  // cam intrinsics RW / prior (residual padded to 17)
      // rows: projection parameter q (q < np), 15 readout, 16 time offset (as above: static indices)
      E.m = 17;
      const double* v = d.var[4] + (int64_t)vi[FK == 6 ? 1 : 0] * 24;
      const double* b = FK == 6 ? d.var[4] + (int64_t)vi[0] * 24 : c;
      const int np = (int)v[1];
      int j = 0;
#pragma unroll
      for (int q = 0; q < 17; q++) {
        E.e[q] = 0.0;
        const bool on = q < 15 ? q < np : q == 15 ? v[7] != 0.0 : v[8] != 0.0;
        if (!on) continue;
        const double dv = q < 15 ? v[9 + q] - b[9 + q] : q == 15 ? v[5] - b[5] : v[6] - b[6];
        const double sq = FK == 6 ? c[j] : sqrt(c[24 + j]);
        E.e[q] = dv * sq;
        if constexpr (!Report) {
          if (FK == 6) {
            E.J[q][E.col[0] + j] = -sq;
            E.J[q][E.col[1] + j] = sq;
          } else {
            E.J[q][E.col[0] + j] = sq;
          }
        }
        if constexpr (Report)
          if (rep->raw) rep->raw[(k - rep->first) * mRows + j] = E.e[q];
        j++;
      }
      if constexpr (Report)
        if (rep->raw)
          for (; j < mRows; j++) rep->raw[(k - rep->first) * mRows + j] = 0.0;
    } else {  // SE3 RW (7, 8), pose prior (9), SE3 priors (12, 13)
      E.m = 6;
      const int vk = (FK == 7 || FK == 13) ? 7 : (FK == 9 ? 1 : 5);
      se3 err;
      double sq[6];
      if (FK == 7 || FK == 8) {
        err = se3_mul(se3_load(d.var[vk] + (int64_t)vi[1] * 7), se3_inv(se3_load(d.var[vk] + (int64_t)vi[0] * 7)));
        for (int i = 0; i < 6; i++) sq[i] = c[i];
      } else {
        err = se3_mul(se3_load(d.var[vk] + (int64_t)vi[0] * 7), se3_inv(se3_load(c)));
        for (int i = 0; i < 6; i++) sq[i] = FK == 9 ? 1.0 : sqrt(c[7 + i]);
      }
      double lg[6], Ji[36];
      se3_log(err, lg);
      if constexpr (!Report) se3_leftJacInv(lg, Ji);
      for (int i = 0; i < 6; i++) E.e[i] = lg[i] * sq[i];
      if constexpr (!Report) {
        const int cn = (FK == 7 || FK == 8) ? E.col[1] : E.col[0];
        for (int i = 0; i < 6; i++)
          for (int j = 0; j < 6; j++) E.J[i][cn + j] = sq[i] * Ji[i * 6 + j];
        if (FK == 7 || FK == 8) {
          double A[36];
          se3_Adj(err, A);
          for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
              double x = 0;
              for (int q = 0; q < 6; q++) x += Ji[i * 6 + q] * A[q * 6 + j];
              E.J[i][E.col[0] + j] = -sq[i] * x;
            }
        }
      }
      if (FK == 9) {
        whiten = true;
        U = c + 43;
      }
    }
    // whitening of the residual by a square root U of the precision (P = U^T U, row-major m x m);
    // the Jacobian is whitened by small_assemble_kernel.  m is the kind's residual size (E.m), a
    // compile-time bound so E.e stays in registers
    constexpr int m = mRows;
    if constexpr (Report) {
      const int64_t row = k - rep->first;
      double su = 0;
#pragma unroll
      for (int i = 0; i < m; i++) su += E.e[i] * E.e[i];
      if (rep->squ) rep->squ[row] = 0.5 * su;
      if (!kCompact && rep->raw)
#pragma unroll
        for (int i = 0; i < m; i++) rep->raw[row * m + i] = E.e[i];
    }
    if (whiten) {
      double te[m];
#pragma unroll
      for (int i = 0; i < m; i++) {
        double s = 0;
#pragma unroll
        for (int q = 0; q < m; q++) s += U[i * m + q] * E.e[q];
        te[i] = s;
      }
#pragma unroll
      for (int i = 0; i < m; i++) E.e[i] = te[i];
    }
    double sq = 0;
#pragma unroll
    for (int i = 0; i < m; i++) sq += E.e[i] * E.e[i];
    double rho, drho;
    if (useImuLoss) huber_jet2(d.imu.a, d.imu.b, d.imu.k2, d.imu.h, sq, rho, drho);
    else rho = sq, drho = 1.0;
    if constexpr (Report) {
      // covWeightedSquaredError and singleCost = computeSingleCost(i, false) (Factor.h:172-232)
      const int64_t row = k - rep->first;
      acc[0] = 0.5 * (useImuLoss ? huber_val(d.imu.a, d.imu.b, d.imu.k2, d.imu.h, sq) : sq);
      if (rep->sqw) rep->sqw[row] = 0.5 * sq;
      if (rep->cost) rep->cost[row] = acc[0];
    } else if (a.mode == 2) {
      acc[0] = 0.5 * (useImuLoss ? huber_val(d.imu.a, d.imu.b, d.imu.k2, d.imu.h, sq) : sq);
    } else {
      acc[0] = 0.5 * rho;
      double* se = d.sE + slot * kSmallE;
      se[0] = drho;
#pragma unroll
      for (int i = 0; i < m; i++) se[1 + i] = E.e[i];
      int32_t* mt = d.sMeta + slot * kSmallMeta;
      mt[0] = m, mt[1] = colc, mt[2] = nv, mt[3] = whiten ? (int32_t)(U - a.consts) : -1, mt[4] = FK;
#pragma unroll
      for (int s = 0; s < nv; s++) mt[5 + s] = E.red[s], mt[15 + s] = E.col[s], mt[25 + s] = E.dim[s];
    }
  }
  return acc[0];
}

// f(std::integral_constant<int, FK>{}) for the one kind FK of [LO, HI] equal to fk: small_eval is a template
// over the kind, so a kernel over kinds [LO, HI] holds those instantiations and no others
template <int LO, int HI, class F>
__device__ __forceinline__ void small_dispatch(int fk, F&& f) {
  if constexpr (LO <= HI) {
    if (fk == LO) f(std::integral_constant<int, LO>{});
    else small_dispatch<LO + 1, HI>(fk, f);
  }
}

// all kinds in one launch: block b evaluates kind FK for the blocks [first[FK], first[FK + 1]) (one
// lane per factor); a dispatch per block instead of 13 serial launches of a few waves each
struct SmallLaunch {
  SmallArgs a[14];
  int32_t first[15];
  int32_t countCost;  // the root counts the small factors' cost (partitioned: every rank evaluates)
};
// kinds [LO, HI] per launch: the IMU kinds (1-3) get a kernel of their own, so their register
// allocation is not the union with the priors' and random walks' paths
template <int LO, int HI>
__global__ void __launch_bounds__(64) small_kernel(Dev d, SmallLaunch L) {
  const int b = blockIdx.x + L.first[LO];
  int fk = LO;
  while (fk < HI && b >= L.first[fk + 1]) fk++;
  const int64_t k = (int64_t)(b - L.first[fk]) * 64 + threadIdx.x;
  double acc[1] = {0.0};
  small_dispatch<LO, HI>(fk, [&](auto kind) {
    constexpr int FK = decltype(kind)::value;
    acc[0] = small_eval<FK>(d, L.a[FK], k);
  });
  if (!L.countCost) acc[0] = 0.0;
  block_sum_atomic<1>(acc, d.red + (L.a[1].mode == 2 ? 1 : 0));
}

// Residual report of one small kind: rows [R.first, R.first + R.n) through small_eval's evaluate-only
// instantiation, one lane per factor; adds into no reduction slot
template <int LO, int HI>
__global__ void __launch_bounds__(64) small_report_kernel(Dev d, SmallArgs a, int fk, RepRows R) {
  const int64_t k = R.first + (int64_t)blockIdx.x * 64 + threadIdx.x;
  small_dispatch<LO, HI>(fk, [&](auto kind) { small_eval<decltype(kind)::value, true>(d, a, k, &R); });
}

// singleExpectedDelta of the small kinds (Factor.h:470-540; inspect.hpp), two launches.
// 1. small_eval<FK> with Jacobians (the linearization's instantiation, mode 1), one lane per factor of rows
//    [first, a.n), over a copy of Dev whose staging pointers are the inspection's own (launch_small_expected):
//    the Jacobian blocks, [rho', whitened residual] and meta go to slot k - first there, and v0 = 0.5 rho to
//    v0[k - first].  d.sJ / d.sE / d.sMeta of the last linearization, the reduction and error slots are
//    neither read nor written.
template <int LO, int HI>
__global__ void __launch_bounds__(64) small_expected_eval_kernel(Dev d, SmallArgs a, int fk, int64_t first, double* v0) {
  const int64_t k = first + (int64_t)blockIdx.x * 64 + threadIdx.x;
  small_dispatch<LO, HI>(fk, [&](auto kind) {
    const double c = small_eval<decltype(kind)::value>(d, a, k);
    if (k < a.n) v0[k - first] = c;
  });
}
// 2. one wave per staged factor (4 per workgroup): w = rho' P e = rho' U^T (U e) from the whitened residual
//    (P = U^T U; no U: w = rho' e), lane r < m; then the lanes over the columns of every slot with a reduced
//    id (constant, unregistered and gravity slots have none): g = J_col^T w from the raw Jacobian, its product
//    with the step at rvOff[red] + j and its square, summed over the wave in a fixed order.  The calibration
//    kinds' blocks hold their enabled entries only (dim columns), as the step does.
__global__ void __launch_bounds__(256) small_expected_dot_kernel(Dev d, InsStage S, int fk, InsRows R) {
  __shared__ double wl[4][kMaxM + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
  if (slot >= R.n) return;
  const int32_t* mt = S.sMeta + slot * kSmallMeta;
  const int m = mt[0], nv = mt[2], uoff = mt[3];
  const double* Jg = S.sJ + slot * kSmallJ;
  const double* se = S.sE + slot * kSmallE;
  const double drho = se[0];
  if (lane < m) {
    double x = se[1 + lane];
    if (uoff >= 0) {
      const double* U = d.sf[fk].consts + uoff;
      x = 0.0;
      for (int i = 0; i < m; i++) x += U[i * m + lane] * se[1 + i];
    }
    wl[wave][lane] = drho * x;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
  double dl = 0.0, g2 = 0.0;
  for (int s = 0; s < nv; s++) {
    const int red = mt[5 + s];
    if (red < 0) continue;
    const int col = mt[15 + s], dim = mt[25 + s];
    const double* sp = R.stepRed + d.rvOff[red];
    for (int j = lane; j < dim; j += 64) {
      double g = 0.0;
      for (int r = 0; r < m; r++) g += Jg[r * kMaxCols + col + j] * wl[wave][r];
      dl += sp[j] * g, g2 += g * g;
    }
  }
  dl = wave_sum(dl), g2 = wave_sum(g2);
  if (lane == 0) R.delta[slot] = dl, R.gnorm[slot] = sqrt(g2);
}

// Assembly of the staged small factors, one wave per factor (4 per workgroup): whitened Jacobian
// U J in LDS (lane = column), gradient rho' J^T e (mode 0 / 1) and, in mode 0, the Gauss-Newton
// block rho' J^T J over the factor's non-constant columns, lane-parallel over the lower-triangle
// entries, fp64 atomics into the reduced tiles (Optimizer.cpp:136-146 via the factor stores'
// jacobian accumulation, InertialFactor / PriorFactor / RandomWalkFactor).
// MM: row capacity of the launch (its kinds' residual sizes), so that the per-wave LDS copy of the
// whitened Jacobian is only as large as needed (IMU factors: 9 rows -> 6 workgroups per CU)
// The active columns are ordered by reduced row and the lower-triangle entries enumerated column by
// column, so the lanes of one atomic instruction add into consecutive rows of a tile column (a few
// cache lines per instruction instead of one line per lane: the L2's atomic rate bounds this kernel).
// The entries' tiles come from a per-wave table over the factor's distinct tile rows, filled
// lane-parallel before the entry loop (rows beyond the table look theirs up); sized so the IMU launch
// keeps 6 workgroups per CU.
constexpr int kAsmTiles = 7;
template <int MM>
__global__ void __launch_bounds__(256) small_assemble_kernel(Dev d, int mode, double* gOut, int64_t s0, int64_t s1) {
  __shared__ double Jl[4][MM * kMaxCols];
  // active column: (staged column, reduced row << 5 | tile-row slot + 1; reduced rows < 2^26)
  __shared__ int32_t act[4][kMaxCols][2];
  __shared__ int32_t trow[4][kAsmTiles];   // the factor's distinct tile rows
  __shared__ int32_t tpair[4][kAsmTiles * kAsmTiles];  // tileIdx of (tile row u, tile row v), u >= v
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t slot = s0 + (int64_t)blockIdx.x * 4 + wave;
  if (slot >= s1) return;
  const int32_t* mt = d.sMeta + slot * kSmallMeta;
  const int m = mt[0], colc = mt[1], nv = mt[2], uoff = mt[3], fk = mt[4];
  const double* Jg = d.sJ + slot * kSmallJ;
  const double* se = d.sE + slot * kSmallE;
  const double drho = se[0];
  double* J = Jl[wave];
  const double* U = uoff >= 0 ? d.sf[fk].consts + uoff : nullptr;
  for (int j = lane; j < colc; j += 64) {
    double col[MM];  // statically indexed (registers): every loop over it is unrolled to MM
#pragma unroll
    for (int i = 0; i < MM; i++) col[i] = i < m ? Jg[i * kMaxCols + j] : 0.0;
    if (U) {
#pragma unroll
      for (int i = 0; i < MM; i++) {
        if (i >= m) break;
        double s = 0;
#pragma unroll
        for (int q = 0; q < MM; q++)
          if (q < m) s += U[i * m + q] * col[q];
        J[i * kMaxCols + j] = s;
      }
    } else {
#pragma unroll
      for (int i = 0; i < MM; i++)
        if (i < m) J[i * kMaxCols + j] = col[i];
    }
  }
  const int T = d.T;
  // the factor's variables, lane s < nv: first reduced row, dimension, staged column (dimension 0: none)
  int32_t vro = 0x7fffffff, vdim = 0, vcol = 0;
  if (lane < nv) {
    const int red = mt[5 + lane];
    if (red >= 0) vro = (int32_t)d.rvOff[red], vdim = mt[25 + lane], vcol = mt[15 + lane];
  }
  int32_t vstart = 0, nAct = 0;  // first active column of the lane's variable in row order; column count
  for (int s = 0; s < nv; s++) {
    const int32_t ro = __builtin_amdgcn_readlane(vro, s), dim = __builtin_amdgcn_readlane(vdim, s);
    if (ro < vro) vstart += dim;
    nAct += dim;
  }
  if (nAct <= 64) {  // lane j: active column j; the distinct tile rows by ballot rounds
    const bool on = lane < nAct;
    int32_t R = 0, c = 0;
    for (int s = 0; s < nv; s++) {
      const int32_t st = __builtin_amdgcn_readlane(vstart, s), dim = __builtin_amdgcn_readlane(vdim, s);
      if (lane >= st && lane < st + dim) {
        R = __builtin_amdgcn_readlane(vro, s) + (lane - st);
        c = __builtin_amdgcn_readlane(vcol, s) + (lane - st);
      }
    }
    const int32_t t = R / T;
    uint64_t left = __ballot(on);
    int nu = 0, u = -1;
    while (left) {
      const int32_t tl = __builtin_amdgcn_readlane(t, __builtin_ctzll(left));
      const bool hit = on && t == tl;
      left &= ~__ballot(hit);
      if (nu < kAsmTiles) {
        if (hit) u = nu;
        if (lane == 0) trow[wave][nu] = tl;
        nu++;
      }
    }
    if (on) act[wave][lane][0] = c, act[wave][lane][1] = R << 5 | (u + 1);
    if (lane == 0) act[wave][kMaxCols - 1][0] = nu, act[wave][kMaxCols - 1][1] = nAct;
  } else if (lane == 0) {
    // the factor's variables by first reduced row (insertion sort, <= 10), then their columns
    int32_t vro[10], vs[10], nvar = 0;
    for (int s = 0; s < nv; s++) {
      const int red = mt[5 + s];
      if (red < 0) continue;
      const int32_t ro = (int32_t)d.rvOff[red];
      int k = nvar++;
      for (; k > 0 && vro[k - 1] > ro; k--) vro[k] = vro[k - 1], vs[k] = vs[k - 1];
      vro[k] = ro, vs[k] = s;
    }
    int n = 0, nu = 0;
    for (int k = 0; k < nvar; k++) {
      const int s = vs[k];
      for (int i = 0; i < mt[25 + s]; i++) {
        const int32_t R = vro[k] + i, t = R / T;
        int u = 0;
        while (u < nu && trow[wave][u] != t) u++;
        if (u == nu && nu < kAsmTiles) trow[wave][nu++] = t;
        act[wave][n][0] = mt[15 + s] + i, act[wave][n][1] = R << 5 | (u < kAsmTiles ? u + 1 : 0), n++;
      }
    }
    // counts (slot kMaxCols - 1 is never a column: colc <= 80 incl. scratch)
    act[wave][kMaxCols - 1][0] = nu, act[wave][kMaxCols - 1][1] = n;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  const int A = act[wave][kMaxCols - 1][1];
  for (int a = lane; a < A; a += 64) {
    const int c = act[wave][a][0];
    double g = 0;
    for (int r = 0; r < m; r++) g += J[r * kMaxCols + c] * se[1 + r];
    const int32_t R = act[wave][a][1] >> 5;
    if (owns_col(d, R / T)) atomicAdd(gOut + R, drho * g);
  }
  if (mode != 0) return;
  const int nu = act[wave][kMaxCols - 1][0];
  for (int q = lane; q < nu * nu; q += 64) {
    const int tu = trow[wave][q / nu], tv = trow[wave][q % nu];
    tpair[wave][q] = tu >= tv ? d.tileIdx[(int64_t)tu * d.nT + tv] : -1;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // entry p of the column-major lower triangle: column b, row a >= b (R_a >= R_b by the ordering);
  // q = P - 1 - p decoded row-major gives (A - 1 - b, A - 1 - a)
  const int P = A * (A + 1) / 2;
  for (int p = lane; p < P; p += 64) {
    const int q = P - 1 - p;
    int i = (int)((sqrtf(8.0f * q + 1.0f) - 1.0f) * 0.5f);  // f32 estimate, corrected below
    while (i * (i + 1) / 2 > q) i--;
    while ((i + 1) * (i + 2) / 2 <= q) i++;
    const int b = A - 1 - i, a = A - 1 - (q - i * (i + 1) / 2);
    const int ca = act[wave][a][0], cb = act[wave][b][0];
    double hs = 0;
    for (int r = 0; r < m; r++) hs += J[r * kMaxCols + ca] * J[r * kMaxCols + cb];
    const int32_t wa = act[wave][a][1], wb = act[wave][b][1];
    const int32_t R = wa >> 5, C = wb >> 5, uR = (wa & 31) - 1, uC = (wb & 31) - 1;
    if (!owns_col(d, C / T)) continue;
    double* dst = uR >= 0 && uC >= 0 ? d.tiles + (int64_t)tpair[wave][uR * nu + uC] * T * T + (C % T) * T + (R % T)
                                     : tile_addr(d, R, C);
    atomicAdd(dst, drho * hs);
  }
}

void launch_small_eval(const Dev& d, int mode, double* gOut, hipStream_t st) {
  SmallLaunch L{};
  int32_t nb = 0;
  for (int fk = 1; fk < 14; fk++) {
    const SmallFactors& f = d.sf[fk];
    L.a[fk] = SmallArgs{f.n, f.vars, f.consts, f.nc, mode, gOut};
    L.first[fk] = nb;
    nb += (int32_t)((f.n + 63) / 64);
  }
  L.first[14] = nb;
  L.countCost = d.root;
  const int32_t nImu = L.first[4] - L.first[1], nRest = L.first[14] - L.first[4];
  if (nImu > 0) hipLaunchKernelGGL((small_kernel<1, 3>), dim3((unsigned)nImu), dim3(64), 0, st, d, L);
  if (nRest > 0) hipLaunchKernelGGL((small_kernel<4, 13>), dim3((unsigned)nRest), dim3(64), 0, st, d, L);
}

void launch_small_rows(const Dev& d, int fk, const RepRows& R, hipStream_t st) {
  if (R.n <= 0) return;
  const SmallFactors& f = d.sf[fk];
  const SmallArgs a{R.first + R.n, f.vars, f.consts, f.nc, 2, nullptr};
  const dim3 grid((unsigned)((R.n + 63) / 64));
  if (fk <= 3) hipLaunchKernelGGL((small_report_kernel<1, 3>), grid, dim3(64), 0, st, d, a, fk, R);
  else hipLaunchKernelGGL((small_report_kernel<4, 13>), grid, dim3(64), 0, st, d, a, fk, R);
}

void launch_small_expected(const Dev& d, int fk, const InsRows& R, const InsStage& S, hipStream_t st) {
  if (R.n <= 0 || R.n > S.cap) return;
  // the evaluation's view of the handle: the inspection's staging, row R.first at slot 0
  Dev di = d;
  di.sJ = S.sJ, di.sE = S.sE, di.sMeta = S.sMeta;
  di.sf[fk].stage = -R.first;
  const SmallFactors& f = d.sf[fk];
  const SmallArgs a{R.first + R.n, f.vars, f.consts, f.nc, 1, nullptr};
  const dim3 grid((unsigned)((R.n + 63) / 64));
  if (fk <= 3) hipLaunchKernelGGL((small_expected_eval_kernel<1, 3>), grid, dim3(64), 0, st, di, a, fk, R.first, R.v0);
  else hipLaunchKernelGGL((small_expected_eval_kernel<4, 13>), grid, dim3(64), 0, st, di, a, fk, R.first, R.v0);
  hipLaunchKernelGGL(small_expected_dot_kernel, dim3((unsigned)((R.n + 3) / 4)), dim3(256), 0, st, d, S, fk, R);
}

void launch_small_assemble(const Dev& d, int mode, double* gOut, hipStream_t st, int part = 3);
void launch_small(const Dev& d, int mode, double* gOut, hipStream_t st) {
  launch_small_eval(d, mode, gOut, st);
  launch_small_assemble(d, mode, gOut, st);
}
// part bit 0: the IMU kinds' launch, bit 1: the omega priors' and the rest's launches
void launch_small_assemble(const Dev& d, int mode, double* gOut, hipStream_t st, int part) {
  if (mode == 2 || d.nSmallStage <= 0) return;
  // three launches by residual size: IMU kinds 1-3 (9 rows), omega priors (3), the rest (<= 23); the
  // staging slots run kind by kind
  const int64_t a = d.sf[1].stage, b = d.sf[4].stage, c = d.sf[5].stage, e = d.nSmallStage;
  if (b > a && (part & 1))
    launchK(small_assemble_kernel<9>, dim3((unsigned)((b - a + 3) / 4)), dim3(256), 0, st, d, mode, gOut, a, b);
  if (c > b && (part & 2))
    hipLaunchKernelGGL(small_assemble_kernel<3>, dim3((unsigned)((c - b + 3) / 4)), dim3(256), 0, st, d, mode, gOut, b, c);
  if (e > c && (part & 2))
    hipLaunchKernelGGL(small_assemble_kernel<kMaxM>, dim3((unsigned)((e - c + 3) / 4)), dim3(256), 0, st, d, mode, gOut,
                       c, e);
}

}  // namespace viba
