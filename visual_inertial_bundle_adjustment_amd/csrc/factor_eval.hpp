// Device-side factor evaluators shared by the factor kernels (visual.hip, small.hip, refine.hip), device
// code only:
//   wave_sum / block_sum_atomic  the reductions of a lane's terms
//   VisOut, vis_eval, rs_eval    VisualFactor / RollingShutterVisualFactor (VisualFactor.cpp:40-82, 131-210):
//                                whitened residual and, WantJ, the Jacobian blocks
//   VisObs, vis_obs_load,        one observation's indices and the evaluation behind them: loads the pose,
//   vis_obs_eval                 extrinsics, camera and velocity and takes the global- or rolling-shutter path.
//                                Every consumer of a visual residual (linearization, cost pass, residual
//                                report, expected delta, point refinement) goes through vis_obs_eval.
#pragma once
#include "device_math.hpp"
#include "engine.hpp"

namespace viba {
using namespace dev;

__device__ __forceinline__ v3 mk3(const double* base, int h) {
  const double* p = base + (int64_t)h * 3;
  return mk(p[0], p[1], p[2]);
}

// ------------------------------------------------------------------ reduction helpers
// sum over the wave in a fixed tree, the result in every lane
__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

template <int N>
__device__ void block_sum_atomic(double (&v)[N], double* out) {
  __shared__ double sh[N][4];
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double x = wave_sum(v[k]);
    if ((threadIdx.x & 63) == 0) sh[k][threadIdx.x >> 6] = x;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
    for (int k = 0; k < N; k++) {
      double s = 0;
      for (int w = 0; w < nw; w++) s += sh[k][w];
      if (s != 0.0) atomicAdd(out + k, s);
    }
  }
}

// ------------------------------------------------------------------ visual factor evaluation
// Jintr (2 x 17, rows at 0 and 17) points into the caller's LDS staging (visual_lin_kernel): the
// largest block stays out of registers; unused when WantJ is false
struct VisOut {
  double e[2];
  double Jpt[6], Jpose[12], Jextr[12], Jvel[6];
  double* Jintr;
};

// VisualFactor::operator() (VisualFactor.cpp:40-82) for T_bw given; Jacobians wrt point, the
// pose argument (2x6), extrinsics (2x6) and intrinsics (2x nparams); PointOnly: the point Jacobian
// alone (point refinement, varGradHess of the point variable)
template <bool WantJ, bool PointOnly = false>
__device__ bool vis_eval(const double* obsC, v3 X, const se3& Tbw, const se3& Tcb, const double* cam,
                         VisOut& o) {
  v3 pRig = se3_act(Tbw, X);
  v3 pCam = se3_act(Tcb, pRig);
  double uv[2], Jc[6], Jp[30];
  if (!project<WantJ>(cam, pCam, uv, Jc, Jp)) return false;
  const double s00 = obsC[2], s01 = obsC[3], s10 = obsC[4], s11 = obsC[5];
  const double r0 = uv[0] - obsC[0], r1 = uv[1] - obsC[1];
  o.e[0] = s00 * r0 + s01 * r1;
  o.e[1] = s10 * r0 + s11 * r1;
  if (WantJ) {
    double dW[6];  // sqrtH * dProj (2x3)
#pragma unroll
    for (int j = 0; j < 3; j++) dW[j] = s00 * Jc[j] + s01 * Jc[3 + j], dW[3 + j] = s10 * Jc[j] + s11 * Jc[3 + j];
    m3 Rcb = qmat(Tcb.R);
    m3 Rcw = qmat(qmul(Tcb.R, Tbw.R));
#pragma unroll
    for (int r = 0; r < 2; r++) {
#pragma unroll
      for (int j = 0; j < 3; j++)
        o.Jpt[r * 3 + j] = dW[r * 3] * Rcw.a[0][j] + dW[r * 3 + 1] * Rcw.a[1][j] + dW[r * 3 + 2] * Rcw.a[2][j];
      if (PointOnly) continue;
      double A[3];
#pragma unroll
      for (int j = 0; j < 3; j++)
        A[j] = dW[r * 3] * Rcb.a[0][j] + dW[r * 3 + 1] * Rcb.a[1][j] + dW[r * 3 + 2] * Rcb.a[2][j];
      // [A, A hat(-p)] ; A hat(-p) = p x A (row vector form): (A hat(-p))_j = sum_i A_i hat(-p)_ij
      const v3 mp = neg(pRig);
      o.Jpose[r * 6 + 0] = A[0], o.Jpose[r * 6 + 1] = A[1], o.Jpose[r * 6 + 2] = A[2];
      o.Jpose[r * 6 + 3] = A[1] * mp.z - A[2] * mp.y;
      o.Jpose[r * 6 + 4] = -A[0] * mp.z + A[2] * mp.x;
      o.Jpose[r * 6 + 5] = A[0] * mp.y - A[1] * mp.x;
      const v3 mc = neg(pCam);
      const double* B = dW + r * 3;
      o.Jextr[r * 6 + 0] = B[0], o.Jextr[r * 6 + 1] = B[1], o.Jextr[r * 6 + 2] = B[2];
      o.Jextr[r * 6 + 3] = B[1] * mc.z - B[2] * mc.y;
      o.Jextr[r * 6 + 4] = -B[0] * mc.z + B[2] * mc.x;
      o.Jextr[r * 6 + 5] = B[0] * mc.y - B[1] * mc.x;
    }
    if (PointOnly) return true;
    const int n = (int)cam[1];
#pragma unroll
    for (int j = 0; j < 17; j++) {
      // n <= 15 projection parameters: columns 15, 16 (readout, offset) are never read from Jp, which
      // keeps every Jp index static and in bounds (a possibly-out-of-bounds select spilled Jp to scratch)
      const bool in = j < 15 && j < n;
      const double a0 = in ? Jp[j < 15 ? j : 0] : 0.0, a1 = in ? Jp[15 + (j < 15 ? j : 0)] : 0.0;
      o.Jintr[j] = s00 * a0 + s01 * a1;
      o.Jintr[17 + j] = s10 * a0 + s11 * a1;
    }
  }
  return true;
}

// RollingShutterVisualFactor::operator() (VisualFactor.cpp:131-210)
template <bool WantJ, bool PointOnly = false>
__device__ bool rs_eval(const Dev& d, const double* obsC, int rs, v3 X, const se3& Tbw, const se3& Tcb,
                        const double* cam, v3 vel, bool wantTime, bool wantVel, VisOut& o, bool* oor) {
  const double tpf = obsC[1] / cam[3] - 0.5;
  const double ro = cam[4] != 0.0 ? cam[5] : 0.0;
  const double dt = ro * tpf - cam[6];
  const int64_t s0 = d.rsOff[rs], ns = d.rsN[rs];
  const double* S = d.rsS + s0 * 11;
  const double* I = d.rsI + (s0 - rs) * 9;
  const double* G = d.rsG + rs * 3;
  se3 Twb = se3_inv(Tbw);
  q4 Rbw = qinv(Twb.R);
  se3 TmidAtT = rs_estimate(S, I, (int)ns, G, dt, vel, Rbw, oor);
  if (*oor) return false;
  se3 TAtTMid = se3_inv(TmidAtT);
  se3 TAtTw = se3_mul(TAtTMid, Tbw);
  if (!vis_eval<WantJ, PointOnly>(obsC, X, TAtTw, Tcb, cam, o)) return false;
  if (WantJ && !PointOnly) {
    double Jt[12];  // wrt T_AtT_w
#pragma unroll
    for (int i = 0; i < 12; i++) Jt[i] = o.Jpose[i];
    const int n = (int)cam[1];
    const bool estRO = cam[7] != 0.0, estOff = cam[8] != 0.0;
    if (wantTime && (estRO || estOff)) {
      const double kEps = 1e-6;
      se3 TP = rs_estimate(S, I, (int)ns, G, dt + kEps, vel, Rbw, oor);
      if (*oor) return false;
      se3 dd = se3_mul(se3_inv(TP), TmidAtT);
      double lg[6];
      se3_log(dd, lg);
      double dE[2];
#pragma unroll
      for (int r = 0; r < 2; r++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += Jt[r * 6 + k] * (lg[k] / kEps);
        dE[r] = s;
      }
      // columns after the n projection parameters: readout time (if estimated), then time offset;
      // written by an unrolled select (a runtime index would put the whole record in scratch)
      const int iRO = estRO ? n : -1, iOff = estOff ? n + (estRO ? 1 : 0) : -1;
#pragma unroll
      for (int j = 0; j < 17; j++) {
        if (j == iOff) o.Jintr[j] = -dE[0], o.Jintr[17 + j] = -dE[1];
        if (j == iRO) o.Jintr[j] = dE[0] * tpf, o.Jintr[17 + j] = dE[1] * tpf;
      }
    }
    // pose Jacobian: Jt * (Adj(T_AtT_Mid) + [0, hat(R_AtT_w (v dt + 0.5 dt^2 g))])
    double M[36];
    se3_Adj(TAtTMid, M);
    v3 vv = add(scl(dt, vel), scl(0.5 * dt * dt, mk(G[0], G[1], G[2])));
    m3 H = hat(qrot(TAtTw.R, vv));
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) M[i * 6 + 3 + j] += H.a[i][j];
#pragma unroll
    for (int r = 0; r < 2; r++)
#pragma unroll
      for (int j = 0; j < 6; j++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += Jt[r * 6 + k] * M[k * 6 + j];
        o.Jpose[r * 6 + j] = s;
      }
    if (wantVel) {
      m3 R = qmat(TAtTw.R);
#pragma unroll
      for (int r = 0; r < 2; r++)
#pragma unroll
        for (int j = 0; j < 3; j++)
          o.Jvel[r * 3 + j] = -dt * (Jt[r * 6] * R.a[0][j] + Jt[r * 6 + 1] * R.a[1][j] + Jt[r * 6 + 2] * R.a[2][j]);
    } else {
#pragma unroll
      for (int i = 0; i < 6; i++) o.Jvel[i] = 0.0;
    }
  }
  return true;
}

// ------------------------------------------------------------------ one observation
// the indices of an observation (Dev::obPack: observation id, variable handles, rolling-shutter table or
// -1, flags: 1 intrinsics estimated, 2 velocity estimated) and its 6 doubles (u, v, sqrtH 2x2)
struct VisObs {
  int32_t o, pt, pose, extr, intr, rs, vel, flags;
  const double* obsC;
};

// position i of obCostOrder: two coalesced 16 B reads
__device__ __forceinline__ VisObs vis_obs_load(const Dev& d, int64_t i) {
  const int4 pa = reinterpret_cast<const int4*>(d.obPack)[2 * i], pb = reinterpret_cast<const int4*>(d.obPack)[2 * i + 1];
  return VisObs{pa.x, pa.y, pa.z, pa.w, pb.x, pb.y, pb.z, pb.w, d.obCP + i * 6};
}

// the observation at point X (its own point, or a trial point of the refinement): vis_eval for a global
// shutter (Jvel zeroed when the full Jacobian is wanted), rs_eval with the velocity for a rolling one; the
// time and velocity columns are formed only where the flags ask for them.  False if the factor fails; oor is
// raised when a rolling-shutter lookup was out of range (the callers keep their own error words).
template <bool WantJ, bool PointOnly = false>
__device__ __forceinline__ bool vis_obs_eval(const Dev& d, const VisObs ob, v3 X, VisOut& v, bool& oor) {
  se3 Tbw = se3_load(d.var[1] + (int64_t)ob.pose * 7);
  se3 Tcb = se3_load(d.var[5] + (int64_t)ob.extr * 7);
  const double* cam = d.var[4] + (int64_t)ob.intr * 24;
  if (ob.rs < 0) {
    const bool ok = vis_eval<WantJ, PointOnly>(ob.obsC, X, Tbw, Tcb, cam, v);
    if (WantJ && !PointOnly)
#pragma unroll
      for (int i = 0; i < 6; i++) v.Jvel[i] = 0.0;
    return ok;
  }
  return rs_eval<WantJ, PointOnly>(d, ob.obsC, ob.rs, X, Tbw, Tcb, cam, mk3(d.var[2], ob.vel), WantJ && (ob.flags & 1) != 0,
                                   WantJ && (ob.flags & 2) != 0, v, &oor);
}

// BaseMapVisualFactor::operator() (BaseMapVisualFactor.cpp:15-36) of the base-map factor at sorted position i
// (engine.hpp BaseMapDev) at point X: the global-shutter evaluation with the key rig's pose, the camera's
// extrinsics and record as constants -- vis_eval's order is the reference's (T_bodyImu_world * X, then
// T_Cam_BodyImu, fail below z = 1e-6, sqrtH * (proj - uv), J = sqrtH * dProj * R_cb * R_bw); the camera's
// estimate flags, readout time and time offset are never read on this path.  Residual in v.e, WantJ: v.Jpt.
template <bool WantJ>
__device__ __forceinline__ bool bm_eval(const Dev& d, int64_t i, v3 X, VisOut& v) {
  const int32_t c = d.bm.camOf[i];
  const se3 Tbw = se3_load(d.bm.rig + (int64_t)d.bm.camRig[c] * 7);
  const se3 Tcb = se3_load(d.bm.camT + (int64_t)c * 7);
  return vis_eval<WantJ, true>(d.bm.C + i * 6, X, Tbw, Tcb, d.bm.cam + (int64_t)c * 24, v);
}

}  // namespace viba
