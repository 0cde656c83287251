// Kernels of the visual factors (gfx950), one observation per lane, all through vis_obs_eval (factor_eval.hpp):
//   visual_lin_kernel<Cost>     linearization: the loss-whitened residual and Jacobian planes
//                               (sqrt(rho') * [e | J], HuberLossWithCutoff, SoftLoss.h:115-176) staged in LDS
//                               and stored as whole records, with the ResultCache rules of Factor.h:555-583;
//                               Cost: also the global-shutter cost sums of a speculative linearization
//   visual_cost_kernel          cost pass with the makeComparableWithStored rules of Factor.h:390-417
//   visual_report_kernel<Hist>  residual report (report.hpp): per-row errors, or the grouped histogram
//   visual_expected_kernel      singleExpectedDelta along a step (inspect.hpp)
// and their launchers.
#include "factor_eval.hpp"
#include "inspect.hpp"
#include "report.hpp"
#include <algorithm>

namespace viba {

// ------------------------------------------------------------------ linearization
// Linearization of the visual factors, one observation per lane. The whitened record is staged in
// LDS per wave and copied out record by record with 16 B lane stores (A: planes 0..31, B: 32..71), so
// a record's lines are written whole (per-lane 576 B record stores wrote partial lines, read for
// ownership: 2.5x the algorithmic HBM traffic).  Lanes take the observations in obCostOrder (each
// range global shutter first), so a wave runs one of the two evaluation paths; the order leaves only
// the record's position, which stays the observation's own slot.  Region A is staged at an odd record stride (33
// doubles: the per-lane ds_write_b64 of one plane hits 32 distinct banks); region B at kJB = 40, so a
// two-wave block takes exactly 40 KB and four blocks (the VGPR limit, 2 waves per SIMD) fit a CU's
// 160 KB -- at 41 only three did.  Its per-lane plane writes then conflict 8-way, a few hundred LDS
// cycles against the evaluation's tens of thousands.
typedef double double2_t __attribute__((ext_vector_type(2)));
typedef float float2_t __attribute__((ext_vector_type(2)));
// two adjacent record planes, rounded to the record type
__device__ __forceinline__ void store_planes(double* p, double a, double b) { *(double2_t*)p = double2_t{a, b}; }
__device__ __forceinline__ void store_planes(float* p, double a, double b) { *(float2_t*)p = float2_t{(float)a, (float)b}; }
constexpr int kVisBlock = 128;  // two waves, 2 x 20 KB of staging

// Cost: also the cost pass's sums (visual_cost_kernel, comparable) of the global-shutter observations
// into d.costS -- the linearization point of a speculative linearization is the stepped variables the
// cost pass evaluates; the rolling-shutter ones are not folded in (the cost pass evaluates them with
// the tables of the iteration's linearization, the speculative linearization with rebuilt ones).
// Only with dontRetry = 0: every observation is evaluated.
template <bool Cost>
__global__ void __launch_bounds__(kVisBlock) visual_lin_kernel(Dev d, int updateCache, int dontRetry, int64_t lo,
                                                               int64_t hi) {
  __shared__ double stage[kVisBlock / 64][64 * kJB];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t p0 = lo + (int64_t)blockIdx.x * kVisBlock + wave * 64;  // the wave's first position
  const int nrec = (int)max<int64_t>(0, min<int64_t>(64, hi - p0));
  // the observation of this lane: the range in obCostOrder (global shutter first), so a wave takes one
  // evaluation path; its record still goes to the observation's own slot
  VisObs ob{};
  if (lane < nrec) ob = vis_obs_load(d, p0 + lane);
  const int32_t o = ob.o;
  double* S = stage[wave];
  double acc[1] = {0.0};
  double cst[4] = {0.0, 0.0, 0.0, 0.0};  // Cost: cost, numTotal, numInvalid, numPrevInvalid
  VisOut v;
  v.Jintr = S + lane * kJB;  // region-B position of the record (intrinsics are planes 32..65)
  bool ok = false;
  double w = 0.0;
  if (lane < nrec) {
    ok = true;
    bool oor = false;
    const double c0 = d.cache[o];
    if (dontRetry && c0 < 0.0) {
      ok = false;
      if (updateCache) d.cacheW[o] = c0;  // (carried into the write buffer of a speculative linearization)
    } else {
      ok = vis_obs_eval<true>(d, ob, mk3(d.var[0], ob.pt), v, oor);
      if (oor) atomicOr(d.err, 1);
      if (!ok && (updateCache || dontRetry)) (updateCache ? d.cacheW : d.cache)[o] = -1.0;
    }
    if (ok) {
      const double s = v.e[0] * v.e[0] + v.e[1] * v.e[1];
      double rho, drho;
      huber_jet2(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s, rho, drho);
      w = sqrt(drho);
      acc[0] = 0.5 * rho;
      if (updateCache) d.cacheW[o] = 0.5 * rho;
    }
    if (Cost && ob.rs < 0) {  // visual_cost_kernel's sums, comparable
      const bool prevInvalid = c0 < 0.0;
      cst[1] = 1.0;
      cst[2] = ok ? 0.0 : 1.0;
      cst[3] = prevInvalid ? 1.0 : 0.0;
      cst[0] = prevInvalid ? 0.0 : (ok ? acc[0] : c0);
    }
  }
  // region B (intrinsics already in place from the evaluation): scale by w, velocity, copy out
  if (lane < nrec) {
    double* r = S + lane * kJB;
#pragma unroll
    for (int i = 0; i < 34; i++) r[i] = ok ? w * r[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) r[kJvel - kJA + i] = ok ? w * v.Jvel[i] : 0.0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    // wave-uniform trip count: the shuffle must read o from an active lane
    rec_t* dst = d.Jt + d.nObsPad * kJA;
    const int nq = nrec * (kJB / 2);
    for (int q0 = 0; q0 < nq; q0 += 64) {
      const int q = q0 + lane, r = min(q / (kJB / 2), 63), c = 2 * (q % (kJB / 2));
      const int64_t orec = __shfl(o, r, 64);
      if (q < nq) store_planes(dst + orec * kJB + c, S[r * kJB + c], S[r * kJB + c + 1]);
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  // region A: e (2), point (6), pose (12), extrinsics (12)
  if (lane < nrec) {
    double* r = S + lane * (kJA + 1);
#pragma unroll
    for (int i = 0; i < 2; i++) r[kJe + i] = ok ? w * v.e[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) r[kJpt + i] = ok ? w * v.Jpt[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 12; i++) r[kJpose + i] = ok ? w * v.Jpose[i] : 0.0;
#pragma unroll
    for (int i = 0; i < 12; i++) r[kJextr + i] = ok ? w * v.Jextr[i] : 0.0;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  {
    const int nq = nrec * (kJA / 2);
    for (int q0 = 0; q0 < nq; q0 += 64) {
      const int q = q0 + lane, r = min(q / (kJA / 2), 63), c = 2 * (q % (kJA / 2));
      const int64_t orec = __shfl(o, r, 64);
      if (q < nq) store_planes(d.Jt + orec * kJA + c, S[r * (kJA + 1) + c], S[r * (kJA + 1) + c + 1]);
    }
  }
  // wave sum, one atomic per wave (no LDS: the staging owns all of it)
  const double x = wave_sum(acc[0]);
  if (lane == 0 && x != 0.0) atomicAdd(d.redS + (blockIdx.x & 63) * 8 + 0, x);
  if (Cost) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const double y = wave_sum(cst[k]);
      if (lane == 0 && y != 0.0) atomicAdd(d.costS + (blockIdx.x & 63) * 8 + 1 + k, y);
    }
  }
}

// cost pass: red[1] += cost, red[2..4] += stats (numTotal, numInvalid, numPrevInvalid)
__global__ void __launch_bounds__(256) visual_cost_kernel(Dev d, int comparable, int64_t lo, int64_t hi) {
  const int64_t i = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < hi) {
    // position i of obCostOrder (a permutation of [lo, hi): global shutter first), packed (Dev::obPack)
    const VisObs ob = vis_obs_load(d, i);
    VisOut v;
    v.Jintr = nullptr;
    bool oor = false;
    const bool ok = vis_obs_eval<false>(d, ob, mk3(d.var[0], ob.pt), v, oor);
    if (oor) atomicOr(d.err, 32);  // (bit 32: in the cost pass, after the iteration's solve)
    const double prev = d.cache[ob.o];
    const bool prevInvalid = prev < 0.0;
    acc[1] = 1.0;
    acc[2] = ok ? 0.0 : 1.0;
    acc[3] = prevInvalid ? 1.0 : 0.0;
    if (comparable && prevInvalid) {
      // forced comparable: contributes nothing
    } else if (comparable && !ok) {
      acc[0] = prev;
    } else if (ok) {
      const double s = v.e[0] * v.e[0] + v.e[1] * v.e[1];
      acc[0] = 0.5 * huber_val(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s);
    }
  }
  block_sum_atomic<4>(acc, d.redS + (blockIdx.x & 63) * 8 + 1);
}

// Residual report of the visual factors (Histograms::showHistogramsVisual, Histograms.cpp:185-255, and the
// rawError / unweightedError logs): the cost pass's evaluation at the current variables and tables, not
// comparable, reading neither the ResultCache nor the reduction / error slots of the LM loop (err is the
// report's own word).  The functor whitens its return by sqrtH, so unweightedSquaredError =
// covWeightedSquaredError = 0.5 |e|^2 and singleCost = 0.5 rho(|e|^2) (Factor.h:172-232).
//   Hist:  item t = position t of obCostOrder (global shutter first: a wave takes one evaluation path);
//          every workgroup walks its share of the positions and bins sqrt(2 * 0.5 |e|^2) into an LDS
//          table [group][bin], flushed once at the end (rep_flush): no per-observation buffer
//   !Hist: item t = row R.first + t of vb_add_factors order (posOfRow: its position), the requested
//          arrays stored at t, coalesced
template <bool Hist>
__global__ void __launch_bounds__(256) visual_report_kernel(Dev d, const int32_t* posOfRow, RepRows R, RepHist H,
                                                            int32_t* err) {
  __shared__ RepTable tab;
  if (Hist) rep_clear(tab, H);
  const int64_t n = Hist ? d.nObs : R.n;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t i = Hist ? t : posOfRow[R.first + t];
    const VisObs ob = vis_obs_load(d, i);
    VisOut v;
    v.Jintr = nullptr;
    bool oor = false;
    const bool ok = vis_obs_eval<false>(d, ob, mk3(d.var[0], ob.pt), v, oor);
    if (oor) atomicOr(err, 1);
    const double s = ok ? v.e[0] * v.e[0] + v.e[1] * v.e[1] : 0.0;
    const double cost = ok ? 0.5 * huber_val(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s) : 0.0;
    if (Hist) {
      rep_add(tab, H, H.grp ? H.grp[i] : 0, ok, sqrt(2.0 * (0.5 * s)), cost);
    } else {
      if (R.raw) R.raw[2 * t] = ok ? v.e[0] : 0.0, R.raw[2 * t + 1] = ok ? v.e[1] : 0.0;
      if (R.squ) R.squ[t] = 0.5 * s;
      if (R.sqw) R.sqw[t] = 0.5 * s;
      if (R.cost) R.cost[t] = cost;
      if (R.valid) R.valid[t] = ok ? 1 : 0;
    }
  }
  if (Hist) rep_flush(tab, H);
}

// singleExpectedDelta of the visual factors (Factor.h:470-540; inspect.hpp): the linearization's evaluation
// (vis_eval<true> / rs_eval<true>, fp64 in both builds; the stored records d.Jt are not read) at the current
// variables and tables, one lane per item.  With w = rho' e the lane forms J_s^T w block by block and dots it
// with the step of the slot: stepPt + 3 ptLm[point], stepRed + rvOff[obRed[4 o + slot]]; a slot with reduced
// id -1 (constant, unregistered, no velocity) is skipped.  A failing factor gets (-1, 0, 0); beyond the loss
// cutoff rho' = 0, so delta = gnorm = 0 with v0 = 0.5 (2 a k - a^2).
// The point, pose, extrinsics and velocity blocks stay in registers; the 2 x 17 intrinsics block is the
// lane's 35-double row of LDS (odd stride: a plane's 64 lanes hit distinct banks), as visual_lin_kernel keeps
// it out of registers: 252 VGPRs, no scratch, 2 waves per SIMD (35 KB per 2-wave block, 4 blocks per CU).
// All in registers it took 256 VGPRs + 52 AGPRs at 1 wave per SIMD (62 VGPRs spilled when held to 2) and ran
// the whole x0 pass 17 % slower at config C.
//   posOfRow == nullptr: item t = position R.first + t of obCostOrder (global shutter first: a wave takes
//                        one evaluation path)
//   otherwise:           item t = row R.first + t of vb_add_factors order, stored at t, coalesced
// One kernel for both, so a row's numbers do not depend on the mode.  Reads neither the ResultCache nor the
// reduction / error slots of the LM loop (err is the caller's own word).
constexpr int kInsBlock = 128, kInsJ = 35;
__global__ void __launch_bounds__(kInsBlock) visual_expected_kernel(Dev d, const int32_t* posOfRow, InsRows R,
                                                                    int32_t* err) {
  const int64_t t = (int64_t)blockIdx.x * kInsBlock + threadIdx.x;
  if (t >= R.n) return;
  const int64_t i = posOfRow ? posOfRow[R.first + t] : R.first + t;
  const VisObs ob = vis_obs_load(d, i);
  // the slots' landmark / reduced ids and step offsets, loaded before the evaluation: behind it their two
  // dependent loads cost nothing, after it every slot's branch waited for its own chain
  const int32_t lm = d.ptLm[ob.pt];
  const int4 rd = reinterpret_cast<const int4*>(d.obRed)[ob.o];
  const int64_t oPose = rd.x >= 0 ? d.rvOff[rd.x] : 0, oExtr = rd.y >= 0 ? d.rvOff[rd.y] : 0;
  const int64_t oIntr = rd.z >= 0 ? d.rvOff[rd.z] : 0, oVel = rd.w >= 0 ? d.rvOff[rd.w] : 0;
  const int dimIntr = rd.z >= 0 ? d.rvDim[rd.z] : 0;
  __shared__ double jl[kInsBlock * kInsJ];
  double* ji = jl + threadIdx.x * kInsJ;
  VisOut v;
  v.Jintr = ji;
  bool oor = false;
  const bool ok = vis_obs_eval<true>(d, ob, mk3(d.var[0], ob.pt), v, oor);
  if (oor) atomicOr(err, 1);
  double v0 = -1.0, delta = 0.0, g2 = 0.0;
  if (ok) {
    const double s = v.e[0] * v.e[0] + v.e[1] * v.e[1];
    double rho, drho;
    huber_jet2(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s, rho, drho);
    v0 = 0.5 * rho;
    const double w0 = drho * v.e[0], w1 = drho * v.e[1];
    if (lm >= 0) {
      const double* sp = R.stepPt + (int64_t)lm * 3;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double g = v.Jpt[j] * w0 + v.Jpt[3 + j] * w1;
        delta += sp[j] * g, g2 += g * g;
      }
    }
    if (rd.x >= 0) {
      const double* sp = R.stepRed + oPose;
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const double g = v.Jpose[j] * w0 + v.Jpose[6 + j] * w1;
        delta += sp[j] * g, g2 += g * g;
      }
    }
    if (rd.y >= 0) {
      const double* sp = R.stepRed + oExtr;
#pragma unroll
      for (int j = 0; j < 6; j++) {
        const double g = v.Jextr[j] * w0 + v.Jextr[6 + j] * w1;
        delta += sp[j] * g, g2 += g * g;
      }
    }
    if (rd.z >= 0) {
      // tangent: the projection parameters, then readout time / time offset where estimated (<= 17)
      const double* sp = R.stepRed + oIntr;
#pragma unroll
      for (int j = 0; j < 17; j++) {
        if (j < dimIntr) {
          const double g = ji[j] * w0 + ji[17 + j] * w1;
          delta += sp[j] * g, g2 += g * g;
        }
      }
    }
    if (rd.w >= 0) {
      const double* sp = R.stepRed + oVel;
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double g = v.Jvel[j] * w0 + v.Jvel[3 + j] * w1;
        delta += sp[j] * g, g2 += g * g;
      }
    }
  }
  R.v0[t] = v0, R.delta[t] = delta, R.gnorm[t] = sqrt(g2);
}

// ------------------------------------------------------------------ launch wrappers
void launch_visual_lin(const Dev& d, int updateCache, int dontRetry, int64_t lo, int64_t hi, hipStream_t st) {
  if (hi <= lo) return;
  const int64_t n = hi - lo;
  if (d.costS)
    launchK(visual_lin_kernel<true>, dim3((unsigned)((n + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, st, d,
            updateCache, dontRetry, lo, hi);
  else
    launchK(visual_lin_kernel<false>, dim3((unsigned)((n + kVisBlock - 1) / kVisBlock)), dim3(kVisBlock), 0, st, d,
            updateCache, dontRetry, lo, hi);
}
void launch_visual_cost(const Dev& d, int comparable, int64_t lo, int64_t hi, hipStream_t st) {
  if (hi <= lo) return;
  const int64_t n = hi - lo;
  launchK(visual_cost_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d, comparable,
                     lo, hi);
}

// residual report (report.hpp)
void launch_visual_rows(const Dev& d, const int32_t* posOfRow, const RepRows& R, int32_t* err, hipStream_t st) {
  if (R.n <= 0) return;
  hipLaunchKernelGGL(visual_report_kernel<false>, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, d, posOfRow, R,
                     RepHist{}, err);
}
void launch_visual_hist(const Dev& d, const RepHist& H, int32_t* err, int blocks, hipStream_t st) {
  if (d.nObs <= 0) return;
  const int64_t nb = std::min<int64_t>((d.nObs + 255) / 256, std::max(1, blocks));
  hipLaunchKernelGGL(visual_report_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, d, (const int32_t*)nullptr,
                     RepRows{}, H, err);
}

// non-linearity inspection (inspect.hpp)
void launch_visual_expected(const Dev& d, const int32_t* posOfRow, const InsRows& R, int32_t* err, hipStream_t st) {
  if (R.n <= 0) return;
  hipLaunchKernelGGL(visual_expected_kernel, dim3((unsigned)((R.n + kInsBlock - 1) / kInsBlock)), dim3(kInsBlock), 0, st, d,
                     posOfRow, R, err);
}

}  // namespace viba
