// Kernels of the base-map visual factors (gfx950; BaseMapVisualFactor.{h,cpp}, MultiSessionProblemImpl.h:19-40):
// a point observed by a camera of a constant key rig of a base map (engine.hpp BaseMapDev).  One factor per
// lane through bm_eval (factor_eval.hpp: vis_eval<WantJ, PointOnly = true> with constant pose, extrinsics and
// camera):
//   basemap_lin_kernel          linearization: sqrt(rho') * [e | Jpt], one 64 B fp64 record per factor, with the
//                               ResultCache rules of visual_lin_kernel (Factor.h:555-583); cost into redS column 0.
//                               Per factor: 8 B of indices, 48 B of constants, the camera's tables (L2-resident),
//                               24 B of the point, 8 + 8 B of cache, 64 B of record
//   basemap_sum_kernel          per landmark with factors: V = sum Jp^T Jp, g = sum Jp^T e over its records in
//                               position order, stored (no float atomics: repeats bit for bit); 64 B read per
//                               factor, 72 B written per landmark
//   basemap_cost_kernel         cost pass with visual_cost_kernel's comparable rules (Factor.h:390-417) into redS
//                               columns 1..4; the linearization's reads without the record
//   basemap_report_kernel<Hist> residual report (report.hpp; Histograms.cpp:257-306): per-row errors, or the
//                               one-group histogram
// and their launchers.  None is launched on a handle without base-map factors.
#include "factor_eval.hpp"
#include "report.hpp"
#include <algorithm>

namespace viba {

__global__ void __launch_bounds__(256) basemap_lin_kernel(Dev d, int updateCache, int dontRetry) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc[1] = {0.0};
  if (i < d.bm.n) {
    VisOut v;
    v.Jintr = nullptr;
    bool ok = true;
    double w = 0.0;
    const double c0 = d.bm.cache[i];
    if (dontRetry && c0 < 0.0) {
      ok = false;
    } else {
      ok = bm_eval<true>(d, i, mk3(d.var[0], d.bm.pt[i]), v);
      if (!ok && (updateCache || dontRetry)) d.bm.cache[i] = -1.0;
    }
    if (ok) {
      const double s = v.e[0] * v.e[0] + v.e[1] * v.e[1];
      double rho, drho;
      huber_jet2(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s, rho, drho);
      w = sqrt(drho);
      acc[0] = 0.5 * rho;
      if (updateCache) d.bm.cache[i] = 0.5 * rho;
    }
    if (i < d.bm.nFree) {  // (a constant point's factor adds cost and CostStats only)
      double* r = d.bm.rec + i * 8;
      r[0] = ok ? w * v.e[0] : 0.0, r[1] = ok ? w * v.e[1] : 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) r[2 + k] = ok ? w * v.Jpt[k] : 0.0;
    }
  }
  block_sum_atomic<1>(acc, d.redS + (blockIdx.x & 63) * 8 + 0);
}

// item t = landmark lmWith[t]: its records summed in position order into Vg[9 l] (v00 v10 v20 v11 v21 v22, g)
__global__ void __launch_bounds__(256) basemap_sum_kernel(Dev d) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= d.bm.nLmWith) return;
  const int64_t l = d.bm.lmWith[t];
  double v00 = 0, v10 = 0, v20 = 0, v11 = 0, v21 = 0, v22 = 0, g0 = 0, g1 = 0, g2 = 0;
  for (int64_t i = d.bm.start[l]; i < d.bm.start[l + 1]; i++) {
    const double* r = d.bm.rec + i * 8;
    const double e0 = r[0], e1 = r[1], a0 = r[2], a1 = r[3], a2 = r[4], b0 = r[5], b1 = r[6], b2 = r[7];
    g0 += a0 * e0 + b0 * e1, g1 += a1 * e0 + b1 * e1, g2 += a2 * e0 + b2 * e1;
    v00 += a0 * a0 + b0 * b0, v10 += a1 * a0 + b1 * b0, v20 += a2 * a0 + b2 * b0;
    v11 += a1 * a1 + b1 * b1, v21 += a2 * a1 + b2 * b1, v22 += a2 * a2 + b2 * b2;
  }
  double* o = d.bm.Vg + l * 9;
  o[0] = v00, o[1] = v10, o[2] = v20, o[3] = v11, o[4] = v21, o[5] = v22, o[6] = g0, o[7] = g1, o[8] = g2;
}

// cost pass: red[1] += cost, red[2..4] += stats (numTotal, numInvalid, numPrevInvalid), as visual_cost_kernel
__global__ void __launch_bounds__(256) basemap_cost_kernel(Dev d, int comparable) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < d.bm.n) {
    VisOut v;
    v.Jintr = nullptr;
    const bool ok = bm_eval<false>(d, i, mk3(d.var[0], d.bm.pt[i]), v);
    const double prev = d.bm.cache[i];
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

// Residual report of the base-map factors (Histograms.cpp:257-306): the cost pass's evaluation at the current
// variables, not comparable, reading neither the cache nor the LM loop's reduction slots.  The functor whitens
// its return by sqrtH: unweightedSquaredError = covWeightedSquaredError = 0.5 |e|^2.
//   Hist:  item t = sorted position t, binned into the workgroup's LDS table (one group)
//   !Hist: item t = row R.first + t of vb_add_basemap_factors order, stored at t
template <bool Hist>
__global__ void __launch_bounds__(256) basemap_report_kernel(Dev d, RepRows R, RepHist H) {
  __shared__ RepTable tab;
  if (Hist) rep_clear(tab, H);
  const int64_t n = Hist ? d.bm.n : R.n;
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    const int64_t i = Hist ? t : d.bm.posOfRow[R.first + t];
    VisOut v;
    v.Jintr = nullptr;
    const bool ok = bm_eval<false>(d, i, mk3(d.var[0], d.bm.pt[i]), v);
    const double s = ok ? v.e[0] * v.e[0] + v.e[1] * v.e[1] : 0.0;
    const double cost = ok ? 0.5 * huber_val(d.reproj.a, d.reproj.b, d.reproj.k2, d.reproj.h, s) : 0.0;
    if (Hist) {
      rep_add(tab, H, 0, ok, sqrt(2.0 * (0.5 * s)), cost);
    } else {
      if (R.raw) R.raw[2 * t] = ok ? v.e[0] : 0.0, R.raw[2 * t + 1] = ok ? v.e[1] : 0.0;
      if (R.squ) R.squ[t] = 0.5 * s;
      if (R.cost) R.cost[t] = cost;
      if (R.valid) R.valid[t] = ok ? 1 : 0;
    }
  }
  if (Hist) rep_flush(tab, H);
}

// ------------------------------------------------------------------ launch wrappers
void launch_basemap_lin(const Dev& d, int updateCache, int dontRetry, hipStream_t st) {
  if (d.bm.n <= 0) return;
  hipLaunchKernelGGL(basemap_lin_kernel, dim3((unsigned)((d.bm.n + 255) / 256)), dim3(256), 0, st, d, updateCache, dontRetry);
  if (d.bm.nLmWith > 0)
    hipLaunchKernelGGL(basemap_sum_kernel, dim3((unsigned)((d.bm.nLmWith + 255) / 256)), dim3(256), 0, st, d);
}
void launch_basemap_cost(const Dev& d, int comparable, hipStream_t st) {
  if (d.bm.n <= 0) return;
  hipLaunchKernelGGL(basemap_cost_kernel, dim3((unsigned)((d.bm.n + 255) / 256)), dim3(256), 0, st, d, comparable);
}
void launch_basemap_rows(const Dev& d, const RepRows& R, hipStream_t st) {
  if (R.n <= 0) return;
  hipLaunchKernelGGL(basemap_report_kernel<false>, dim3((unsigned)((R.n + 255) / 256)), dim3(256), 0, st, d, R, RepHist{});
}
void launch_basemap_hist(const Dev& d, const RepHist& H, int blocks, hipStream_t st) {
  if (d.bm.n <= 0) return;
  const int64_t nb = std::min<int64_t>((d.bm.n + 255) / 256, std::max(1, blocks));
  hipLaunchKernelGGL(basemap_report_kernel<true>, dim3((unsigned)nb), dim3(256), 0, st, d, RepRows{}, H);
}

}  // namespace viba
