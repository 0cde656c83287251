// Calibration against factory on the device (gfx950): vb_calib_projection_offsets, the image projection offsets
// of SingleSessionAdapter::compareCalibrationVsFactory (viba/single_session/EvalCalibration.cpp:57-116).
//
// The reference walks a 20 x 15 px grid for every (rig, camera) entry of rigCamToModelIndex.  The rigs of one
// calibration window share their (intrinsics, extrinsics) variables, so one evaluation per distinct pair with
// the pair's rig count as a weight gives the same multiset of values.  fp64 in both library variants.
//
//   ce_grid_kernel    one lane per (factory camera, grid pixel): the +-3 px box check (four unproject +
//                     project round trips through the factory model) and the pixel's unit ray
//   ce_offset_kernel  one workgroup per (pair, 256 grid pixels), one lane per pixel, looping over the
//                     distances: pc = T_var (T_factory^-1 (ray d)), |px - project_var(pc)| into the value
//                     array (NaN = absent); the workgroup's sample count, sum and sum of squares per distance
//                     go to a slab by a fixed butterfly + wave order, no atomics
//   ce_stats_kernel   one workgroup per (series, distance): the slab rows of the series' pairs times their
//                     weights, lanes striding over the rows and a fixed tree over the lanes -> count, mean,
//                     rmse, and the two ranks floor / ceil of pct / 100 (N - 1) for p50 and p90
//   ce_hist_kernel    radix select, one 8-bit digit per pass from the top: the values are non-negative doubles,
//   ce_pick_kernel    so their bit patterns order as unsigned integers.  A workgroup (one pair, one distance)
//                     bins the keys that still match a rank's prefix into an LDS table of 4 ranks x 256 int64
//                     weights and adds its non-zero bins to the global table (64-bit integer atomics: exact and
//                     order-free); ce_pick_kernel walks the 256 bins of a rank to the digit holding it, extends
//                     the prefix and clears the bins.  After eight passes the prefix is the value of the rank.
//   ce_quantile_kernel  StatsValueContainer::pX's interpolation of the two ranks
//
// The kernels read the handle's camera variables and write only buffers of this call.
#include <algorithm>
#include <cmath>
#include <limits>

#include "device_math.hpp"
#include "host.hpp"
#include "triang_core.hpp"

namespace viba {
namespace {

constexpr int kCeBlock = 256;
constexpr double kCeStepX = 20.0, kCeStepY = 15.0;  // EvalCalibration.cpp:73
constexpr int kCeRanks = 4;                         // p50 below / above, p90 below / above

struct CeGrid {  // the grid of one factory camera: x = x0 + 20 ix, y = y0 + 15 iy, pixel g = ix * ny + iy
  double x0, y0;
  int32_t nx, ny;
};

struct CeArgs {
  int32_t nF, maxGrid, nDist, nSeries, bpp;  // bpp: workgroups per pair = ceil(maxGrid / 256)
  int64_t nPairs;
  const CeGrid* grid;
  const double *fcam, *fT, *varIntr, *varExtr, *dist;
  const int32_t *intrVar, *extrVar, *fcamOfPair, *seriesOfPair;
  const int64_t* weight;
  uint8_t* valid;  // nF x maxGrid
  double* ray;     // nF x maxGrid x 3
  double* values;  // nPairs x nDist x maxGrid
  // slab: per (workgroup of ce_offset_kernel, distance)
  int64_t* slabN;
  double *slabS, *slabQ;
  // per (series, distance)
  int64_t* count;
  double *mean, *rmse, *p50, *p90;
  // per (series, distance, rank): rank still to find within the prefix, prefix, bins
  int64_t* rankLeft;
  unsigned long long *prefix, *bins;
};

__device__ __forceinline__ double ce_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ int ce_wave_sum(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__global__ void __launch_bounds__(kCeBlock) ce_grid_kernel(CeArgs A) {
  const int64_t t = (int64_t)blockIdx.x * kCeBlock + threadIdx.x;
  if (t >= (int64_t)A.nF * A.maxGrid) return;
  const int32_t c = (int32_t)(t / A.maxGrid), g = (int32_t)(t % A.maxGrid);
  const CeGrid G = A.grid[c];
  uint8_t ok = 0;
  triang::V3 n = {0.0, 0.0, 0.0};
  if (g < G.nx * G.ny) {
    const double* cam = A.fcam + VB_CAM_DATA * (int64_t)c;
    const double px = G.x0 + kCeStepX * (g / G.ny), py = G.y0 + kCeStepY * (g % G.ny);
    bool bad = false;  // a 6 x 6 box around px must be valid for the projection (:80-95)
#pragma unroll 1
    for (int p = 0; p < 4; p++) {
      const double u = px + ((p & 1) ? -3.0 : 3.0), v = py + ((p & 2) ? -3.0 : 3.0);
      const triang::V3 r = triang::unproject(cam, u, v);
      double uv[2];
      const bool projOk = dev::project<false>(cam, dev::v3{r.x, r.y, r.z}, uv, nullptr, nullptr);
      const double du = u - uv[0], dv = v - uv[1];
      if (!projOk || du * du + dv * dv > 1e-6) bad = true;
    }
    if (!bad) {
      const triang::V3 r = triang::unproject(cam, px, py);
      n = triang::scl3(1.0 / triang::norm3(r), r);
      ok = 1;
    }
  }
  A.valid[t] = ok;
  A.ray[3 * t] = n.x, A.ray[3 * t + 1] = n.y, A.ray[3 * t + 2] = n.z;
}

__global__ void __launch_bounds__(kCeBlock) ce_offset_kernel(CeArgs A) {
  __shared__ int sN[kCeBlock / 64];
  __shared__ double sS[kCeBlock / 64], sQ[kCeBlock / 64];
  const int64_t pair = blockIdx.x / A.bpp;
  const int32_t g = (int32_t)(blockIdx.x % A.bpp) * kCeBlock + threadIdx.x;
  const int32_t fc = A.fcamOfPair[pair];
  const bool inGrid = g < A.maxGrid;
  const bool live = inGrid && A.valid[(int64_t)fc * A.maxGrid + g];
  const CeGrid G = A.grid[fc];
  const double* cam = A.varIntr + VB_CAM_DATA * (int64_t)A.intrVar[pair];
  const double* Tv = A.varExtr + 7 * (int64_t)A.extrVar[pair];
  const double* Tf = A.fT + 7 * (int64_t)fc;
  const dev::q4 qv = {Tv[0], Tv[1], Tv[2], Tv[3]}, qfi = dev::qinv(dev::q4{Tf[0], Tf[1], Tf[2], Tf[3]});
  const dev::v3 tv = {Tv[4], Tv[5], Tv[6]};
  // Sophus inverse(): (q^-1, q^-1 * (-t))
  const dev::v3 tfi = dev::qrot(qfi, dev::v3{-Tf[4], -Tf[5], -Tf[6]});
  dev::v3 ray = {0.0, 0.0, 0.0};
  double px = 0.0, py = 0.0;
  if (live) {
    const double* r = A.ray + 3 * ((int64_t)fc * A.maxGrid + g);
    ray = {r[0], r[1], r[2]};
    px = G.x0 + kCeStepX * (g / G.ny), py = G.y0 + kCeStepY * (g % G.ny);
  }
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int32_t d = 0; d < A.nDist; d++) {
    double val = std::numeric_limits<double>::quiet_NaN();
    if (live) {
      const dev::v3 pb = dev::add(dev::qrot(qfi, dev::scl(A.dist[d], ray)), tfi);
      const dev::v3 pc = dev::add(dev::qrot(qv, pb), tv);
      double uv[2];
      if (dev::project<false>(cam, pc, uv, nullptr, nullptr)) {
        const double du = px - uv[0], dv = py - uv[1];
        val = sqrt(du * du + dv * dv);
      }
    }
    if (inGrid) A.values[(pair * A.nDist + d) * A.maxGrid + g] = val;
    const bool has = val == val;
    const int n = ce_wave_sum(has ? 1 : 0);
    const double s = ce_wave_sum(has ? val : 0.0), q = ce_wave_sum(has ? val * val : 0.0);
    if (lane == 0) sN[wave] = n, sS[wave] = s, sQ[wave] = q;
    __syncthreads();
    if (threadIdx.x == 0) {
      int nn = 0;
      double ss = 0.0, qq = 0.0;
      for (int w = 0; w < kCeBlock / 64; w++) nn += sN[w], ss += sS[w], qq += sQ[w];
      const int64_t o = (int64_t)blockIdx.x * A.nDist + d;
      A.slabN[o] = nn, A.slabS[o] = ss, A.slabQ[o] = qq;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kCeBlock) ce_stats_kernel(CeArgs A) {
  __shared__ long long sN[kCeBlock];
  __shared__ double sS[kCeBlock], sQ[kCeBlock];
  const int32_t s = blockIdx.x / A.nDist, d = blockIdx.x % A.nDist;
  long long n = 0;
  double sum = 0.0, sq = 0.0;
  const int64_t nBlk = A.nPairs * A.bpp;
  for (int64_t b = threadIdx.x; b < nBlk; b += kCeBlock) {
    const int64_t pair = b / A.bpp;
    if (A.seriesOfPair[pair] != s) continue;
    const int64_t w = A.weight[pair], o = b * A.nDist + d;
    n += w * A.slabN[o], sum += (double)w * A.slabS[o], sq += (double)w * A.slabQ[o];
  }
  sN[threadIdx.x] = n, sS[threadIdx.x] = sum, sQ[threadIdx.x] = sq;
  __syncthreads();
  for (int off = kCeBlock / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      sN[threadIdx.x] += sN[threadIdx.x + off];
      sS[threadIdx.x] += sS[threadIdx.x + off];
      sQ[threadIdx.x] += sQ[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int64_t N = sN[0];
    const int64_t o = blockIdx.x;
    const double nan = std::numeric_limits<double>::quiet_NaN();
    A.count[o] = N;
    A.mean[o] = N > 0 ? sS[0] / (double)N : nan;
    A.rmse[o] = N > 0 ? sqrt(sQ[0] / (double)N) : nan;
    // StatsValueContainer::pX: pos = (percentile / 100.0) * (size - 1)
    const double pos50 = (50.0 / 100.0) * (double)(N - 1), pos90 = (90.0 / 100.0) * (double)(N - 1);
    int64_t* rl = A.rankLeft + kCeRanks * o;
    rl[0] = N > 0 ? (int64_t)floor(pos50) : 0, rl[1] = N > 0 ? (int64_t)ceil(pos50) : 0;
    rl[2] = N > 0 ? (int64_t)floor(pos90) : 0, rl[3] = N > 0 ? (int64_t)ceil(pos90) : 0;
    for (int r = 0; r < kCeRanks; r++) A.prefix[kCeRanks * o + r] = 0ull;
  }
}

// one pass of the radix select: digit (key >> shift) & 255 of the keys whose higher digits equal the rank's prefix
__global__ void __launch_bounds__(kCeBlock) ce_hist_kernel(CeArgs A, int shift) {
  __shared__ unsigned long long tab[kCeRanks][256];
  for (int r = 0; r < kCeRanks; r++) tab[r][threadIdx.x] = 0ull;
  __syncthreads();
  const int64_t blk = blockIdx.x / A.nDist;  // workgroup of ce_offset_kernel
  const int32_t d = (int32_t)(blockIdx.x % A.nDist);
  const int64_t pair = blk / A.bpp;
  const int32_t g = (int32_t)(blk % A.bpp) * kCeBlock + threadIdx.x;
  const unsigned long long w = (unsigned long long)A.weight[pair];
  const int64_t sd = (int64_t)A.seriesOfPair[pair] * A.nDist + d;
  double val = std::numeric_limits<double>::quiet_NaN();
  if (g < A.maxGrid) val = A.values[(pair * A.nDist + d) * A.maxGrid + g];
  const bool has = val == val && w > 0;
  const unsigned long long key = (unsigned long long)__double_as_longlong(val);
  const unsigned digit = (unsigned)(key >> shift) & 255u;
  for (int r = 0; r < kCeRanks; r++) {
    const bool m = has && (shift == 56 || (key >> (shift + 8)) == (A.prefix[kCeRanks * sd + r] >> (shift + 8)));
    // the samples of one pair lie close together: when a wave's matching keys share the digit, one add
    const unsigned long long mask = __ballot(m);
    if (mask == 0ull) continue;
    const int first = __ffsll((long long)mask) - 1;
    const unsigned digit0 = (unsigned)__shfl((int)digit, first, 64);
    if (__ballot(m && digit == digit0) == mask) {
      if ((int)(threadIdx.x & 63) == first) atomicAdd(&tab[r][digit0], w * (unsigned long long)__popcll(mask));
    } else if (m) {
      atomicAdd(&tab[r][digit], w);
    }
  }
  __syncthreads();
  for (int r = 0; r < kCeRanks; r++) {
    const unsigned long long c = tab[r][threadIdx.x];
    if (c) atomicAdd(&A.bins[(kCeRanks * sd + r) * 256 + threadIdx.x], c);
  }
}

// one workgroup per (series, distance, rank): the digit whose bins hold the rank, then the bins are cleared
__global__ void __launch_bounds__(256) ce_pick_kernel(CeArgs A, int shift) {
  __shared__ unsigned long long c[256];
  const int64_t sel = blockIdx.x;
  c[threadIdx.x] = A.bins[sel * 256 + threadIdx.x];
  A.bins[sel * 256 + threadIdx.x] = 0ull;
  __syncthreads();
  if (threadIdx.x != 0 || A.count[sel / kCeRanks] <= 0) return;
  const unsigned long long k = (unsigned long long)A.rankLeft[sel];
  unsigned long long cum = 0ull;
  int digit = 255;
  for (int b = 0; b < 256; b++) {
    if (k < cum + c[b]) {
      digit = b;
      break;
    }
    cum += c[b];
  }
  A.prefix[sel] |= (unsigned long long)digit << shift;
  A.rankLeft[sel] = (int64_t)(k - cum);
}

__global__ void __launch_bounds__(64) ce_quantile_kernel(CeArgs A) {
  const int64_t o = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (o >= (int64_t)A.nSeries * A.nDist) return;
  const int64_t N = A.count[o];
  const double nan = std::numeric_limits<double>::quiet_NaN();
  double out[2] = {nan, nan};
  if (N > 0) {
    const double pct[2] = {50.0, 90.0};
    for (int i = 0; i < 2; i++) {
      const double lo = __longlong_as_double((long long)A.prefix[kCeRanks * o + 2 * i]);
      const double hi = __longlong_as_double((long long)A.prefix[kCeRanks * o + 2 * i + 1]);
      const double pos = (pct[i] / 100.0) * (double)(N - 1);
      const double below = floor(pos);
      if (below == ceil(pos)) {
        out[i] = lo;
      } else {
        const double wa = pos - below, wb = 1.0 - wa;
        out[i] = lo * wb + hi * wa;
      }
    }
  }
  A.p50[o] = out[0], A.p90[o] = out[1];
}

}  // namespace
}  // namespace viba

extern "C" {

int vb_calib_projection_offsets(vb_handle h, int32_t n_fcam, const double* factory_cam,
                                const double* factory_T_cam_bodyimu, int64_t n_pairs, const int32_t* cam_intr_var,
                                const int32_t* cam_extr_var, const int32_t* fcam_of_pair, const int64_t* weight,
                                const int32_t* series_of_pair, int32_t n_series, int32_t n_dist,
                                const double* distances, int64_t* count, double* mean, double* rmse, double* p50,
                                double* p90, double* values, uint8_t* valid) {
  const char* what = "vb_calib_projection_offsets";
  if (!h) return fail(VB_E_ARG, std::string(what) + ": null handle");
  if (!h->fin) return fail(VB_E_STATE, std::string(what) + " before vb_finalize");
  const Dev& d = h->fin->d;
  if (!wholeProblem(h))
    return fail(VB_E_UNSUPPORTED, std::string(what) + " needs the whole problem on this handle (no shard / partition)");
  if (n_dist <= 0 || !distances) return fail(VB_E_ARG, std::string(what) + ": n_dist must be positive");
  if (n_series <= 0 || n_fcam < 0 || n_pairs < 0) return fail(VB_E_ARG, std::string(what) + ": bad count");
  if ((n_fcam && (!factory_cam || !factory_T_cam_bodyimu)) ||
      (n_pairs && (!cam_intr_var || !cam_extr_var || !fcam_of_pair || !weight || !series_of_pair)))
    return fail(VB_E_ARG, std::string(what) + ": NULL array with a non-zero count");
  for (int32_t i = 0; i < n_dist; i++)
    if (!std::isfinite(distances[i])) return fail(VB_E_ARG, std::string(what) + ": non-finite distance");
  // the grids: x = fmod(w / 2, 20), + 20, ... < w; y = fmod(h / 2, 15), + 15, ... < h (:73-77)
  std::vector<CeGrid> grid(n_fcam);
  int32_t maxGrid = 0;
  for (int32_t c = 0; c < n_fcam; c++) {
    const double* cam = factory_cam + VB_CAM_DATA * (size_t)c;
    if (cam[0] != (double)VB_CAM_LINEAR && cam[0] != (double)VB_CAM_FISHEYE624)
      return fail(VB_E_ARG, std::string(what) + ": factory camera record with an unknown model");
    const double w = cam[2], hh = cam[3];
    if (!(w >= 1 && w <= 32767 && hh >= 1 && hh <= 32767))
      return fail(VB_E_ARG, std::string(what) + ": factory camera image size outside [1, 32767]");
    CeGrid& G = grid[c];
    G.x0 = std::fmod(w * 0.5, kCeStepX), G.y0 = std::fmod(hh * 0.5, kCeStepY), G.nx = G.ny = 0;
    for (double x = G.x0; x < w; x += kCeStepX) G.nx++;
    for (double y = G.y0; y < hh; y += kCeStepY) G.ny++;
    maxGrid = std::max(maxGrid, G.nx * G.ny);
  }
  const int64_t nIntr = (int64_t)h->prob.data[VB_VAR_CAM_INTR].size() / VB_CAM_DATA;
  const int64_t nExtr = (int64_t)h->prob.data[VB_VAR_CAM_EXTR].size() / 7;
  for (int64_t p = 0; p < n_pairs; p++) {
    if (cam_intr_var[p] < 0 || cam_intr_var[p] >= nIntr || cam_extr_var[p] < 0 || cam_extr_var[p] >= nExtr)
      return fail(VB_E_ARG, std::string(what) + ": camera variable index out of range");
    if (fcam_of_pair[p] < 0 || fcam_of_pair[p] >= n_fcam)
      return fail(VB_E_ARG, std::string(what) + ": factory camera index out of range");
    if (weight[p] < 0) return fail(VB_E_ARG, std::string(what) + ": negative weight");
    if (series_of_pair[p] < 0 || series_of_pair[p] >= n_series)
      return fail(VB_E_ARG, std::string(what) + ": series out of range");
  }
  const size_t nSD = (size_t)n_series * n_dist;
  const double nan = std::numeric_limits<double>::quiet_NaN();
  h->run.calibEvalMs = 0.0;
  if (n_pairs == 0 || maxGrid == 0) {  // no sample anywhere
    for (size_t i = 0; i < nSD; i++) {
      if (count) count[i] = 0;
      if (mean) mean[i] = nan;
      if (rmse) rmse[i] = nan;
      if (p50) p50[i] = nan;
      if (p90) p90[i] = nan;
    }
    return 0;
  }
  CeArgs A{};
  A.nF = n_fcam, A.maxGrid = maxGrid, A.nDist = n_dist, A.nSeries = n_series, A.nPairs = n_pairs;
  A.bpp = (maxGrid + kCeBlock - 1) / kCeBlock;
  const int64_t nBlk = n_pairs * A.bpp;
  if (nBlk * n_dist >= ((int64_t)1 << 31)) return fail(VB_E_ARG, std::string(what) + ": too many pairs for one call");
  HIPCHK(hipSetDevice(h->cfg.device));
  hipStream_t st = h->str.st;
  DevOwner S;  // frees its buffers and events when the call returns, on every path
  hipEvent_t ev[2] = {nullptr, nullptr};
  const size_t nFG = (size_t)n_fcam * maxGrid, nVal = (size_t)n_pairs * n_dist * maxGrid;
  if (S.put(&A.grid, grid.data(), grid.size(), st) || S.put(&A.fcam, factory_cam, (size_t)n_fcam * VB_CAM_DATA, st) ||
      S.put(&A.fT, factory_T_cam_bodyimu, (size_t)n_fcam * 7, st) || S.put(&A.dist, distances, n_dist, st) ||
      S.put(&A.intrVar, cam_intr_var, n_pairs, st) || S.put(&A.extrVar, cam_extr_var, n_pairs, st) ||
      S.put(&A.fcamOfPair, fcam_of_pair, n_pairs, st) || S.put(&A.seriesOfPair, series_of_pair, n_pairs, st) ||
      S.put(&A.weight, weight, n_pairs, st) || S.get(&A.valid, nFG) || S.get(&A.ray, 3 * nFG) ||
      S.get(&A.values, nVal) || S.get(&A.slabN, (size_t)nBlk * n_dist) || S.get(&A.slabS, (size_t)nBlk * n_dist) ||
      S.get(&A.slabQ, (size_t)nBlk * n_dist) || S.get(&A.count, nSD) || S.get(&A.mean, nSD) || S.get(&A.rmse, nSD) ||
      S.get(&A.p50, nSD) || S.get(&A.p90, nSD) || S.get(&A.rankLeft, kCeRanks * nSD) ||
      S.get(&A.prefix, kCeRanks * nSD) || S.get(&A.bins, kCeRanks * nSD * 256) || S.event(&ev[0]) || S.event(&ev[1]))
    return devFail(S, std::string(what) + ": device allocation");
  A.varIntr = d.var[VB_VAR_CAM_INTR], A.varExtr = d.var[VB_VAR_CAM_EXTR];
  HIPCHK(hipMemsetAsync(A.bins, 0, kCeRanks * nSD * 256 * sizeof(unsigned long long), st));
  HIPCHK(hipEventRecord(ev[0], st));
  hipLaunchKernelGGL(ce_grid_kernel, dim3((unsigned)((nFG + kCeBlock - 1) / kCeBlock)), dim3(kCeBlock), 0, st, A);
  hipLaunchKernelGGL(ce_offset_kernel, dim3((unsigned)nBlk), dim3(kCeBlock), 0, st, A);
  hipLaunchKernelGGL(ce_stats_kernel, dim3((unsigned)nSD), dim3(kCeBlock), 0, st, A);
  for (int shift = 56; shift >= 0; shift -= 8) {
    hipLaunchKernelGGL(ce_hist_kernel, dim3((unsigned)(nBlk * n_dist)), dim3(kCeBlock), 0, st, A, shift);
    hipLaunchKernelGGL(ce_pick_kernel, dim3((unsigned)(kCeRanks * nSD)), dim3(256), 0, st, A, shift);
  }
  hipLaunchKernelGGL(ce_quantile_kernel, dim3((unsigned)((nSD + 63) / 64)), dim3(64), 0, st, A);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(ev[1], st));
  if (download(count, A.count, nSD, st) || download(mean, A.mean, nSD, st) || download(rmse, A.rmse, nSD, st) ||
      download(p50, A.p50, nSD, st) || download(p90, A.p90, nSD, st) || download(values, A.values, nVal, st) ||
      download(valid, A.valid, nFG, st))
    return VB_E_HIP;
  HIPCHK(hipStreamSynchronize(st));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, ev[0], ev[1]));
  h->run.calibEvalMs = ms;
  return 0;
}

int vb_calib_eval_device_ms(vb_handle h, double* ms) {
  if (!h || !ms) return fail(VB_E_ARG, "vb_calib_eval_device_ms: null argument");
  *ms = h->run.calibEvalMs;
  return 0;
}

}  // extern "C"
