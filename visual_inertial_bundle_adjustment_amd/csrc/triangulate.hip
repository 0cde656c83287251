// Initial landmark triangulation on the device (vb_triangulate_points, tools.hip).
//
// SingleSessionAdapter::initPointsFromObservations (viba/single_session/InitPointTracks.cpp:29-63) runs
// triangulatePoint (Triangulation.cpp:167-237) on every point track: a RANSAC over pairs of rays with the
// reference's own random sequence (findTriangulationCandidate, :34-97), then two Huber Gauss-Newton
// refinements (refineTriangulationResult, :99-161).  This file restates csrc/session.cpp (vbh_triangulate,
// the host form of the same stage) in two kernels, fp64 in both library variants:
//
//   triang_rays_kernel    one lane per observation: unproject, normalise, rotate into the world frame, camera
//                         centre.  The rays go to a scratch array in observation order, so a track of any
//                         length works, and the Newton loops of the Fisheye624 unprojection fill whole waves
//                         (a wave striding over its own track's observations would run them with n of 64 lanes).
//   triang_tracks_kernel  one wave per track, 4 tracks per 256-thread workgroup as refine_points_kernel:
//                         lane 0 draws the ray pairs (std::mt19937 state in shared memory, triang_core.hpp),
//                         every lane forms the candidate, the lanes stride over the rays / observations for
//                         the scores and the normal equations, which are summed by a fixed butterfly
//                         (__shfl_xor): every lane holds the same bits, and a pair drawn twice scores the
//                         same bits, so `angleSum < bestAngleSum` keeps the first as the host does.
//
// Outputs are zeroed by the caller; a rejected track leaves them zero.
#include <algorithm>

#include "device_math.hpp"
#include "engine.hpp"
#include "triang_core.hpp"

namespace viba {
using namespace triang;

namespace {

constexpr int kTracksPerBlock = 4;

__device__ __forceinline__ double tri_wave_sum(double x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}
__device__ __forceinline__ int tri_wave_sum(int x) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
  return x;
}

__device__ __forceinline__ Ray load_ray(const double* r) { return {{r[0], r[1], r[2]}, {r[3], r[4], r[5]}}; }

__global__ void __launch_bounds__(256) triang_rays_kernel(int64_t nObs, const double* Tcw, const int32_t* obsCam,
                                                          const double* cams, const double* uv, double* rays) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nObs; i += (int64_t)gridDim.x * 256) {
    const Ray r = observation_ray(Tcw + 7 * i, cams + 24 * (int64_t)obsCam[i], uv[2 * i], uv[2 * i + 1]);
    double* o = rays + 6 * i;
    o[0] = r.s.x, o[1] = r.s.y, o[2] = r.s.z, o[3] = r.d.x, o[4] = r.d.y, o[5] = r.d.z;
  }
}

// findTriangulationCandidate (Triangulation.cpp:34-97) over the n rays of one track; wave-uniform result
__device__ bool tri_candidate(const double* rays, int32_t n, int32_t seed, uint32_t* mtState, V3& best) {
  const int lane = threadIdx.x & 63;
  Mt19937 g{mtState, 0};
  if (lane == 0) mt_seed(g, mtState, seed);
  double bestAngleSum = INFINITY;
  int bestInl = 0;
  for (int it = 0; it < kNumRansac; it++) {
    int32_t a = 0, b = 0;
    if (lane == 0) draw_pair(g, n, a, b);  // the state is lane 0's alone
    a = __shfl(a, 0, 64), b = __shfl(b, 0, 64);
    V3 cand;
    if (!pair_candidate(load_ray(rays + 6 * (int64_t)a), load_ray(rays + 6 * (int64_t)b), cand)) continue;
    double angleSum = 0.0;
    int nInl = 0;
    for (int64_t q = lane; q < n; q += 64) {
      const double angle = ray_angle(load_ray(rays + 6 * q), cand);
      if (angle < kOutlierObservationRads) angleSum += angle, nInl++;
      else angleSum += kOutlierObservationRads;
    }
    angleSum = tri_wave_sum(angleSum), nInl = tri_wave_sum(nInl);
    if (nInl < kMinNumInliersInTriangulation) continue;
    if (angleSum < bestAngleSum) bestInl = nInl, best = cand, bestAngleSum = angleSum;
  }
  return bestInl >= kMinNumInliersInTriangulation;
}

// refineTriangulationResult (Triangulation.cpp:99-161): maxIt Gauss-Newton steps under a Huber loss over the
// track's n observations (arrays already offset to the track); inl[q] = image error below thr at the last step
__device__ int tri_refine(int32_t n, const double* Tcw, const int32_t* obsCam, const double* cams, const double* uv,
                          const double* sqrtH, V3& pt, double thr, bool skipOutliers, int maxIt, double lossRadius,
                          uint8_t* inl) {
  const int lane = threadIdx.x & 63;
  int nInl = 0;
  for (int it = 0; it < maxIt; it++) {
    double g0 = 0, g1 = 0, g2 = 0, h00 = 0, h10 = 0, h20 = 0, h11 = 0, h21 = 0, h22 = 0;
    int cnt = 0;
    for (int64_t q = lane; q < n; q += 64) {
      const double* T = Tcw + 7 * q;
      const double x = T[0], y = T[1], z = T[2], w = T[3];
      const double R[3][3] = {{1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)},
                              {2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)},
                              {2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)}};
      const dev::v3 pc = {R[0][0] * pt.x + R[0][1] * pt.y + R[0][2] * pt.z + T[4],
                          R[1][0] * pt.x + R[1][1] * pt.y + R[1][2] * pt.z + T[5],
                          R[2][0] * pt.x + R[2][1] * pt.y + R[2][2] * pt.z + T[6]};
      double img[2], J[6], Jp[30];
      uint8_t flag = 0;
      if (dev::project<true>(cams + 24 * (int64_t)obsCam[q], pc, img, J, Jp)) {  // a failed projection adds nothing
        const double e0 = img[0] - uv[2 * q], e1 = img[1] - uv[2 * q + 1];
        const double* S = sqrtH + 4 * q;
        const double we0 = S[0] * e0 + S[1] * e1, we1 = S[2] * e0 + S[3] * e1;
        const bool in = e0 * e0 + e1 * e1 < thr * thr;
        if (in) cnt++, flag = 1;
        if (in || !skipOutliers) {
          double D[2][3];  // sqrtH * J * R_cam_world
#pragma unroll
          for (int r = 0; r < 2; r++)
#pragma unroll
            for (int c = 0; c < 3; c++) {
              double s = 0;
#pragma unroll
              for (int k = 0; k < 3; k++) s += (S[2 * r] * J[k] + S[2 * r + 1] * J[3 + k]) * R[k][c];
              D[r][c] = s;
            }
          const double der = huber_der(lossRadius, we0 * we0 + we1 * we1);
          g0 += der * (we0 * D[0][0] + we1 * D[1][0]);
          g1 += der * (we0 * D[0][1] + we1 * D[1][1]);
          g2 += der * (we0 * D[0][2] + we1 * D[1][2]);
          h00 += der * (D[0][0] * D[0][0] + D[1][0] * D[1][0]);
          h10 += der * (D[0][1] * D[0][0] + D[1][1] * D[1][0]);
          h20 += der * (D[0][2] * D[0][0] + D[1][2] * D[1][0]);
          h11 += der * (D[0][1] * D[0][1] + D[1][1] * D[1][1]);
          h21 += der * (D[0][2] * D[0][1] + D[1][2] * D[1][1]);
          h22 += der * (D[0][2] * D[0][2] + D[1][2] * D[1][2]);
        }
      }
      if (it == maxIt - 1) inl[q] = flag;
    }
    nInl = tri_wave_sum(cnt);
    const double g[3] = {tri_wave_sum(g0), tri_wave_sum(g1), tri_wave_sum(g2)};
    const double H[3][3] = {{tri_wave_sum(h00), 0, 0}, {tri_wave_sum(h10), tri_wave_sum(h11), 0},
                            {tri_wave_sum(h20), tri_wave_sum(h21), tri_wave_sum(h22)}};
    // point -= H.llt().solve(grad); a pivot that is not positive skips the step and keeps the point
    double L[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 3; j++) {
      if (!ok) break;
      double d = H[j][j];
      for (int k = 0; k < j; k++) d -= L[j][k] * L[j][k];
      if (!(d > 0)) {
        ok = false;
        break;
      }
      L[j][j] = sqrt(d);
      for (int i = j + 1; i < 3; i++) {
        double s = H[i][j];
        for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
        L[i][j] = s / L[j][j];
      }
    }
    if (!ok) continue;
    double y[3], x[3];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      double s = g[i];
      for (int k = 0; k < i; k++) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 2; i >= 0; i--) {
      double s = y[i];
      for (int k = i + 1; k < 3; k++) s -= L[k][i] * x[k];
      x[i] = s / L[i][i];
    }
    pt = {pt.x - x[0], pt.y - x[1], pt.z - x[2]};
  }
  return nInl;
}

__global__ void __launch_bounds__(256) triang_tracks_kernel(int64_t nTracks, const int64_t* start, const int32_t* seed,
                                                            const double* Tcw, const int32_t* obsCam, const double* cams,
                                                            const double* uv, const double* sqrtH, const double* rays,
                                                            double* point, uint8_t* ok, uint8_t* inlier) {
  __shared__ uint32_t mtState[kTracksPerBlock][kMtN];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int64_t p = (int64_t)blockIdx.x * kTracksPerBlock + wave; p < nTracks;
       p += (int64_t)gridDim.x * kTracksPerBlock) {
    const int64_t b = start[p];
    const int32_t n = (int32_t)(start[p + 1] - b);
    if (n < kMinInlierObs) continue;
    V3 pt{0, 0, 0};
    if (!tri_candidate(rays + 6 * b, n, seed[p], mtState[wave], pt)) continue;
    uint8_t* inl = inlier + b;
    // refine 1 (threshold 3 px, outliers kept, Huber 1.5), refine 2 (2.5 px, outliers skipped, Huber 1.0)
    bool good = tri_refine(n, Tcw + 7 * b, obsCam + b, cams, uv + 2 * b, sqrtH + 4 * b, pt, 3.0, false, 3, 1.5, inl) >=
                kMinNumInliersAfterRefinement;
    good = good && tri_refine(n, Tcw + 7 * b, obsCam + b, cams, uv + 2 * b, sqrtH + 4 * b, pt, 2.5, true, 3, 1.0, inl) >=
                       kMinNumInliersAfterRefinement;
    if (!good) {  // each lane clears the flags it wrote itself
      for (int64_t q = lane; q < n; q += 64) inl[q] = 0;
      continue;
    }
    if (lane == 0) {
      ok[p] = 1;
      point[3 * p] = pt.x, point[3 * p + 1] = pt.y, point[3 * p + 2] = pt.z;
    }
  }
}

}  // namespace

void launch_triangulate(int64_t nTracks, int64_t nObs, const int64_t* start, const int32_t* seed, const double* Tcw,
                        const int32_t* obsCam, const double* cams, const double* uv, const double* sqrtH, double* rays,
                        double* point, uint8_t* ok, uint8_t* inlier, hipStream_t st) {
  constexpr int64_t kMaxBlocks = 1 << 22;  // the kernels stride over the rest
  if (nObs > 0)
    hipLaunchKernelGGL(triang_rays_kernel, dim3((unsigned)std::min<int64_t>((nObs + 255) / 256, kMaxBlocks)), dim3(256), 0,
                       st, nObs, Tcw, obsCam, cams, uv, rays);
  if (nTracks > 0)
    hipLaunchKernelGGL(triang_tracks_kernel,
                       dim3((unsigned)std::min<int64_t>((nTracks + kTracksPerBlock - 1) / kTracksPerBlock, kMaxBlocks)),
                       dim3(256), 0, st, nTracks, start, seed, Tcw, obsCam, cams, uv, sqrtH, rays, point, ok, inlier);
}

}  // namespace viba
