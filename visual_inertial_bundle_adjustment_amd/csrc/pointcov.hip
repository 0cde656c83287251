// Covariances of landmark points (gfx950; the point part of Optimizer::computeJointCovariances /
// computeCovariances, Optimizer.cpp:503-697, which this engine eliminates before it factors).
//
// After the covariance prologue (covariances.hip) the device holds, for a free point p, the Cholesky
// factor L_p of its damped 3 x 3 block (Vchol) and its panel Y_p = L_p^-1 W_p (3 x n_p, panel column c on
// reduced row pcRow[c]), and after the selected inversion (selinv.hip) the tiles of Z = S^-1 on the
// factor's pattern.  The variables a landmark touches are a clique of S, so every tile of Z_cc (c = the
// reduced rows of the panel's columns) is stored, and with H = [V W; W^T U], S = U - Y^T Y:
//   Sigma_pp = L_p^-T (I_3 + Y_p Z_cc Y_p^T) L_p^-1
//   Sigma_px = - L_p^-T Y_p Z_c,x                      (x a reduced variable of the panel)
//   Sigma_xx' = Z_x,x'
//
// One work item per requested point.  The product T = Y_p Z_cc is a gather of n_p^2 doubles for 3 n_p^2
// FMAs: M = 3 fills no fp64 MFMA block, so plain fp64 FMAs, accumulated in fp64 in both builds (Y is
// rec_t).  Lanes own target panel columns j and walk the source columns i from LDS; a tile is
// column-major and only tiles (I, K), I >= K, are stored, so the lanes read row r_j of the stored tile
// (tile of r_j, tile of r_i), coalesced along the row index, for the source columns whose tile is not
// above theirs: the diagonal tiles (both triangles stored by selinv_diag_kernel) and the strict lower
// part, which by the symmetry of Z_cc stands for the strict upper part too:
//   dl_j = sum_{i: tile(i) <= tile(j)} Z(r_j, r_i) y_i     lo_j = the same over tile(i) < tile(j)
//   Y Z Y^T = sum_j dl_j y_j^T + y_j lo_j^T
// The columns of T that a joint block needs (Sigma_px) are few: each is one pass with the lanes over the
// source columns i (coalesced where the source's tile is not above the column's).
//
// Panel width: narrow panels (<= kLmSmallCols columns) one wave per point, wider ones one workgroup per
// point, as the elimination splits them (landmark.hip).  The source columns are staged in LDS in chunks of
// kChunk columns, so LDS never depends on the panel: a panel wider than the chunk streams through it once
// per group of target columns.
#include "kernel_common.hpp"

namespace viba {

namespace {

// sum over the workgroup's threads (all of them call it); the result is valid in thread 0
template <int kThreads>
__device__ __forceinline__ double block_sum(double x, double* part, int tid) {
  x = wave_sum(x);
  if (kThreads == 64) return x;
  __syncthreads();  // the previous sum's readers are done with part
  if ((tid & 63) == 0) part[tid >> 6] = x;
  __syncthreads();
  double s = 0.0;
#pragma unroll
  for (int w = 0; w < kThreads / 64; w++) s += part[w];
  return s;
}

// Z(ra, rb) from the tile store: the stored tile is (max, min) of the two tile indices; a diagonal tile
// holds both triangles.  0 off the pattern (cannot happen inside a landmark's clique).
__device__ __forceinline__ double z_elem(const Dev& d, int32_t ra, int32_t rb) {
  if ((ra >> 6) < (rb >> 6)) {
    const int32_t t = ra;
    ra = rb, rb = t;
  }
  const int32_t t = d.tileIdx[(int64_t)(ra >> 6) * d.nT + (rb >> 6)];
  return t < 0 ? 0.0 : d.tiles[(int64_t)t * TS * TS + (rb & 63) * TS + (ra & 63)];
}

// request q = items[blockIdx.x]: point reqLm[q] (landmark index) with the extra panel columns
// xPc[xStart[q] .. xStart[q + 1]) (relative to the landmark's panel); its (3 + nx)^2 block, column-major,
// goes to out + outOff[q]
template <int kThreads, int kChunk>
__global__ void __launch_bounds__(kThreads) pointcov_kernel(Dev d, const int32_t* items, const int32_t* reqLm,
                                                            const int64_t* xStart, const int32_t* xPc,
                                                            const int64_t* outOff, double* out) {
  __shared__ double Ys[3 * kChunk];
  __shared__ int32_t Rs[kChunk];
  __shared__ double part[kThreads / 64];
  const int tid = threadIdx.x;
  const int64_t q = items[blockIdx.x];
  const int64_t l = reqLm[q];
  const int64_t cb = d.lmY[l] / 3;
  const int n = (int)(d.lmY[l + 1] / 3 - cb);
  const rec_t* Y = d.Y + d.lmY[l];  // plane q of panel column c at Y[3 c + q]
  const int32_t* rows = d.pcRow + cb;
  const int32_t nT = d.nT;
  const int64_t xs = xStart[q];
  const int nx = (int)(xStart[q + 1] - xs);
  const int N = 3 + nx;
  double* o = out + outOff[q];

  // M = Y Z_cc Y^T, lower triangle (m00 m10 m20 m11 m21 m22)
  double m[6] = {0, 0, 0, 0, 0, 0};
  int staged = -1;
  for (int j0 = 0; j0 < n; j0 += kThreads) {
    const int j = j0 + tid;
    const bool act = j < n;
    double y0 = 0, y1 = 0, y2 = 0;
    int32_t rj = 0;
    if (act) y0 = Y[3 * j], y1 = Y[3 * j + 1], y2 = Y[3 * j + 2], rj = rows[j];
    const int32_t Tj = rj >> 6;
    double dl0 = 0, dl1 = 0, dl2 = 0, lo0 = 0, lo1 = 0, lo2 = 0;
    for (int i0 = 0; i0 < n; i0 += kChunk) {
      const int cnt = min(kChunk, n - i0);
      if (staged != i0) {  // (uniform) the source columns [i0, i0 + cnt) into LDS
        __syncthreads();
        for (int c = tid; c < cnt; c += kThreads) {
          Ys[3 * c] = Y[3 * (i0 + c)], Ys[3 * c + 1] = Y[3 * (i0 + c) + 1], Ys[3 * c + 2] = Y[3 * (i0 + c) + 2];
          Rs[c] = rows[i0 + c];
        }
        __syncthreads();
        staged = i0;
      }
      for (int i = 0; i < cnt;) {  // by runs of source columns inside one tile (a variable's rows are consecutive)
        const int32_t Ti = __builtin_amdgcn_readfirstlane(Rs[i]) >> 6;
        int e = i + 1;
        while (e < cnt && (__builtin_amdgcn_readfirstlane(Rs[e]) >> 6) == Ti) e++;
        int64_t tb = -1;
        if (act && Ti <= Tj) {
          const int32_t t = d.tileIdx[(int64_t)Tj * nT + Ti];
          if (t >= 0) tb = (int64_t)t * TS * TS + (rj & 63);
        }
        if (tb >= 0) {
          double a0 = 0, a1 = 0, a2 = 0;
#pragma unroll 4
          for (int k = i; k < e; k++) {
            const double z = d.tiles[tb + (Rs[k] & 63) * TS];
            a0 += Ys[3 * k] * z, a1 += Ys[3 * k + 1] * z, a2 += Ys[3 * k + 2] * z;
          }
          dl0 += a0, dl1 += a1, dl2 += a2;
          if (Ti < Tj) lo0 += a0, lo1 += a1, lo2 += a2;
        }
        i = e;
      }
    }
    m[0] += dl0 * y0 + y0 * lo0, m[1] += dl1 * y0 + y1 * lo0, m[2] += dl2 * y0 + y2 * lo0;
    m[3] += dl1 * y1 + y1 * lo1, m[4] += dl2 * y1 + y2 * lo1, m[5] += dl2 * y2 + y2 * lo2;
  }
#pragma unroll
  for (int k = 0; k < 6; k++) m[k] = block_sum<kThreads>(m[k], part, tid);

  // L^-1 (lower) of the point's damped block
  const double* L = d.Vchol + l * 6;  // l00 l10 l20 l11 l21 l22
  const double i00 = 1.0 / L[0], i11 = 1.0 / L[3], i22 = 1.0 / L[5];
  const double i10 = -L[1] * i00 * i11, i21 = -L[4] * i11 * i22, i20 = -(L[2] * i00 + L[4] * i10) * i22;
  if (tid == 0) {
    // Sigma_pp = Li^T A Li, A = I + M: B = A Li, then the lower triangle of Li^T B, mirrored
    const double a00 = 1.0 + m[0], a10 = m[1], a20 = m[2], a11 = 1.0 + m[3], a21 = m[4], a22 = 1.0 + m[5];
    const double b00 = a00 * i00 + a10 * i10 + a20 * i20, b01 = a10 * i11 + a20 * i21;
    const double b10 = a10 * i00 + a11 * i10 + a21 * i20, b11 = a11 * i11 + a21 * i21;
    const double b20 = a20 * i00 + a21 * i10 + a22 * i20, b21 = a21 * i11 + a22 * i21, b22 = a22 * i22;
    const double s00 = i00 * b00 + i10 * b10 + i20 * b20;
    const double s10 = i11 * b10 + i21 * b20, s11 = i11 * b11 + i21 * b21;
    const double s20 = i22 * b20, s21 = i22 * b21, s22 = i22 * b22;
    (void)b01;
    o[0] = s00, o[1] = s10, o[2] = s20;
    o[N] = s10, o[N + 1] = s11, o[N + 2] = s21;
    o[2 * N] = s20, o[2 * N + 1] = s21, o[2 * N + 2] = s22;
  }
  if (nx == 0) return;

  // Sigma_px: column k of T = Y Z_cc at the extra panel column, lanes over the source columns
  for (int k = 0; k < nx; k++) {
    const int32_t rj = rows[xPc[xs + k]];
    double t0 = 0, t1 = 0, t2 = 0;
    for (int i = tid; i < n; i += kThreads) {
      const double z = z_elem(d, rows[i], rj);
      t0 += (double)Y[3 * i] * z, t1 += (double)Y[3 * i + 1] * z, t2 += (double)Y[3 * i + 2] * z;
    }
    t0 = block_sum<kThreads>(t0, part, tid);
    t1 = block_sum<kThreads>(t1, part, tid);
    t2 = block_sum<kThreads>(t2, part, tid);
    if (tid == 0) {
      const double v0 = -(i00 * t0 + i10 * t1 + i20 * t2), v1 = -(i11 * t1 + i21 * t2), v2 = -(i22 * t2);
      double* c = o + (int64_t)(3 + k) * N;
      c[0] = v0, c[1] = v1, c[2] = v2;
      o[3 + k] = v0, o[N + 3 + k] = v1, o[2 * N + 3 + k] = v2;
    }
  }
  // Sigma_xx': entries of Z
  for (int e = tid; e < nx * nx; e += kThreads) {
    const int a = e % nx, b = e / nx;
    o[(int64_t)(3 + b) * N + 3 + a] = z_elem(d, rows[xPc[xs + a]], rows[xPc[xs + b]]);
  }
}

}  // namespace

// requests items[0, nSmall) have panels of at most kLmSmallCols columns, items[nSmall, nSmall + nBig) wider
void launch_pointcov(const Dev& d, const int32_t* items, int64_t nSmall, int64_t nBig, const int32_t* reqLm,
                     const int64_t* xStart, const int32_t* xPc, const int64_t* outOff, double* out, hipStream_t st) {
  if (nSmall)
    hipLaunchKernelGGL((pointcov_kernel<64, kLmSmallCols>), dim3((unsigned)nSmall), dim3(64), 0, st, d, items, reqLm,
                       xStart, xPc, outOff, out);
  if (nBig)
    hipLaunchKernelGGL((pointcov_kernel<256, 1024>), dim3((unsigned)nBig), dim3(256), 0, st, d, items + nSmall, reqLm,
                       xStart, xPc, outOff, out);
}

}  // namespace viba
