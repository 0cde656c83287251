// Diagonal blocks and rows of the level-scheduled tile Cholesky (gfx950), replacing BaSpaCho's supernodal
// Cholesky (Optimizer.cpp:200-231), over the building blocks of tile_chol.hpp; the forward solve rides
// these launches (fwdB / fwdY).  Per elimination level, after the level's fan-in (fanin.hip):
//   potrf4_kernel          column schedule: 64 x 64 diagonal tiles (+ their 16 x 16 block inverses)
//   trsm_kernel            column schedule: off-diagonal L_IJ = A_IJ L_JJ^-T
//   potrf_trsm_kernel      column schedule: both in one launch (levels with few off-diagonal tiles)
//   snpotrf8_kernel        two-column supernodes: the 128 x 128 diagonal block
//   sntrsm_kernel          two-column supernodes: the rows below the block
//   snpotrf_trsm8_kernel   two-column supernodes: both in one launch (levels with few rows)
//   copy_diag_kernel       the fused levels' diagonal tiles back from the scratch
//   diag_inverse_kernel    64 x 64 inverses of the factored diagonal tiles (for the triangular solves)
//   pad_diag_kernel        identity on the diagonal of the padding rows
#include "tile_chol.hpp"

namespace viba {

// ---------------- column schedule (factorSeq in factor_host.hip)
// factor diagonal tile tiles[b] in place (+ its 16 x 16 block inverses into dinv[cols[b]]); four waves
// per tile, all the diagonal tiles of one level per launch; with fwdB also y_J = L_JJ^-1 b_J
__global__ void __launch_bounds__(256) potrf4_kernel(Dev d, const int32_t* tileList, const int32_t* cols,
                                                     double* dinvAll, const double* fwdB, double* fwdY) {
  __shared__ double T[TS * TS];
  __shared__ double scratch[256];
  __shared__ double dinvS[1024];
  const int tid = threadIdx.x, w = tid >> 6;
  double* A = d.tiles + (int64_t)tileList[blockIdx.x] * TS * TS;
  double* dinvG = dinvAll + (int64_t)cols[blockIdx.x] * 1024;
  potrf_core<4, TS>(d, A, nullptr, nullptr, T, scratch, dinvS, tid);
  if (fwdB && w == 0) potrf_forward(d, T, dinvS, scratch, cols[blockIdx.x], fwdB + (int64_t)cols[blockIdx.x] * TS, fwdY, tid & 63);
  lds_to_global(A, T, TS * TS, tid, 256);
  lds_to_global(dinvG, dinvS, 1024, tid, 256);
}

// potrf + trsm of a level in ONE launch (the levels with few off-diagonal tiles, where the two launches
// and the dependency between them cost more than the work): one block per off-diagonal tile (I, J)
// factors L_JJ itself -- every block of column J computes the identical factor from the untouched A_JJ
// -- then forms L_IJ = A_IJ L_JJ^-T from LDS (its A_IJ loaded before the factorization).  One block
// per column (writer) stores L_JJ into the scratch Lscr (A_JJ is still being read by the others; the
// diagonal tiles are copied back after the last level: copy_diag_kernel) and the inverses into dinv.
// With the fused forward solve every block also derives y_J (only the writer stores it) for its
// b_I -= L_IJ y_J.  items: (diagonal tile, column, target tile or -1, target row, writer) per block.
__global__ void __launch_bounds__(256) potrf_trsm_kernel(Dev d, const int32_t* items, double* Lscr, double* dinvAll,
                                                         double* fwdB, double* fwdY) {
  __shared__ double T[TS * TS];
  __shared__ double scratch[256];
  __shared__ double dinvS[1024];
  const int32_t* it = items + 5 * (int64_t)blockIdx.x;
  const int32_t diagT = it[0], col = it[1], target = it[2], row = it[3], writer = it[4];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  double* At = target >= 0 ? d.tiles + (int64_t)target * TS * TS : nullptr;
  double4_t a[4];
  if (At) load_rows(At, a, w, lr, lq);
  potrf_core<4, TS>(d, d.tiles + (int64_t)diagT * TS * TS, nullptr, nullptr, T, scratch, dinvS, tid);
  if (fwdB && w == 0) potrf_forward(d, T, dinvS, scratch, col, fwdB + (int64_t)col * TS, fwdY, lane, writer != 0);
  if (writer) {
    lds_to_global(Lscr + (int64_t)col * TS * TS, T, TS * TS, tid, 256);
    lds_to_global(dinvAll + (int64_t)col * 1024, dinvS, 1024, tid, 256);
  }
  if (!At) return;
  __syncthreads();  // y_J (scratch[0, 64)) from wave 0
  double4_t Xt[4];
  trsm_lds<4, TS>(T, dinvS, a, Xt, lr, lq);
  store_rows(At, Xt, w, lr, lq);
  if (fwdB) fwd_sub(fwdB + (int64_t)row * TS, lane_dot(Xt, scratch, lq), w, lr, lq);
}

// X = A L_JJ^-T for target tile target[b] with diagonal tile diag[b] of column cols[b]; wave w =
// 16-row block (all on MFMA); every off-diagonal tile of one level per launch
__global__ void __launch_bounds__(256) trsm_kernel(Dev d, const int32_t* diagList, const int32_t* targetList,
                                                   const int32_t* cols, const double* dinvAll, const int32_t* rows,
                                                   const double* fwdY, double* fwdB) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  double* A = d.tiles + (int64_t)targetList[blockIdx.x] * TS * TS;
  double4_t a[4], Xt[4], yv[4];
  load_rows(A, a, w, lr, lq);
  // y_J of the fused forward solve, in flight with the other operands ahead of the substitution chain
  if (fwdB) load_cols(fwdY + (int64_t)cols[blockIdx.x] * TS, yv, lq);
  trsm_rows(d.tiles + (int64_t)diagList[blockIdx.x] * TS * TS, dinvAll + (int64_t)cols[blockIdx.x] * 1024, a, Xt, lr, lq);
  store_rows(A, Xt, w, lr, lq);
  if (fwdB) fwd_sub(fwdB + (int64_t)rows[blockIdx.x] * TS, lane_dot(Xt, yv), w, lr, lq);  // b_I -= L_IJ y_J
}

// ---------------- two-column supernodes (SnSched in host.hpp)
// Two-column supernode diagonal block on eight waves (items: tile (J, J), J, tile (J + 1, J) or -1, tile
// (J + 1, J + 1) or -1): the 128 x 128 Cholesky right-looking by 16-column blocks (8 diag16 steps: the two
// 64-wide chains with the L21 solve and the A22 update folded into the same block loop), the 16 x 16
// inverses, the fused forward solve.  A one-column supernode runs the 64-wide form on waves 0-3.
__global__ void __launch_bounds__(512) snpotrf8_kernel(Dev d, const int32_t* items, double* dinvAll, const double* fwdB,
                                                       double* fwdY) {
  __shared__ double T[128 * 128];
  __shared__ double scratch[256];
  __shared__ double dinvS[8 * 256];
  __shared__ double yb[256];
  const int32_t* it = items + 4 * (int64_t)blockIdx.x;
  const int32_t t11 = it[0], J = it[1], t21 = it[2], t22 = it[3];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  double* A11 = d.tiles + (int64_t)t11 * TS * TS;
  if (t21 < 0) {
    potrf_core<4, 128>(d, A11, nullptr, nullptr, T, scratch, dinvS, tid, fwdB ? fwdB + (int64_t)J * TS : nullptr,
                       nullptr, yb);
    if (fwdB && w == 0) {
      const int64_t row = (int64_t)J * TS + lane;
      fwdY[row] = row < d.nRed ? yb[128 + lane] : 0.0;
    }
    store_block_tiles<4, 128>(A11, nullptr, nullptr, T, tid, 512);
    for (int i = tid; i < 1024; i += 512) dinvAll[(int64_t)J * 1024 + i] = dinvS[i];
    return;
  }
  double* A21 = d.tiles + (int64_t)t21 * TS * TS;
  double* A22 = d.tiles + (int64_t)t22 * TS * TS;
  potrf_core<8, 128>(d, A11, A21, A22, T, scratch, dinvS, tid, fwdB ? fwdB + (int64_t)J * TS : nullptr,
                     fwdB ? fwdB + (int64_t)(J + 1) * TS : nullptr, yb);
  if (fwdB && w < 2) {
    const int64_t row = (int64_t)(J + w) * TS + lane;
    fwdY[row] = row < d.nRed ? yb[128 + 64 * w + lane] : 0.0;
  }
  store_block_tiles<8, 128>(A11, A21, A22, T, tid, 512);
  for (int i = tid; i < 2048; i += 512) dinvAll[(int64_t)J * 1024 + i] = dinvS[i];  // J and J + 1, consecutive
}

// Levels with few rows: the supernode's diagonal block and ONE of its rows per block (potrf_trsm_kernel
// for supernodes).  Every block of a supernode factors the diagonal block itself from the untouched tiles
// (identical result), then forms its row [L_I1 L_I2] = [A_I1 A_I2] L^-T from LDS; the writer block
// stores L11 / L22 into Lscr[J] / Lscr[J + 1] and L21 into Lscr[nT + J] (the tiles are still being read
// by the others; copy_diag_kernel puts them back after the last level), the inverses and y.
// items: tile (J, J), J, tile (J + 1, J) or -1, tile (J + 1, J + 1), tile (I, J) or -1, tile (I, J + 1) or
// -1, I (or -1: no row), writer
__global__ void __launch_bounds__(512) snpotrf_trsm8_kernel(Dev d, const int32_t* items, double* Lscr, double* dinvAll,
                                                            double* fwdB, double* fwdY) {
  __shared__ double T[128 * 128];
  __shared__ double scratch[256];
  __shared__ double dinvS[8 * 256];
  __shared__ double yb[256];
  const int32_t* it = items + 8 * xcd_block(blockIdx.x, gridDim.x);  // one supernode's rows on one XCD
  const int32_t t11 = it[0], J = it[1], t21 = it[2], t22 = it[3], tI1 = it[4], tI2 = it[5], I = it[6], writer = it[7];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  const bool two = t21 >= 0;
  const int64_t nT = d.nT;
  const double* A11 = d.tiles + (int64_t)t11 * TS * TS;
  const double* b0 = fwdB ? fwdB + (int64_t)J * TS : nullptr;
  if (two)
    potrf_core<8, 128>(d, A11, d.tiles + (int64_t)t21 * TS * TS, d.tiles + (int64_t)t22 * TS * TS, T, scratch, dinvS, tid,
                       b0, fwdB ? fwdB + (int64_t)(J + 1) * TS : nullptr, yb);
  else
    potrf_core<4, 128>(d, A11, nullptr, nullptr, T, scratch, dinvS, tid, b0, nullptr, yb);
  // the row's operands (waves 0-3: 16 rows each), in flight during the forward step (loaded before the
  // factorization they spill: the factorization's registers are live)
  double4_t a[8];
  if (I >= 0 && w < 4) {
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int32_t t = k < 4 ? tI1 : tI2;
      if (t >= 0 && (k < 4 || two)) {
#pragma unroll
        for (int r = 0; r < 4; r++) a[k][r] = d.tiles[(int64_t)t * TS * TS + (16 * (k & 3) + lq + 4 * r) * TS + 16 * w + lr];
      } else {
        a[k] = double4_t{0, 0, 0, 0};
      }
    }
  }
  if (fwdB && writer && w < (two ? 2 : 1)) {
    const int64_t row = (int64_t)(J + w) * TS + lane;
    fwdY[row] = row < d.nRed ? yb[128 + 64 * w + lane] : 0.0;
  }
  if (writer) {
    if (two) store_block_tiles<8, 128>(Lscr + J * TS * TS, Lscr + (nT + J) * TS * TS, Lscr + (J + 1) * TS * TS, T, tid, 512);
    else store_block_tiles<4, 128>(Lscr + J * TS * TS, nullptr, nullptr, T, tid, 512);
    for (int i = tid; i < (two ? 2048 : 1024); i += 512) dinvAll[(int64_t)J * 1024 + i] = dinvS[i];
  }
  if (I < 0) return;
  if (w >= 4) return;
  // (the row's dot with y and its subtraction stay written out here: through lane_dot / fwd_sub the compiler
  // allocates this kernel's registers differently, and it is on the default schedule's path)
  double v = 0.0;
  if (two) {
    double4_t X[8];
    trsm_lds<8, 128>(T, dinvS, a, X, lr, lq);
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const int32_t t = k < 4 ? tI1 : tI2;
      if (t >= 0) {
#pragma unroll
        for (int r = 0; r < 4; r++) d.tiles[(int64_t)t * TS * TS + (16 * (k & 3) + lq + 4 * r) * TS + 16 * w + lr] = X[k][r];
      }
#pragma unroll
      for (int r = 0; r < 4; r++) v += X[k][r] * yb[128 + 16 * k + lq + 4 * r];
    }
  } else {
    double4_t a4[4], X[4];
#pragma unroll
    for (int k = 0; k < 4; k++) a4[k] = a[k];
    trsm_lds<4, 128>(T, dinvS, a4, X, lr, lq);
    store_rows(d.tiles + (int64_t)tI1 * TS * TS, X, w, lr, lq);
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int r = 0; r < 4; r++) v += X[k][r] * yb[128 + 16 * k + lq + 4 * r];
  }
  if (fwdB) {
    v = lanegroup_sum(v);
    if (lq == 0) atomicAdd(fwdB + (int64_t)I * TS + 16 * w + lr, -v);
  }
}

// The rows of a supernode, one block per row I below it (items: tile (I, J) or -1, tile (I, J + 1) or -1,
// J, J + 1 or -1, I, tiles (J, J), (J + 1, J), (J + 1, J + 1)): L_I1 = A_I1 L11^-T, A_I2 -= L_I1 L21^T,
// L_I2 = A_I2 L22^-T; with the fused forward solve b_I -= L_I1 y_J + L_I2 y_{J+1}
__device__ __forceinline__ void sntrsm_body(const Dev& d, const int32_t* items, const double* dinvAll, const double* fwdY,
                                            double* fwdB) {
  // consecutive items (the rows of one supernode) on one XCD: its L11 / L21 / L22 stay in that L2
  const int32_t* it = items + 8 * xcd_block(blockIdx.x, gridDim.x);
  const int32_t tI1 = it[0], tI2 = it[1], J = it[2], J2 = it[3], I = it[4], t11 = it[5], t21 = it[6], t22 = it[7];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  double4_t X1[4], a2[4];
  double v = 0.0;
  if (J2 >= 0) load_rows(d.tiles + (int64_t)tI2 * TS * TS, a2, w, lr, lq);
  if (tI1 >= 0) {
    double* A1 = d.tiles + (int64_t)tI1 * TS * TS;
    double4_t a1[4];
    load_rows(A1, a1, w, lr, lq);
    trsm_rows(d.tiles + (int64_t)t11 * TS * TS, dinvAll + (int64_t)J * 1024, a1, X1, lr, lq);
    store_rows(A1, X1, w, lr, lq);
    if (fwdB) v += rows_dot(X1, fwdY + (int64_t)J * TS, lq);
    if (J2 >= 0) gemm_nt_sub(d.tiles + (int64_t)t21 * TS * TS, X1, a2, lr, lq);
  }
  if (J2 >= 0) {
    double4_t X2[4];
    trsm_rows(d.tiles + (int64_t)t22 * TS * TS, dinvAll + (int64_t)J2 * 1024, a2, X2, lr, lq);
    store_rows(d.tiles + (int64_t)tI2 * TS * TS, X2, w, lr, lq);
    if (fwdB) v += rows_dot(X2, fwdY + (int64_t)J2 * TS, lq);
  }
  if (fwdB && lq == 0) atomicAdd(fwdB + (int64_t)I * TS + 16 * w + lr, -v);  // (rows_dot summed the lane groups)
}
__global__ void __launch_bounds__(256) sntrsm_kernel(Dev d, const int32_t* items, const double* dinvAll, const double* fwdY,
                                                     double* fwdB) {
  sntrsm_body(d, items, dinvAll, fwdY, fwdB);
}
// (a four-waves-per-SIMD build of the same body spilled 10 VGPRs: 52.3 against 52.9 it/s, r05)

// the diagonal tiles of the fused levels back from Lscr (pairs: diagonal tile, column)
__global__ void __launch_bounds__(256) copy_diag_kernel(Dev d, const int32_t* pairs, const double* Lscr) {
  const int32_t t = pairs[2 * blockIdx.x], c = pairs[2 * blockIdx.x + 1];
  lds_to_global(d.tiles + (int64_t)t * TS * TS, Lscr + (int64_t)c * TS * TS, TS * TS, threadIdx.x, 256);
}

// Inverse of every factored diagonal tile (one wave per tile, lane = column c of X = L^-1, off the
// factorization's critical path but before the backward solve): x_i = (delta_ic - sum_{k<i} L_ik x_k) / L_ii
// with the 64 reciprocals formed first (one divide per lane) and each row's sum split over four partial
// sums, so the dependent chain per row is a quarter of its FMAs and a multiply (one running sum and a
// divide per row: ~105 us per factorization at config C).
// linv[J] is column-major; the triangular solves apply it as a GEMV.
__global__ void __launch_bounds__(64) diag_inverse_kernel(Dev d, const int32_t* cols, double* linv) {
  __shared__ double L[TS * TS];
  __shared__ double rd[TS];
  const int J = cols ? cols[blockIdx.x] : (int)blockIdx.x, lane = threadIdx.x;
  const double* Ad = d.tiles + (int64_t)d.tileIdx[(int64_t)J * d.nT + J] * TS * TS;
  {
    double v[TS];  // all loads in flight before the LDS stores
#pragma unroll
    for (int c = 0; c < TS; c++) v[c] = Ad[c * TS + lane];
#pragma unroll
    for (int c = 0; c < TS; c++) L[c * TS + lane] = v[c];
  }
  __syncthreads();
  rd[lane] = 1.0 / L[lane * TS + lane];
  __syncthreads();
  double xi[TS];
#pragma unroll
  for (int i = 0; i < TS; i++) {
    double s0 = (i == lane) ? 1.0 : 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
    for (int k = 0; k + 3 < i; k += 4) {
      s0 -= L[k * TS + i] * xi[k], s1 -= L[(k + 1) * TS + i] * xi[k + 1];
      s2 -= L[(k + 2) * TS + i] * xi[k + 2], s3 -= L[(k + 3) * TS + i] * xi[k + 3];
    }
#pragma unroll
    for (int k = i & ~3; k < i; k++) s0 -= L[k * TS + i] * xi[k];
    xi[i] = ((s0 + s1) + (s2 + s3)) * rd[i];
  }
  double* out = linv + (int64_t)J * TS * TS + lane * TS;
#pragma unroll
  for (int i = 0; i < TS; i++) out[i] = xi[i];
}

// identity on the diagonal of the padding rows (rows of no variable: tile alignment of the
// nested-dissection parts, and the tail of the last tile)
__global__ void pad_diag_kernel(Dev d, const int64_t* rows, int64_t n) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && owns_col(d, rows[i] / TS)) *tile_ptr(d, rows[i], rows[i]) = 1.0;
}

// ------------------------------------------------------------------ launch wrappers
// fwdB / fwdY (may be null): the forward solve fused into the factorization (potrf: y_J from b_J;
// trsm: b_I -= L_IJ y_J for its tile, rows[] = the tile's row I)
void launch_potrf(const Dev& d, const int32_t* tiles, const int32_t* cols, int n, double* dinv, hipStream_t st,
                  const double* fwdB, double* fwdY) {
  if (n > 0) launchK(potrf4_kernel, dim3(n), dim3(256), 0, st, d, tiles, cols, dinv, fwdB, fwdY);
}
void launch_potrf_trsm(const Dev& d, const int32_t* items, int n, double* Lscr, double* dinv, hipStream_t st,
                       double* fwdB, double* fwdY) {
  if (n > 0) launchK(potrf_trsm_kernel, dim3(n), dim3(256), 0, st, d, items, Lscr, dinv, fwdB, fwdY);
}
void launch_trsm(const Dev& d, const int32_t* diag, const int32_t* target, const int32_t* cols, int n, const double* dinv,
                 hipStream_t st, const int32_t* rows, const double* fwdY, double* fwdB) {
  if (n > 0) launchK(trsm_kernel, dim3(n), dim3(256), 0, st, d, diag, target, cols, dinv, rows, fwdY, fwdB);
}
void launch_snpotrf(const Dev& d, const int32_t* items, int n, double* dinv, hipStream_t st, const double* fwdB,
                    double* fwdY) {
  if (n > 0) launchK(snpotrf8_kernel, dim3(n), dim3(512), 0, st, d, items, dinv, fwdB, fwdY);
}
void launch_snpotrf_trsm(const Dev& d, const int32_t* items, int n, double* Lscr, double* dinv, hipStream_t st,
                         double* fwdB, double* fwdY) {
  if (n > 0) launchK(snpotrf_trsm8_kernel, dim3(n), dim3(512), 0, st, d, items, Lscr, dinv, fwdB, fwdY);
}
void launch_sntrsm(const Dev& d, const int32_t* items, int n, const double* dinv, hipStream_t st, const double* fwdY,
                   double* fwdB) {
  if (n > 0) launchK(sntrsm_kernel, dim3(n), dim3(256), 0, st, d, items, dinv, fwdY, fwdB);
}
void launch_copy_diag(const Dev& d, const int32_t* pairs, int n, const double* Lscr, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(copy_diag_kernel, dim3(n), dim3(256), 0, st, d, pairs, Lscr);
}
// inverses of the diagonal factor tiles of the listed columns (all columns if cols == nullptr)
void launch_diag_inverse(const Dev& d, const int32_t* cols, int64_t n, double* linv, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(diag_inverse_kernel, dim3((unsigned)n), dim3(64), 0, st, d, cols, linv);
}
void launch_pad_diag(const Dev& d, const int64_t* rows, int64_t n, hipStream_t st) {
  if (n > 0) hipLaunchKernelGGL(pad_diag_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d, rows, n);
}

}  // namespace viba
