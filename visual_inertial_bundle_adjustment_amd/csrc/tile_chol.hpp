// Device building blocks of the tile Cholesky (gfx950), shared by both schedules' kernels (chol.hip); no
// kernels, no launchers:
//   diag16                 16 x 16 Cholesky + inverse of one diagonal block (rowbcast, rsqrt_nr, Chol16)
//   potrf_core             (16 NB)-wide diagonal block on NB waves, optionally with the forward solve fused
//   potrf_forward          the forward step y_J = L_JJ^-1 b_J as one wave's pass after the factorization
//   trsm_rows, trsm_lds    a wave's 16 rows of A L^-T, L from global / from LDS; gemm_nt_sub: acc -= X M^T
//   load_rows, store_rows, load_cols, rows_dot, fwd_sub   the D-layout row block and its forward update
//   lds_to_global, store_block_tiles                      the factored block back to its tiles
// Inside a tile everything is blocked by 16 and runs on v_mfma_f64_16x16x4_f64, computed TRANSPOSED:
// an accumulator D (lane l, register r) = D[(l >> 4) + 4 r][l & 15] is exactly the B operand of k-step
// r (B[4 r + (l >> 4)][l & 15]), so chained products need no data movement.  The only scalar work is
// the factor + inverse of the four 16 x 16 diagonal blocks (dinv[J]: 4 x 256 doubles, column-major).
#pragma once
#include "kernel_common.hpp"

namespace viba {

// Broadcast lane J of each 16-lane row to the whole row: one v_mov_b64_dpp row_newbcast:J
// (the 16 x 16 diagonal blocks live in lanes 0..15, one row / column per lane)
template <int J>
__device__ __forceinline__ double rowbcast(double v) {
  return __builtin_amdgcn_mov_dpp(v, 0x150 + J, 0xF, 0xF, true);
}

// 1 / sqrt(x): v_rsq_f64 + one third-order refinement (the IEEE sqrt + divide sequences are ~40
// dependent instructions on the factorization's serial chain)
__device__ __forceinline__ double rsqrt_nr(double x) {
  double y = __builtin_amdgcn_rsq(x);
  // one third-order step, e = 1 - x y^2: y (1 + e / 2 + 3 e^2 / 8), four dependent operations where two
  // Newton steps take six (v_rsq_f64 is good to ~2^-23, so the result is within ~1.5 ulp either way)
  const double e = __builtin_fma(-(x * y), y, 1.0);
  return __builtin_fma(e * y, __builtin_fma(e, 0.375, 0.5), y);
}

// 16 x 16 Cholesky, lane r holds row r in s[0..16) (lanes >= 16 compute garbage, ignored):
// right-looking; step C broadcasts the pivot and the scaled column by DPP.
template <int C, int J>
struct Upd16 {
  static __device__ __forceinline__ void run(double (&s)[16], double lc) {
    s[J] -= lc * rowbcast<J>(lc);
    Upd16<C, J + 1>::run(s, lc);
  }
};
template <int C>
struct Upd16<C, 16> {
  static __device__ __forceinline__ void run(double (&)[16], double) {}
};
// Step C: pivot, column C of L, rank-1 update of the trailing columns (right-looking); invd[C] =
// 1 / L_CC (the same value in every lane).  Only the pivot chain is serial here; the inverse is
// formed afterwards (diag16), off this chain.
template <int C>
struct Chol16 {
  static __device__ __forceinline__ void run(double (&s)[16], double (&invd)[16], int lane, bool& bad) {
    const double piv = rowbcast<C>(s[C]);
    bad |= !(piv > 0.0);
    const double y = rsqrt_nr(piv);
    invd[C] = y;
    const double lc = s[C] * y;  // lane C holds the pivot itself: L_CC = piv * y
    s[C] = lc;
    Upd16<C, C + 1>::run(s, lc);
    Chol16<C + 1>::run(s, invd, lane, bad);
  }
};
template <>
struct Chol16<16> {
  static __device__ __forceinline__ void run(double (&)[16], double (&)[16], int, bool&) {}
};

// Factor + invert the 16 x 16 diagonal block i of T (LDS) given S (its updated value, D layout; only
// its lower triangle is valid): writes L_ii into T and Dinv_i into dinvS (LDS).  Cholesky first, lane
// r holding row r (pivot chain only: DPP row broadcasts, v_rsq_f64 + Newton), then X = L^-1 with
// lane c computing column c right-looking: once x_k is known every later row's accumulator takes its
// term, so the serial chain is one FMA + one multiply per row (L from LDS by broadcast reads).
// (A one-MFMA-per-pivot variant -- the rank-1 update as a v_mfma_f64_16x16x4_f64 on the D layout --
// measured slower: each pivot then waits on a dependent MFMA + readlane, 7.9k vs 5.7k cycles.)
template <int LDT = TS>
__device__ __forceinline__ void diag16(double* T, double* scratch, double* dinvS, int i, double4_t S, int lane,
                                       bool& bad) {
  const int lr = lane & 15, lq = lane >> 4;
#pragma unroll
  for (int r = 0; r < 4; r++) scratch[(lq + 4 * r) * 16 + lr] = S[r];  // row-major S[i'][j']
  __builtin_amdgcn_wave_barrier();
  double s[16], invd[16];
#pragma unroll
  for (int c = 0; c < 16; c++) s[c] = scratch[lr * 16 + c];
  Chol16<0>::run(s, invd, lane, bad);
  __builtin_amdgcn_wave_barrier();  // every lane has read S
  if (lane < 16) {  // L_ii into the scratch (for X below) and into T; s dies here
#pragma unroll
    for (int c = 0; c < 16; c++) {
      const double v = (c <= lane) ? s[c] : 0.0;
      scratch[lane * 16 + c] = v;
      T[(16 * i + c) * LDT + 16 * i + lane] = v;
    }
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  double acc[16];  // becomes column lr of X = L_ii^-1 in place (x_k = acc_k / L_kk)
#pragma unroll
  for (int r = 0; r < 16; r++) acc[r] = (r == lr) ? 1.0 : 0.0;
#pragma unroll
  for (int k = 0; k < 16; k++) {
    acc[k] *= invd[k];
#pragma unroll
    for (int r = k + 1; r < 16; r++) acc[r] -= scratch[r * 16 + k] * acc[k];
  }
  if (lane < 16) {
#pragma unroll
    for (int r = 0; r < 16; r++) dinvS[i * 256 + lane * 16 + r] = acc[r];  // rows above the lane stay +0.0
  }
  __builtin_amdgcn_wave_barrier();
}

// copy n doubles LDS -> global with `nthreads` threads (pointer-stepped, bounded unroll: keeps the
// compiler from materialising every address up front)
__device__ __forceinline__ void lds_to_global(double* dst, const double* src, int n, int tid, int nthreads) {
  double* p = dst + tid;
  const double* q = src + tid;
#pragma unroll 8
  for (int i = tid; i < n; i += nthreads, p += nthreads, q += nthreads) *p = *q;
}

__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// forward step of the column's solve after its factorization (one wave; T, dinvS: the factored 64 x 64
// tile and its 16 x 16 block inverses in LDS): y_J = L_JJ^-1 b_J, b_J complete since every L_JK y_K
// update landed in an earlier level's launch
__device__ __forceinline__ void potrf_forward(const Dev& d, const double* T, const double* dinvS, double* sh, int J,
                                              const double* bJ, double* y, int lane, bool store = true) {
  // right-looking by 16-row blocks: lane r keeps b_r; once y_i is known every later row subtracts
  // L(r, block i) y_i, so each block's chain is one 16-term GEMV + one 16-term update (bJ: b_J's 64 rows)
  double br = bJ[lane];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    sh[64 + lane] = br;
    wave_sync_lds();
    if ((lane >> 4) == i) {
      const int l = lane & 15;
      double v = 0.0;
#pragma unroll
      for (int m = 0; m < 16; m++) v += dinvS[i * 256 + m * 16 + l] * sh[64 + 16 * i + m];
      sh[16 * i + l] = v;
    }
    wave_sync_lds();
    if (i < 3) {
#pragma unroll
      for (int m = 0; m < 16; m++) br -= T[(16 * i + m) * TS + lane] * sh[16 * i + m];
    }
  }
  const int64_t row = (int64_t)J * TS + lane;
  if (store) y[row] = row < d.nRed ? sh[lane] : 0.0;  // y_J also stays in sh[0, 64)
}

// X = A L^-T for one tile row block per wave: acc holds A (D layout: lane (lr, lq), register r = element
// (row 16 w + lr, column 16 k + lq + 4 r)); L the factored diagonal tile, dinv its 16 x 16 block inverses.
// Every operand (24 of L, 16 of the inverses, all independent) is loaded before the substitution chain,
// which then runs on registers instead of waiting on a global load per k-step.
template <int LD = TS>
__device__ __forceinline__ void trsm_rows(const double* L, const double* dinv, double4_t (&acc)[4], double4_t (&Xt)[4],
                                          int lr, int lq) {
  double lv[6][4], dv[4][4];
#pragma unroll
  for (int k = 1; k < 4; k++)
#pragma unroll
    for (int k2 = 0; k2 < k; k2++)
#pragma unroll
      for (int s = 0; s < 4; s++) lv[k * (k - 1) / 2 + k2][s] = L[(16 * k2 + 4 * s + lq) * LD + 16 * k + lr];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int s = 0; s < 4; s++) dv[k][s] = dinv[k * 256 + (4 * s + lq) * 16 + lr];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double4_t a = acc[k];
#pragma unroll
    for (int k2 = 0; k2 < k; k2++)
#pragma unroll
      for (int s = 0; s < 4; s++) a = mfma64(-lv[k * (k - 1) / 2 + k2][s], Xt[k2][s], a);
    double4_t res = double4_t{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; s++) res = mfma64(dv[k][s], a[s], res);
    Xt[k] = res;
  }
}
// acc -= X M^T over all four column blocks of M (a full tile: the update of a supernode's second column by
// its first), X in D layout, M column-major in memory (global or LDS)
template <int LD = TS>
__device__ __forceinline__ void gemm_nt_sub(const double* M, const double4_t (&Xt)[4], double4_t (&acc)[4], int lr, int lq,
                                            int kmax = 3) {
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (k > kmax) break;
    double mv[4][4];
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
      for (int s = 0; s < 4; s++) mv[k2][s] = M[(16 * k2 + 4 * s + lq) * LD + 16 * k + lr];
#pragma unroll
    for (int k2 = 0; k2 < 4; k2++)
#pragma unroll
      for (int s = 0; s < 4; s++) acc[k] = mfma64(-mv[k2][s], Xt[k2][s], acc[k]);
  }
}
__device__ __forceinline__ void load_rows(const double* A, double4_t (&acc)[4], int w, int lr, int lq) {
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int r = 0; r < 4; r++) acc[k][r] = A[(16 * k + lq + 4 * r) * TS + 16 * w + lr];
}
__device__ __forceinline__ void store_rows(double* A, const double4_t (&X)[4], int w, int lr, int lq) {
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int r = 0; r < 4; r++) A[(16 * k + lq + 4 * r) * TS + 16 * w + lr] = X[k][r];
}
// a lane's value summed over the four lane groups lq (every lane gets the sum of its lr)
__device__ __forceinline__ double lanegroup_sum(double v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}
// the entries of y (16 NB values, LDS / global) at this lane's columns: 16 k + lq + 4 r per register
template <int NB>
__device__ __forceinline__ void load_cols(const double* y, double4_t (&yv)[NB], int lq) {
#pragma unroll
  for (int k = 0; k < NB; k++)
#pragma unroll
    for (int r = 0; r < 4; r++) yv[k][r] = y[16 * k + lq + 4 * r];
}
// this lane's part of the wave's rows of X y (row 16 w + lr over the lane's columns)
template <int NB>
__device__ __forceinline__ double lane_dot(const double4_t (&X)[NB], const double4_t (&yv)[NB]) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < NB; k++)
#pragma unroll
    for (int r = 0; r < 4; r++) v += X[k][r] * yv[k][r];
  return v;
}
template <int NB>
__device__ __forceinline__ double lane_dot(const double4_t (&X)[NB], const double* y, int lq) {
  double v = 0.0;
#pragma unroll
  for (int k = 0; k < NB; k++)
#pragma unroll
    for (int r = 0; r < 4; r++) v += X[k][r] * y[16 * k + lq + 4 * r];
  return v;
}
// this wave's rows of X y, summed over the lane groups: lanes lq == 0 hold row 16 w + lr
__device__ __forceinline__ double rows_dot(const double4_t (&X)[4], const double* y, int lq) {
  return lanegroup_sum(lane_dot(X, y, lq));
}
// the fused forward solve's update of row block I (bI: its 64 rows of b) by this wave's rows: b_I -= the
// lanes' parts v (lane_dot) summed over the lane groups
__device__ __forceinline__ void fwd_sub(double* bI, double v, int w, int lr, int lq) {
  v = lanegroup_sum(v);
  if (lq == 0) atomicAdd(bI + 16 * w + lr, -v);
}

// A (16 NB)-wide diagonal block held as up to three tiles (A11; for NB = 8 also A21 = tile (J + 1, J),
// A22 = tile (J + 1, J + 1)), right-looking over the 16-column blocks k: NB waves, wave w keeps its 16-row
// block of the lower triangle (A_wj^T for j <= w, D layout) in registers; L goes to LDS T (stride LDT), the
// 16 x 16 block inverses to dinvS (NB x 256); the upper blocks are written as zeros.  Waves >= NB only pass
// the barriers.  Wave k factors + inverts its diagonal block (diag16); every wave below then forms L_wk =
// A_wk Dinv_k^T (4 MFMAs), publishes it in LDS and takes its own diagonal update L_wk L_wk^T from registers,
// and after a barrier updates its blocks k < j < w with L_jk -- while wave k + 1 is already in diag16.
// Between two diag16 the chain is 8 dependent MFMAs (a one-wave left-looking form chains up to 36 of them);
// the terms are subtracted in the same order as there.
// With b0 (the fused forward solve; b1: the second column's 64 rows) the forward substitution runs inside
// the block loop: wave k forms y_k = Dinv_k b_k right after its diag16, and every wave below subtracts
// L_wk y_k from its rows with the L_wk it just formed -- no serial pass after the factorization.  y goes to
// yb[128, 128 + 16 NB) (yb[0, 16 NB): staging of b).
template <int NB, int LDT>
__device__ __forceinline__ void potrf_core(const Dev& d, const double* A11, const double* A21, const double* A22,
                                           double* T, double* scratch, double* dinvS, int tid,
                                           const double* b0 = nullptr, const double* b1 = nullptr,
                                           double* yb = nullptr) {
  const int lane = tid & 63, w = tid >> 6;
  const int lr = lane & 15, lq = lane >> 4;
  double bw = 0.0;  // b of this wave's 16 rows (lane: row 16 w + lr)
  if (b0 && w < NB) bw = (w < 4 ? b0 : b1)[16 * (w & 3) + lr];
  double4_t R[NB];
  if (w < NB) {
#pragma unroll
    for (int j = 0; j < NB; j++) {
      const double* P = w < 4 ? A11 : (j < 4 ? A21 : A22);
      const int rr = 16 * (w & 3), cc = 16 * (j & 3);
      if (j < w) {
#pragma unroll
        for (int r = 0; r < 4; r++) R[j][r] = P[(cc + lq + 4 * r) * TS + rr + lr];
      } else if (j == w) {
#pragma unroll
        for (int r = 0; r < 4; r++) R[j][r] = P[(cc + lr) * TS + rr + lq + 4 * r];  // lower part valid
      } else {
#pragma unroll
        for (int r = 0; r < 4; r++) T[(16 * j + lq + 4 * r) * LDT + 16 * w + lr] = 0.0;
      }
    }
  }
  bool bad = false;
#pragma unroll
  for (int k = 0; k < NB; k++) {
    if (w == k) {
      diag16<LDT>(T, scratch, dinvS, k, R[k], lane, bad);
      if (b0) {  // y_k = Dinv_k b_k (this wave's rows are final)
        if (lq == 0) yb[16 * k + lr] = bw;
        wave_sync_lds();
        if (lq == 0) {
          double v = 0.0;
#pragma unroll
          for (int m = 0; m < 16; m++) v += dinvS[k * 256 + m * 16 + lr] * yb[16 * k + m];
          yb[128 + 16 * k + lr] = v;
        }
      }
    }
    __syncthreads();
    double4_t Lt = double4_t{0, 0, 0, 0};
    if (w > k && w < NB) {
#pragma unroll
      for (int s = 0; s < 4; s++) Lt = mfma64(dinvS[k * 256 + (4 * s + lq) * 16 + lr], R[k][s], Lt);
#pragma unroll
      for (int r = 0; r < 4; r++) T[(16 * k + lq + 4 * r) * LDT + 16 * w + lr] = Lt[r];
      if (b0) {  // b_w -= L_wk y_k (lane (lr, lq) holds L(16 w + lr, 16 k + lq + 4 r))
        double v = 0.0;
#pragma unroll
        for (int r = 0; r < 4; r++) v += Lt[r] * yb[128 + 16 * k + lq + 4 * r];
        bw -= lanegroup_sum(v);
      }
#pragma unroll
      for (int j = k + 1; j < NB; j++)
        if (j == w) {
#pragma unroll
          for (int s = 0; s < 4; s++) R[j] = mfma64(-Lt[s], Lt[s], R[j]);
        }
    }
    if (k < NB - 2) {
      __syncthreads();
#pragma unroll
      for (int j = k + 1; j < NB - 1; j++)
        if (j < w && w < NB) {
#pragma unroll
          for (int s = 0; s < 4; s++) R[j] = mfma64(-T[(16 * k + 4 * s + lq) * LDT + 16 * j + lr], Lt[s], R[j]);
        }
    }
  }
  __syncthreads();
  if (bad && lane == 0) atomicOr(d.err, 8);
}

// this wave's 16 rows of [A_I1 A_I2] L^-T over the (16 NB)-wide factored block in LDS (T, dinvS):
// a[k] = column block k of A (D layout) in, X[k] out
template <int NB, int LDT>
__device__ __forceinline__ void trsm_lds(const double* T, const double* dinvS, const double4_t (&a)[NB], double4_t (&X)[NB],
                                         int lr, int lq) {
#pragma unroll
  for (int k = 0; k < NB; k++) {
    double4_t acc = a[k];
#pragma unroll
    for (int k2 = 0; k2 < k; k2++)
#pragma unroll
      for (int s = 0; s < 4; s++) acc = mfma64(-T[(16 * k2 + 4 * s + lq) * LDT + 16 * k + lr], X[k2][s], acc);
    double4_t res = double4_t{0, 0, 0, 0};
#pragma unroll
    for (int s = 0; s < 4; s++) res = mfma64(dinvS[k * 256 + (4 * s + lq) * 16 + lr], acc[s], res);
    X[k] = res;
  }
}

// block (bi, bj) (16 x 16) of the factored diagonal block in LDS -> its global tile (the 64 x 64 tiles
// of a pair: (J, J) blocks < 4, (J + 1, J) rows >= 4, (J + 1, J + 1) both >= 4)
template <int NB, int LDT>
__device__ __forceinline__ void store_block_tiles(double* L11, double* L21, double* L22, const double* T, int tid,
                                                  int nthreads) {
  for (int i = tid; i < (16 * NB) * (16 * NB); i += nthreads) {
    const int col = i / (16 * NB), row = i % (16 * NB);
    if (row < 64 && col >= 64) continue;  // upper block (none stored)
    double* P = row < 64 ? L11 : (col < 64 ? L21 : L22);
    P[(col & 63) * TS + (row & 63)] = T[col * LDT + row];
  }
}

}  // namespace viba
