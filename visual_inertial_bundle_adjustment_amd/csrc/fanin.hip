// Fan-in of the level-scheduled tile Cholesky (gfx950):
//   fanin_kernel          A_IJ -= sum_K L_IK L_JK^T for a level's target tiles (v_mfma_f64_16x16x4), operands
//                         through a ring of LDS stages filled by global_load_lds
#include "kernel_common.hpp"

namespace viba {

// Fan-in (left-looking) update of target tile (I, J): A_IJ -= sum_K L_IK L_JK^T over one chunk of the
// target's contribution list, computed at the level of column J (right before its potrf / trsm), so
// the target is read and written once per chunk instead of once per contribution.
// work[4 b .. 4 b + 4) = (target tile, first contribution, count, atomic); pairs[2 c] = L_IK tile,
// pairs[2 c + 1] = L_JK tile; `atomic`: the target's list is split over several chunks.
//
// The four waves share every contribution: wave w owns the 32 x 32 block (p in [32 (w >> 1), +32),
// q in [32 (w & 1), +32)) of the product, computed transposed (D = L_JK L_IK^T, so the MFMA output
// column lane & 15 runs along the tile's contiguous row index).  Operands are staged per quarter
// contribution (K = 16 columns of both tiles, 16 KB) by async global_load_lds (16 B per lane) into a
// three-deep LDS ring (48 KB: three workgroups per CU): stage s + 1 is in flight while stage s feeds
// v_mfma_f64_16x16x4_f64 and the CU's other workgroups cover the rest of the HBM latency (measured on
// config C: K 16 x 3 buffers 41.6 TF/s, 16 x 4 40.2, 8 x 4 38.3, 32 x 3 35.0, 8 x 8 32.0 -- the
// workgroups per CU matter more than the depth of one ring).  Writing stage s + R - 2 into buffer
// (s + R - 2) % R is safe after one barrier per stage: its last reader was stage s - 2.  Odd columns
// are stored rotated by 16 rows so each half-wave of a ds_read_b64 (two columns) hits all 64 banks.
constexpr int kFanK = 16;                  // columns per stage
constexpr int kFanRing = 3;                // stages in the LDS ring (kFanRing - 1 in flight)
constexpr int kStage = 2 * kFanK * TS;     // doubles per stage: [L_JK, L_IK][kFanK columns][64 rows]
constexpr int kFanWaves = 4;               // waves per fan-in workgroup
constexpr int kGlds = kStage / 128 / kFanWaves;  // global_load_lds per wave per stage (1 KB = 128 doubles each)
// LDS row rotation of stage column t (rows stored at (row + rot) & 63): odd columns by 16, so a half-wave
// reading two columns of one row range hits all 64 banks
__device__ __forceinline__ int fan_rot(int t) { return 16 * (t & 1); }

__device__ __forceinline__ void fanin_issue(const Dev& d, const int32_t* pairs, int32_t start, int s, double* buf,
                                            int wave, int lane) {
  const int64_t c = start + s / (TS / kFanK);
  const int k0 = (s % (TS / kFanK)) * kFanK;
  // constant address space: scalar loads (lgkmcnt), so no vmcnt wait drains the LDS ring
  const __attribute__((address_space(4))) int32_t* pc = (const __attribute__((address_space(4))) int32_t*)pairs;
  const int64_t tk = pc[2 * c + 1], ti = pc[2 * c];
  const int hi = lane >> 5;
#pragma unroll
  for (int j = 0; j < kGlds; j++) {
    const int i = wave * kGlds + j, tile = i / (kFanK / 2), cp = i % (kFanK / 2);  // 1 KB = 2 columns each
    const int row = (2 * (lane & 31) - fan_rot(2 * cp + hi)) & 63;
    const double* src = d.tiles + (tile ? ti : tk) * TS * TS + (int64_t)(k0 + 2 * cp + hi) * TS + row;
    glds<16>(src, buf + tile * kFanK * TS + cp * 2 * TS);
  }
}

// Fan-in accumulation of contributions [start, start + count) of one target: acc = sum L_IK L_JK^T over
// the wave's 32 x 32 quadrant (ring in `stg`; every wave passes a barrier per stage, so all waves call it).
// Issue-after-barrier: kFanRing - 1 stages in flight; stage s + R - 1 goes into the buffer of stage
// s - 1, whose readers all passed this iteration's barrier.
__device__ __forceinline__ void fanin_accum(const Dev& d, const int32_t* pairs, int32_t start, int32_t count,
                                            double* stg, int wave, int lane, double4_t (&acc)[2][2]) {
  static_assert(kGlds * (kFanRing - 1) <= 63, "vmcnt range");
  const int l15 = lane & 15, l4 = lane >> 4;
  const int pb = (wave >> 1) * 32, qb = (wave & 1) * 32;
  const int32_t nst = (TS / kFanK) * count;
#pragma unroll
  for (int a = 0; a < 2; a++)
#pragma unroll
    for (int b = 0; b < 2; b++) acc[a][b] = double4_t{0, 0, 0, 0};
  constexpr int kAhead = kFanRing - 1;
  for (int s = 0; s < kAhead && s < nst; s++) fanin_issue(d, pairs, start, s, stg + s * kStage, wave, lane);
  for (int s = 0; s < nst; s++) {
    // this wave's part of stage s landed (later stages may stay in flight)
    if (s + 1 < nst) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kGlds) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // ... and every other wave's
    __builtin_amdgcn_sched_barrier(0);
    if (s + kAhead < nst) fanin_issue(d, pairs, start, s + kAhead, stg + ((s + kAhead) % kFanRing) * kStage, wave, lane);
    __builtin_amdgcn_sched_barrier(0);
    const double* bk = stg + (s % kFanRing) * kStage;
    const double* bi = bk + kFanK * TS;
#pragma unroll
    for (int t0 = 0; t0 < kFanK; t0 += 4) {
      const int t = t0 + l4, rot = (t & 1) * 16;
      double av[2], bv[2];
#pragma unroll
      for (int a = 0; a < 2; a++) av[a] = bk[t * TS + ((pb + a * 16 + l15 + rot) & 63)];
#pragma unroll
      for (int b = 0; b < 2; b++) bv[b] = bi[t * TS + ((qb + b * 16 + l15 + rot) & 63)];
#pragma unroll
      for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++) acc[a][b] = mfma64(av[a], bv[b], acc[a][b]);
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// C -= acc (the wave's quadrant): agent-scope fp64 atomics when the target's list is split over
// several workgroups, else a read-modify-write with all 16 loads in flight before the stores
__device__ __forceinline__ void fanin_store(double* C, bool atomic, int wave, int lane, const double4_t (&acc)[2][2]) {
  const int l15 = lane & 15, l4 = lane >> 4;
  const int pb = (wave >> 1) * 32, qb = (wave & 1) * 32;
  double* Cw = C + (pb + l4) * TS + qb + l15;
  if (atomic) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) atomicAdd(Cw + (a * 16 + 4 * r) * TS + b * 16, -acc[a][b][r]);
  } else {
    double v[2][2][4];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) v[a][b][r] = Cw[(a * 16 + 4 * r) * TS + b * 16];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
      for (int b = 0; b < 2; b++)
#pragma unroll
        for (int r = 0; r < 4; r++) Cw[(a * 16 + 4 * r) * TS + b * 16] = v[a][b][r] - acc[a][b][r];
  }
}

__global__ void __launch_bounds__(kFanWaves * 64) fanin_kernel(Dev d, const int32_t* work, const int32_t* pairs) {
  __shared__ double stg[kFanRing * kStage];
  const int32_t* wk = work + 4 * xcd_block(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double4_t acc[2][2];
  fanin_accum(d, pairs, wk[1], wk[2], stg, wave, lane, acc);
  fanin_store(d.tiles + (int64_t)wk[0] * TS * TS, wk[3] != 0, wave, lane, acc);
}

void launch_fanin(const Dev& d, const int32_t* work, const int32_t* pairs, int n, hipStream_t st) {
  if (n > 0) launchK(fanin_kernel, dim3(n), dim3(kFanWaves * 64), 0, st, d, work, pairs);
}

}  // namespace viba
