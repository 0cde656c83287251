// Direct visual terms of the reduced system by observation group, gfx950:
//   obs_group_kernel      J~^T J~ and J~^T e~ per (rig, camera) group on fp64 MFMA, records staged through LDS
#include "kernel_common.hpp"

namespace viba {

// Direct visual terms by observation group (observations sharing their reduced blocks: one rig, one
// camera).  Per group: H = sum_o J~_o^T J~_o over the 32 columns [pose 6 | extr 6 | intr <= 17 |
// vel 3] and g = sum_o J~_o^T e~_o, on v_mfma_f64_16x16x4_f64 (K = the group's residual rows, 4 per
// k-step = 2 observations; the 4 waves split K and reduce through LDS).  Lane l owns the columns
// l & 15 and 16 + (l & 15); an accumulator D[m][n] (lane: n = l & 15, rows m = (l >> 4) + 4 r) is the
// Gram block directly.  mode 0: H (diagonal damped by (1 + lambda)) into the tiles, g into gRed;
// mode 1: g only into gRedNew (gradient pass of the bad-step path).
constexpr int kGrpBase[4] = {0, 6, 12, 29};

__device__ __forceinline__ int grp_col_row(const Dev& d, const int32_t* red, int c, int& plane, int& stride) {
  const int s = c < 6 ? 0 : c < 12 ? 1 : c < 29 ? 2 : 3;
  const int j = c - kGrpBase[s];
  const int32_t X = red[s];
  plane = slotPlane(s) + j, stride = slotStride(s);
  if (X < 0 || j >= d.rvDim[X]) return -1;
  return (int)(d.rvOff[X] + j);
}

// the end of a group: the 4 waves' accumulators reduced through LDS (`red`: 4 x 64 x 14 doubles, free on
// entry), g into gRed / gRedNew (mode 1), H (diagonal damped by (1 + lambda)) scattered into the tiles
__device__ __forceinline__ void group_finish(const Dev& d, double lambda, int mode, int row0, int row1, const hacc4_t& a00,
                                             const hacc4_t& a10, const hacc4_t& a11, double g0, double g1, double* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l15 = lane & 15, l4 = lane >> 4;
  // reduce the 4 waves (and, for g, the 4 lane groups) through LDS
  double* mine = red + (wave * 64 + lane) * 14;
#pragma unroll
  for (int k = 0; k < 4; k++) mine[k] = a00[k], mine[4 + k] = a10[k], mine[8 + k] = a11[k];
  mine[12] = g0, mine[13] = g1;
  __syncthreads();
  if (wave != 0) return;
  double t[14];
#pragma unroll
  for (int k = 0; k < 14; k++) t[k] = red[lane * 14 + k] + red[(64 + lane) * 14 + k] + red[(128 + lane) * 14 + k] + red[(192 + lane) * 14 + k];
  // g: lanes l15 of the 4 lane groups hold partial sums of the same columns
  double gc0 = t[12], gc1 = t[13];
#pragma unroll
  for (int off = 16; off < 64; off += 16) {
    gc0 += __shfl(t[12], (lane + off) & 63, 64);
    gc1 += __shfl(t[13], (lane + off) & 63, 64);
  }
  double* gOut = mode == 0 ? d.gRed : d.gRedNew;
  if (l4 == 0) {
    if (row0 >= 0 && gc0 != 0.0) atomicAdd(gOut + row0, gc0);
    if (row1 >= 0 && gc1 != 0.0) atomicAdd(gOut + row1, gc1);
  }
  if (mode != 0) return;
  // H (32 x 32, symmetric) into LDS over the reduction buffer (this wave has read it): D[m][n],
  // m = kAccL4 l4 + kAccR k (+16), n = l15 (+16); the cross block also mirrored
  double* H = red;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int m = kAccL4 * l4 + kAccR * k;
    H[m * 32 + l15] = t[k];
    H[(16 + m) * 32 + 16 + l15] = t[8 + k];
    H[(16 + m) * 32 + l15] = t[4 + k], H[l15 * 32 + 16 + m] = t[4 + k];
  }
  // the valid columns ordered by reduced row (lane c < 32: column c), their distinct tile rows
  int32_t* ord = reinterpret_cast<int32_t*>(H + 32 * 32);  // [32] column at sorted position
  int32_t* crow = ord + 32;                                // [32] column's reduced row
  int32_t* cu = crow + 32;                                 // [32] column's tile-row slot
  int32_t* trow = cu + 32;                                 // [8] distinct tile rows
  int32_t* tpair = trow + 8;                               // [64] tileIdx of (tile row u, v)
  const int rowc = lane < 32 ? (lane < 16 ? row0 : row1) : -1;  // lane c < 32: column c
  const bool val = rowc >= 0;
  int rank = 0;
  for (int c = 0; c < 32; c++) {
    const int rc = __builtin_amdgcn_readlane(rowc, c);
    if (rc >= 0 && rc < rowc) rank++;
  }
  const int nc = __popcll(__ballot(val));
  if (val) ord[rank] = lane;
  const int tr = rowc / TS;
  uint64_t left = __ballot(val);
  int nu = 0, u = -1;
  while (left) {
    const int tl = __builtin_amdgcn_readlane(tr, __builtin_ctzll(left));
    const bool hit = val && tr == tl;
    left &= ~__ballot(hit);
    if (hit) u = nu;
    if (lane == 0) trow[nu] = tl;
    nu++;  // <= 8: four variables, a tile row boundary inside each at most
  }
  if (lane < 32) crow[lane] = rowc, cu[lane] = u;
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  for (int q = lane; q < nu * nu; q += 64) {
    const int tu = trow[q / nu], tv = trow[q % nu];
    tpair[q] = tu >= tv ? d.tileIdx[(int64_t)tu * d.nT + tv] : -1;
  }
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  // lower-triangle entries column by column over the ordered columns (consecutive lanes on consecutive
  // rows of one tile column); diagonal damped by (1 + lambda)
  const int P = nc * (nc + 1) / 2;
  for (int p = lane; p < P; p += 64) {
    const int q = P - 1 - p;
    int i = (int)((sqrtf(8.0f * q + 1.0f) - 1.0f) * 0.5f);
    while (i * (i + 1) / 2 > q) i--;
    while ((i + 1) * (i + 2) / 2 <= q) i++;
    const int b = nc - 1 - i, a = nc - 1 - (q - i * (i + 1) / 2);
    const int ca = ord[a], cb = ord[b];
    double v = H[ca * 32 + cb];
    if (v == 0.0) continue;
    const int R = crow[ca], C = crow[cb];
    if (a == b) v *= 1.0 + lambda;
    const int32_t ti = tpair[cu[ca] * nu + cu[cb]];
    if (ti >= 0) atomicAdd(d.tiles + (int64_t)ti * TS * TS + (C % TS) * TS + (R % TS), v);
    else atomicOr(d.err, 4);
  }
}

// The group's records are streamed through LDS in chunks of kGrpChunk observations, each record copied
// whole (both regions, 16 B per lane by global_load_lds: a handful of wide loads per thread per chunk,
// where gathering the three operands of every k-step straight from HBM, behind an index load, ran
// 1.05 ms against 0.79 alone on config C), double-buffered (chunk k + 1 in flight while chunk k feeds the
// MFMAs).  Staged record c holds plane p at stage[c * kGrpPlanes + p] (p < 2) / [.. + p - kGrpShift] (p >= 8).  The group's observation indices
// come into LDS first, by windows of kGrpIdx.
// observations per staged chunk: swept at config C (r05u, the kernel alone): fp64 16 / 24 / 32 / 48 / 64 ->
// 818 / 794 / 862 / 1045 / 1041 us (LDS per workgroup sets the occupancy); fp32 records 609 / 564 / 550 /
// 543 / 632 us
// Round 6 (r06ad): the point Jacobian's pieces (planes 2..7, never read here) are not staged, and the chunk
// takes as many records as the same loads and buffer hold: fp64 31 records of 33 pieces in 4 loads per thread
// (4 * 256 / 33 = 31; 24 records of 36 pieces before), fp32 records 45 records of 17 pieces in 3 loads
// (3 * 256 / 17 = 45; 32 records of 18 pieces before).
constexpr int kRecPieces = kJPlanes / kRecV;                       // 16 B pieces per record (36 / 18)
constexpr int kGrpSkip = 8 / kRecV - 1;                            // pieces after the first holding planes < 8 only
constexpr int kGrpPieces = kRecPieces - kGrpSkip;                  // staged pieces per record (33 / 17)
constexpr int kGrpPlanes = kGrpPieces * kRecV;                     // staged planes per record
constexpr int kGrpShift = kGrpSkip * kRecV;                        // record plane p >= 8 is staged plane p - kGrpShift
constexpr int kGrpLoads = VIBA_MIXED ? 3 : 4;                      // global_load_lds per thread per chunk
constexpr int kGrpChunk = kGrpLoads * 256 / kGrpPieces;            // records per chunk (fp64 4 * 256 / 33 = 31, fp32 records 3 * 256 / 17 = 45)
constexpr int kGrpStage = kGrpLoads * 256 * kRecV;                 // rec_t per buffer (tail pieces land past the chunk)
constexpr int kGrpIdx = 1024;                                      // observation indices per window
static_assert(kJA % kRecV == 0 && kJB % kRecV == 0, "record regions in whole 16 B pieces");
constexpr int kGrpLds = 2 * kGrpStage * (int)sizeof(rec_t) > 4 * 64 * 14 * 8 ? 2 * kGrpStage * (int)sizeof(rec_t) : 4 * 64 * 14 * 8;

// three LDS reads behind one wait, in inline asm: as plain loads the compiler put an s_waitcnt vmcnt(0)
// before each (it cannot tell them from the global_load_lds stores in flight into the other buffer),
// which drained the next chunk's loads before this chunk's products
__device__ __forceinline__ void lds_read3(const double* a, const double* b, const double* c, double& x, double& y, double& z) {
  asm volatile("ds_read_b64 %0, %3\n\tds_read_b64 %1, %4\n\tds_read_b64 %2, %5\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(x), "=&v"(y), "=&v"(z)
               : "v"(lds_addr(a)), "v"(lds_addr(b)), "v"(lds_addr(c))
               : "memory");
}
__device__ __forceinline__ void lds_read3(const float* a, const float* b, const float* c, float& x, float& y, float& z) {
  asm volatile("ds_read_b32 %0, %3\n\tds_read_b32 %1, %4\n\tds_read_b32 %2, %5\n\ts_waitcnt lgkmcnt(0)"
               : "=&v"(x), "=&v"(y), "=&v"(z)
               : "v"(lds_addr(a)), "v"(lds_addr(b)), "v"(lds_addr(c))
               : "memory");
}

__device__ __forceinline__ void group_issue(const Dev& d, const int32_t* sIdx, int nv, rec_t* buf, int wave, int lane) {
#pragma unroll
  for (int j = 0; j < kGrpLoads; j++) {
    const int i = j * 256 + wave * 64 + lane;
    int c = i / kGrpPieces;
    const int qs = i - c * kGrpPieces;
    const int q = qs == 0 ? 0 : qs + kGrpSkip;  // the record's piece (the point Jacobian's are skipped)
    if (c >= nv) c = 0;  // past the chunk's observations: a valid record again, never read
    const int64_t o = sIdx[c];
    const rec_t* src = q < kJA / kRecV ? d.Jt + o * kJA + q * kRecV
                                        : d.Jt + d.nObsPad * kJA + o * kJB + (q - kJA / kRecV) * kRecV;
    glds<16>(src, buf + (j * 256 + wave * 64) * kRecV);
  }
}

__global__ void __launch_bounds__(256) obs_group_kernel(Dev d, double lambda, int mode) {
  __shared__ __attribute__((aligned(16))) double smem[kGrpLds / 8];  // the two buffers, then the epilogue's
  __shared__ int32_t sIdx[kGrpIdx];
  rec_t* stg = reinterpret_cast<rec_t*>(smem);
  const int64_t g = xcd_block(blockIdx.x, gridDim.x);
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int32_t* rv = d.grpRed + 4 * g;
  int p0, s0, p1, s1;
  const int row0 = grp_col_row(d, rv, l15, p0, s0);
  const int row1 = grp_col_row(d, rv, 16 + l15, p1, s1);
  const int64_t o0 = d.grpStart[g], n = d.grpStart[g + 1] - o0;
  const int r = l4 & 1;
  // this lane's staged planes (K row parity r)
  const int q0 = row0 >= 0 ? p0 + r * s0 - kGrpShift : 0, q1 = row1 >= 0 ? p1 + r * s1 - kGrpShift : 0;
  hacc4_t a00 = {0, 0, 0, 0}, a10 = {0, 0, 0, 0}, a11 = {0, 0, 0, 0};
  double g0 = 0.0, g1 = 0.0;
  for (int64_t w0 = 0; w0 < n; w0 += kGrpIdx) {
    const int nw = (int)min<int64_t>(n - w0, kGrpIdx);
    for (int i = tid; i < nw; i += 256) sIdx[i] = d.grpObs[o0 + w0 + i];
    __syncthreads();
    const int nch = (nw + kGrpChunk - 1) / kGrpChunk;
    group_issue(d, sIdx, min(nw, kGrpChunk), stg, wave, lane);
    for (int k = 0; k < nch; k++) {
      const int c0 = k * kGrpChunk, nv = min(nw - c0, kGrpChunk);
      if (k + 1 < nch) {  // buffer (k + 1) & 1: its readers (chunk k - 1) passed the last barrier
        group_issue(d, sIdx + c0 + kGrpChunk, min(nw - c0 - kGrpChunk, kGrpChunk), stg + ((k + 1) & 1) * kGrpStage, wave, lane);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kGrpLoads) : "memory");
      } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      }
      __builtin_amdgcn_s_barrier();  // every wave's part of chunk k landed
      __builtin_amdgcn_sched_barrier(0);
      const rec_t* S = stg + (k & 1) * kGrpStage;
      for (int ks = wave; 2 * ks < nv; ks += 4) {
        const int c = 2 * ks + (l4 >> 1);
        const rec_t* rc = S + min(c, nv - 1) * kGrpPlanes;  // branch-free: past the chunk / invalid columns masked
        rec_t er, v0, v1;
        lds_read3(rc + kJe + r, rc + q0, rc + q1, er, v0, v1);
        if (c >= nv) er = v0 = v1 = 0;
        if (row0 < 0) v0 = 0;
        if (row1 < 0) v1 = 0;
        g0 += (double)v0 * er, g1 += (double)v1 * er;
        if (mode == 0) {
          a00 = mfma_h(v0, v0, a00);
          a10 = mfma_h(v1, v0, a10);
          a11 = mfma_h(v1, v1, a11);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();  // chunk k's readers done before its buffer is refilled (or sIdx / the epilogue)
    }
  }
  group_finish(d, lambda, mode, row0, row1, a00, a10, a11, g0, g1, smem);
}

// ------------------------------------------------------------------ launch wrapper
// independent of the landmark elimination: vb_damp_factor_solve runs the groups on the side stream beside it
void launch_groups(const Dev& d, double lambda, hipStream_t st, int mode) {
  if (d.nGroups) launchK(obs_group_kernel, dim3((unsigned)d.nGroups), dim3(256), 0, st, d, lambda, mode);
}
}  // namespace viba
