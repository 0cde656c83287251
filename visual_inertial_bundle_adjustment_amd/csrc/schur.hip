// Schur complement of the eliminated landmark block into the reduced system (the update half of BaSpaCho's
// elimination of the point range, Optimizer.cpp:200-206, and addDamping on the reduced diagonal,
// Optimizer.cpp:136-146), gfx950:
//   schur_run4_kernel     S_IJ -= sum_l Y_lI^T Y_lJ by target tile, compact runs, register operands
//   damp_small_kernel     the reduced diagonal's damping
//   reduced_rhs_kernel    rhs = gRedNew - sum Y^T zNew (new-gradient solve)
#include "kernel_common.hpp"
#include "host.hpp"

namespace viba {

// Schur assembly by target tile (finalize.hip builds the work list; engine.hpp TileWork / TileEnt), in
// compact runs with register operands.  finalize.hip sorts every tile's landmark entries by their (row mask
// in tile I, row mask in tile J): a work item is a sequence of RUNS of landmarks touching exactly the
// same tile rows.  Within a run the c-th panel column of a landmark inside tile I is compact column c
// (its rows ascend with its columns), K is dense (3 rows per landmark), and the compact nJ x nI product
// needs only ceil(nJ / 16) x ceil(nI / 16) blocks of v_mfma_f64_16x16x4_f64 per 4 K rows: 34M MFMAs
// on config C against 70M for the tile-coordinate form (16-row masks, one padded k-step per landmark;
// that form and the LDS-image forms are in the history).  No images and no barriers: a task is (run, chunk of <= kCh landmarks, compact
// block row a of the J side); a wave takes every fourth task of its item and accumulates the nI-wide
// block row over the chunk's K (3 rows per landmark), its operands loaded straight from the Y panel (lane l:
// compact column 16 a + (l & 15) / 16 b + (l & 15); K rows by plane groups, schur_task).  At the end of the task the block row is added into
// the item's LDS tile accumulator with LDS atomics (tasks of different waves overlap), through
// wave-private compact -> tile row maps.
constexpr int kCh = kSchurCh;  // landmarks per task
constexpr int kTR = kSchurTR;  // compact block rows per task (1 or 2)

// C -= acc of one task through the run's compact -> tile row maps: every map entry of the task read up
// front (one LDS wait), the adds predicated
// the plane groups' loads one group ahead (VIBA_SCHUR_PF=1: with two-row fp64 tasks the operands of two groups
// and the accumulators need three waves per SIMD, and ran as fast as four waves without it, 2558 / 2557 us, r06w)
// or not (default: four waves per SIMD, the other waves cover the latency; fp32 records 2026 -> 1726 us alone
// at config C, r06r; fp64 with one-row tasks 2522 -> 2458 us, r06aa)
#ifndef VIBA_SCHUR_PF
#define VIBA_SCHUR_PF 0
#endif
#ifndef VIBA_SCHUR_WAVES
#define VIBA_SCHUR_WAVES (VIBA_SCHUR_PF ? 3 : 4)
#endif
// one panel column's three planes of the plane-interleaved Y: a 16 B and an 8 B load (fp64), one 12 B load (fp32)
__device__ __forceinline__ void load3(const double* p, double (&v)[3]) {
  typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
  const d2u x = *reinterpret_cast<const d2u*>(p);
  v[0] = x.x, v[1] = x.y, v[2] = p[2];
}
__device__ __forceinline__ void load3(const float* p, float (&v)[3]) {
  typedef float f3u __attribute__((ext_vector_type(3), aligned(4)));
  const f3u x = *reinterpret_cast<const f3u*>(p);
  v[0] = x.x, v[1] = x.y, v[2] = x.z;
}
// two adjacent panel columns' planes (fp64: three 16 B loads for six values, where two load3 take four)
__device__ __forceinline__ void load6(const double* p, double (&v0)[3], double (&v1)[3]) {
  typedef double d2u __attribute__((ext_vector_type(2), aligned(8)));
  const d2u x = *reinterpret_cast<const d2u*>(p), y = *reinterpret_cast<const d2u*>(p + 2),
            z = *reinterpret_cast<const d2u*>(p + 4);
  v0[0] = x.x, v0[1] = x.y, v0[2] = y.x, v1[0] = y.y, v1[1] = z.x, v1[2] = z.y;
}

__device__ __forceinline__ void load6(const float* p, float (&v0)[3], float (&v1)[3]) { load3(p, v0), load3(p + 3, v1); }

// Compact column of operand block b, lane l15 (I side), and compact row r of J-side block i.  Off-diagonal
// fp64 tasks pair the blocks: blocks 2p and 2p + 1 take the even and the odd compact columns of
// [32 p, 32 p + 32), so a lane's two columns are adjacent in the panel (load6); an unpaired block (the last of
// an odd count, a one-row task, diagonal tiles, fp32 records) takes 16 consecutive columns.  The diagonal
// tiles keep the consecutive map: their block triangle must be the element triangle.
template <int NB, bool PAIR>
__device__ __forceinline__ int schur_col(int b, int l15) {
  return (PAIR && b < 2 * (NB / 2)) ? 32 * (b >> 1) + 2 * l15 + (b & 1) : 16 * b + l15;
}
template <int NR, bool PAIR>
__device__ __forceinline__ int schur_row(int a0, int i, int r) {
  return (PAIR && NR == 2) ? 32 * (a0 >> 1) + 2 * r + i : 16 * (a0 + i) + r;
}

template <int NBI, int NR, bool DIAG>
__device__ __forceinline__ void schur_epilogue(const hacc4_t (&acc)[NR][NBI], int a0, int l4, int l15,
                                               const uint8_t* posI, const uint8_t* posJ, int nI, int nJ, double* C) {
  constexpr bool PAIR = !DIAG && !VIBA_MIXED;
  int colT[NBI];
  int rowT[NR][4];
#pragma unroll
  for (int b = 0; b < NBI; b++) colT[b] = posI[min(schur_col<NBI, PAIR>(b, l15), TS - 1)];
#pragma unroll
  for (int i = 0; i < NR; i++)
#pragma unroll
    for (int q = 0; q < 4; q++) rowT[i][q] = posJ[min(schur_row<NR, PAIR>(a0, i, kAccL4 * l4 + kAccR * q), TS - 1)];
#pragma unroll
  for (int i = 0; i < NR; i++)
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const bool mv = schur_row<NR, PAIR>(a0, i, kAccL4 * l4 + kAccR * q) < nJ;
#pragma unroll
      for (int b = 0; b < NBI; b++)
        if ((!DIAG || a0 + i <= b) && mv && schur_col<NBI, PAIR>(b, l15) < nI)
          atomicAdd(C + rowT[i][q] * TS + colT[b], -(double)acc[i][b][q]);
    }
}

// rhs -= Y^T z over a chunk's landmarks (diagonal tiles), lanes over the run's compact I columns, four
// landmarks' loads in flight per step
__device__ __forceinline__ void schur_rhs(const Dev& d, const uint32_t (*ecol)[2], const TileEnt* ents, int c0, int nl,
                                          int lane, const uint8_t* posI, double* rq) {
  double racc = 0.0;
  int e = c0;
  for (; e + 4 <= c0 + nl; e += 4) {
    double y[4][3], z[4][3];
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const rec_t* yp = d.Y + 3 * ((int64_t)ecol[e + u][0] + lane);
      const double* zz = d.z + 3 * (int64_t)ents[e + u].lm;
#pragma unroll
      for (int q = 0; q < 3; q++) y[u][q] = (double)yp[q], z[u][q] = zz[q];
    }
#pragma unroll
    for (int u = 0; u < 4; u++) racc += y[u][0] * z[u][0] + y[u][1] * z[u][1] + y[u][2] * z[u][2];
  }
  for (; e < c0 + nl; e++) {
    const rec_t* y = d.Y + 3 * ((int64_t)ecol[e][0] + lane);
    const double* zz = d.z + 3 * (int64_t)ents[e].lm;
    racc += (double)y[0] * zz[0] + (double)y[1] * zz[1] + (double)y[2] * zz[2];
  }
  atomicAdd(&rq[posI[lane]], -racc);
}

// One task's K loop: acc[i][b] += A_i^T B_b over the K rows (3 per landmark) of landmarks c0 .. c0 + rows / 3,
// A_i = compact J-side block row a0 + i (NR of them), B_b = compact I-side block b < NBI.  Round 6: Y is
// plane-interleaved (plane q of panel column c at Y[3 c + q]) and the K rows are taken in plane groups: per
// group of four landmarks, lane group l4 takes landmark c0 + 4 m + l4 and its three planes over three
// consecutive k-steps, so a lane loads one column's three planes at once (a 16 B and an 8 B load, or one 12 B
// load for fp32 records) instead of three 8 B gathers for three k-steps (the gathers cost as instructions:
// DESIGN.md §4).  The last group's lanes past the task's landmarks read the zero pad (a dense remainder loop
// for the last nl % 4 landmarks held the accumulators across two loop bodies: fp64 spilled at four waves per
// SIMD; r06w: 2609 -> 2557 us alone at config C).  Columns past nJ / nI load neighbouring panel data into
// accumulator rows / columns that are never stored.
template <int NBI, int NR, bool DIAG>
__device__ __forceinline__ void schur_task(const Dev& d, const uint2* ec, int c0, int rows, int a0, int l4, int l15,
                                           const uint8_t* posI, const uint8_t* posJ, int nI, int nJ, double* C) {
  hacc4_t acc[NR][NBI];
#pragma unroll
  for (int i = 0; i < NR; i++)
#pragma unroll
    for (int b = 0; b < NBI; b++) acc[i][b] = hacc4_t{0, 0, 0, 0};
  const rec_t* Y = d.Y;  // plane-interleaved: plane q of global panel column c at Y[3 c + q]
  auto mm = [&](const rec_t (&av)[NR], const rec_t (&bv)[NBI]) {
#pragma unroll
    for (int i = 0; i < NR; i++)
#pragma unroll
      for (int b = 0; b < NBI; b++)
        if (!DIAG || a0 + i <= b) acc[i][b] = mfma_h(av[i], bv[b], acc[i][b]);
  };
  // groups of four landmarks: lane group l4 takes landmark c0 + 4 m + l4 and its three planes over three
  // consecutive k-steps, so its operands of those k-steps are one column's three consecutive values (one 16 B
  // and one 8 B load per operand block instead of three 8 B gathers); the next group's loads are issued
  // before this group's MFMAs
  const int nl = rows / 3, nfull = (nl + 3) >> 2;
  constexpr bool PAIR = !DIAG && !VIBA_MIXED;
  auto ld3 = [&](int m, rec_t (&a3)[NR][3], rec_t (&b3)[NBI][3]) {
    // lanes past the task's landmarks read the zero pad (panel column 0 of yZero: every offset below < 192)
    const bool lv = 4 * m + l4 < nl;
    const uint2 c = lv ? ec[c0 + 4 * m + l4] : make_uint2(0u, 0u);
    const rec_t* base = lv ? Y : d.yZero;
    const rec_t* pJ = base + 3 * (int64_t)c.y;
    const rec_t* pI = base + 3 * (int64_t)c.x;
    if constexpr (PAIR && NR == 2) {
      load6(pJ + 3 * schur_row<NR, PAIR>(a0, 0, l15), a3[0], a3[1]);
    } else {
#pragma unroll
      for (int i = 0; i < NR; i++) load3(pJ + 3 * schur_row<NR, PAIR>(a0, i, l15), a3[i]);
    }
#pragma unroll
    for (int b = 0; b < NBI; b++) {
      if (PAIR && b < 2 * (NBI / 2)) {
        if ((b & 1) == 0) load6(pI + 3 * schur_col<NBI, PAIR>(b, l15), b3[b], b3[b + 1]);
      } else {
        load3(pI + 3 * schur_col<NBI, PAIR>(b, l15), b3[b]);
      }
    }
  };
  auto mm3 = [&](const rec_t (&a3)[NR][3], const rec_t (&b3)[NBI][3]) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
      rec_t av[NR], bv[NBI];
#pragma unroll
      for (int i = 0; i < NR; i++) av[i] = a3[i][q];
#pragma unroll
      for (int b = 0; b < NBI; b++) bv[b] = b3[b][q];
      mm(av, bv);
    }
  };
#if VIBA_SCHUR_PF
  if (nfull > 0) {
    rec_t a3[NR][3], b3[NBI][3];
    ld3(0, a3, b3);
    for (int m = 0; m < nfull; m++) {
      rec_t a3n[NR][3], b3n[NBI][3];
      if (m + 1 < nfull) ld3(m + 1, a3n, b3n);
      mm3(a3, b3);
      if (m + 1 < nfull) {
#pragma unroll
        for (int i = 0; i < NR; i++)
#pragma unroll
          for (int q = 0; q < 3; q++) a3[i][q] = a3n[i][q];
#pragma unroll
        for (int b = 0; b < NBI; b++)
#pragma unroll
          for (int q = 0; q < 3; q++) b3[b][q] = b3n[b][q];
      }
    }
  }
#else
#pragma unroll 1
  for (int m = 0; m < nfull; m++) {  // (the other waves of the SIMD cover the loads' latency)
    rec_t a3[NR][3], b3[NBI][3];
    ld3(m, a3, b3);
    mm3(a3, b3);
    __builtin_amdgcn_sched_barrier(0);  // no hoisting of the next group's loads (register pressure)
  }
#endif
  // C -= acc through the run's compact -> tile maps (LDS atomics: tasks of other waves overlap)
  schur_epilogue<NBI, NR, DIAG>(acc, a0, l4, l15, posI, posJ, nI, nJ, C);
}

// Schur tile products, one workgroup per work item (TileWork: a target tile and <= 256 of its landmark
// entries).  The item's runs (masks) and its tasks come precomputed from finalize (api.hip), the
// tasks dealt to the waves longest-first (TileWork::wOff), so the kernel has no run scan and the waves
// are balanced at the final barrier.  Four waves per SIMD (the k-loops are bound by gather latency).
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VIBA_SCHUR_WAVES, VIBA_SCHUR_WAVES))) schur_run4_kernel(Dev d, double lambda) {
  __shared__ double C[TS * TS];
  __shared__ uint32_t ecol[256][2];
  __shared__ uint64_t rmask[256][2];
  __shared__ uint8_t posW[4][2][TS];
  __shared__ double rq[TS];
  const int64_t w = xcd_block(blockIdx.x, gridDim.x);
  const TileWork* wp = d.tileWorks + w;  // fields read in place (a by-value copy went to scratch:
  const TileWork wk = *wp;                 // wOff is indexed by the wave)
  const bool diag = wk.I == wk.J;
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int l15 = lane & 15, l4 = lane >> 4;
  const int cnt = wk.count;
  const TileEnt* ents = d.tileEnts + wk.start;
  if (tid < cnt) ecol[tid][0] = ents[tid].colI, ecol[tid][1] = ents[tid].colJ;
  if (tid < wk.nRuns) {
    const uint64_t* rm = d.schurRuns + 2 * ((int64_t)wk.runFirst + tid);
    rmask[tid][0] = rm[0], rmask[tid][1] = rm[1];
  }
  for (int i = tid; i < TS * TS; i += 256) C[i] = 0.0;
  if (tid < TS) rq[tid] = 0.0;
  __syncthreads();
  uint8_t* posI = posW[wave][0];
  uint8_t* posJ = posW[wave][1];
  const uint2* ec2 = reinterpret_cast<const uint2*>(&ecol[0][0]);
  const uint32_t* tasks = d.schurTasks + wk.taskFirst;
  const int tBeg = wp->wOff[wave], tEnd = wp->wOff[wave + 1];
  int cur = -1;
  for (int t = tBeg; t < tEnd; t++) {
    const uint32_t code = __builtin_amdgcn_readfirstlane(tasks[t]);
    const int r = code & 255, c0 = (code >> 8) & 255, nl = (code >> 16) & 63, a0 = (code >> 22) & 3;
    const uint64_t mI = uniform64(rmask[r][0]), mJ = uniform64(rmask[r][1]);
    const int nI = __popcll(mI), nJ = __popcll(mJ);
    const int nbI = (nI + 15) >> 4, nbJ = (nJ + 15) >> 4;
    if (r != cur) {  // the run's compact -> tile row maps (wave-private)
      __builtin_amdgcn_wave_barrier();  // the previous run's readers are done
      if ((mI >> lane) & 1) posI[__popcll(mI & ((1ull << lane) - 1))] = (uint8_t)lane;
      if ((mJ >> lane) & 1) posJ[__popcll(mJ & ((1ull << lane) - 1))] = (uint8_t)lane;
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      cur = r;
    }
    const int rows = 3 * nl;
    const int nr = min(kTR, nbJ - a0);
    const int sel = ((nbI - 1) * 2 + (nr - 1)) * 2 + (diag ? 1 : 0);
    // one specialised task (k-loop + epilogue) per (I-side blocks, J-side rows of this task, diagonal
    // tile): no per-MFMA predicates, gathers at immediate offsets from per-step base pointers
    switch (sel) {
#define VIBA_SCHUR_CASE(NBI, NR)                                                                      \
  case ((NBI - 1) * 2 + (NR - 1)) * 2:                                                                \
    schur_task<NBI, NR, false>(d, ec2, c0, rows, a0, l4, l15, posI, posJ, nI, nJ, C);                 \
    break;                                                                                            \
  case ((NBI - 1) * 2 + (NR - 1)) * 2 + 1:                                                            \
    schur_task<NBI, NR, true>(d, ec2, c0, rows, a0, l4, l15, posI, posJ, nI, nJ, C);                  \
    break;
      VIBA_SCHUR_CASE(1, 1) VIBA_SCHUR_CASE(2, 1) VIBA_SCHUR_CASE(3, 1) VIBA_SCHUR_CASE(4, 1)
#if VIBA_SCHUR_TR == 2
      VIBA_SCHUR_CASE(1, 2) VIBA_SCHUR_CASE(2, 2) VIBA_SCHUR_CASE(3, 2) VIBA_SCHUR_CASE(4, 2)
#endif
#undef VIBA_SCHUR_CASE
      default: break;
    }
    if (diag && a0 == 0 && lane < nI) schur_rhs(d, ecol, ents, c0, nl, lane, posI, rq);
  }
  __syncthreads();
  double* Ct = d.tiles + (int64_t)wk.tile * TS * TS;
  if (wk.kind == 1) {
    for (int i = tid; i < TS * TS; i += 256)
      if (C[i] != 0.0) atomicAdd(Ct + i, C[i]);
  } else if (wk.kind == 2) {  // the only writer of the tile (left out of the clear)
    for (int i = tid; i < TS * TS; i += 256) Ct[i] = C[i];
  } else {
    for (int i = tid; i < TS * TS; i += 256) Ct[i] += C[i];
  }
  if (diag && tid < TS) {
    const int64_t row = (int64_t)wk.I * TS + tid;
    if (row < d.nRed && rq[tid] != 0.0) atomicAdd(d.rhs + row, rq[tid]);
  }
}

// damping of the small-factor part of the diagonal (visual part: obs_group_kernel) and the
// identity term (Optimizer.cpp:136-146 addDamping: H_ii += lambda * H_ii + lambda)
__global__ void damp_small_kernel(Dev d, double lambda, int addIdentity) {
  const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= d.nRed || !owns_col(d, r / TS)) return;
  double* p = tile_ptr(d, r, r);
  *p = *p * (1.0 + lambda) + (addIdentity ? lambda : 0.0);
}

// new reduced RHS (vb_solve_with_new_gradient / vb_assemble_new_rhs): rhs = gRedNew - sum Y^T zNew over this
// shard's landmarks; rhs starts as a copy of gRedNew, one block per chunk of <= 1024 landmarks of one
// reduced variable X (the calibration variables see every landmark: one block each took 2.6 ms)
__global__ void __launch_bounds__(256) reduced_rhs_kernel(Dev d) {
  __shared__ double g[4][32];
  const int64_t* ch = d.lxChunk + 3 * (int64_t)blockIdx.x;
  const int X1 = (int)ch[0];
  const int d1 = d.rvDim[X1];
  const int64_t off1 = d.rvOff[X1];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // lanes = (landmark slot, column j): P = d1 rounded up to a power of two lanes per landmark, so a
  // wave reads 64 / P landmarks' panel rows at once (runs of d1 doubles per plane) instead of one
  // landmark's 3 d1 values per lane
  const int P = d1 <= 4 ? 4 : d1 <= 8 ? 8 : d1 <= 16 ? 16 : 32;
  const int S = 64 / P, slot = lane / P, j = lane % P;
  double acc = 0.0;
  for (int64_t idx = ch[1] + wave * S + slot; idx < ch[2]; idx += 4 * S) {
    const int64_t l = d.lxLm[idx];
    if (j >= d1 || l < d.lmB || l >= d.lmE) continue;
    const rec_t* y1 = d.Y + d.lmY[l] + 3 * (d.lxCol[idx] + j);
    acc += (double)y1[0] * d.zNew[l * 3] + (double)y1[1] * d.zNew[l * 3 + 1] + (double)y1[2] * d.zNew[l * 3 + 2];
  }
  for (int o = P; o < 64; o <<= 1) acc += __shfl_xor(acc, o, 64);  // over the landmark slots
  if (lane < P && lane < d1) g[wave][lane] = acc;
  __syncthreads();
  if (tid < d1) atomicAdd(&d.rhs[off1 + tid], -(g[0][tid] + g[1][tid] + g[2][tid] + g[3][tid]));
}

// ------------------------------------------------------------------ launch wrappers
// S(tiles) += damping + direct - Schur; rhs = gRed(+visual) - sum Y^T z  (rhs must be zero on entry), in
// three parts: the damping of the assembled direct terms (a read-modify-write of the diagonal, so it
// precedes the observation-group atomics), the observation-group Gram blocks (obs_group.hip), the tile products
void launch_damp(const Dev& d, double lambda, int addIdentity, hipStream_t st) {
  if (d.nRed) launchK(damp_small_kernel, dim3(blocks(d.nRed, 256)), dim3(256), 0, st, d, lambda, addIdentity);
}
void launch_schur_products(const Dev& d, double lambda, hipStream_t st) {
  if (d.nTileWorks) launchK(schur_run4_kernel, dim3((unsigned)d.nTileWorks), dim3(256), 0, st, d, lambda);
  launch_axpby(d.rhs, d.gRed, 1.0, 1.0, d.nRed, st);
}
void launch_schur(const Dev& d, double lambda, int addIdentity, hipStream_t st) {
  launch_damp(d, lambda, addIdentity, st);
  launch_groups(d, lambda, st);
  launch_schur_products(d, lambda, st);
}
void launch_reduced_grad(const Dev& d, int mode, hipStream_t st) {
  if (mode == 0) return launch_groups(d, 0.0, st, 1);  // visual gradient of this shard's observations
  (void)hipMemcpyAsync(d.rhs, d.gRedNew, (size_t)d.nT * TS * sizeof(double), hipMemcpyDeviceToDevice, st);
  if (d.nLxChunk) launchK(reduced_rhs_kernel, dim3((unsigned)d.nLxChunk), dim3(256), 0, st, d);
}
}  // namespace viba

