// Landmark elimination (replacing BaSpaCho's elimination of the point range, Optimizer.cpp:200-206, and
// addDamping on the point block, Optimizer.cpp:136-146), gfx950:
//   landmark_stage_kernel one wave per landmark: V = sum Jp^T Jp (damped), g_p, the W panel in LDS,
//   (_obs_wg, _list, landmark_kernel) 3x3 Cholesky, z = L^-1 g_p, Y = L^-1 W
//   landmark_z_kernel     zNew = L^-1 gpNew
//   landmark_lone_kernel  landmarks that only base-map factors see: the 3 x 3 block alone
// Every path adds the landmark's base-map sums (BaseMapDev::Vg, basemap.hip) to V and g before the damped
// Cholesky, so damping acts on the full block; nothing is read on a handle without base-map factors.
#include "kernel_common.hpp"

namespace viba {

// the one lane that ends a landmark's 3 x 3 block: the breakdown flag, Vchol, z = L^-1 g and gp
__device__ __forceinline__ void landmark_finish(const Dev& d, int64_t l, const Chol3& L, bool ok, const double* g) {
  if (!ok) atomicOr(d.err, 2);
  L.store(d.Vchol + l * 6);
  double z0 = g[0], z1 = g[1], z2 = g[2];
  chol3_fwd(L, z0, z1, z2);
  d.z[l * 3] = z0, d.z[l * 3 + 1] = z1, d.z[l * 3 + 2] = z2;
  d.gp[l * 3] = g[0], d.gp[l * 3 + 1] = g[1], d.gp[l * 3 + 2] = g[2];
}
// the landmark's base-map factors: V (v00 v10 v20 v11 v21 v22) += Vg[0..6), g += Vg[6..9)
__device__ __forceinline__ void basemap_add_g(const Dev& d, int64_t l, double* g) {
  if (!d.bm.Vg) return;
  const double* b = d.bm.Vg + l * 9;
  g[0] += b[6], g[1] += b[7], g[2] += b[8];
}
__device__ __forceinline__ void basemap_add_v(const Dev& d, int64_t l, double& v00, double& v10, double& v20, double& v11,
                                              double& v21, double& v22) {
  if (!d.bm.Vg) return;
  const double* b = d.bm.Vg + l * 9;
  v00 += b[0], v10 += b[1], v20 += b[2], v11 += b[3], v21 += b[4], v22 += b[5];
}
// Y(:, c) = L^-1 w of panel column c (Y plane-interleaved: plane q of panel column c at Y[3 c + q]), and the
// same for the columns first, first + stride, ... of a W panel in LDS
__device__ __forceinline__ void panel_column(const Chol3& L, rec_t* Y, int64_t c, double w0, double w1, double w2) {
  chol3_fwd(L, w0, w1, w2);
  Y[3 * c] = w0, Y[3 * c + 1] = w1, Y[3 * c + 2] = w2;
}
__device__ __forceinline__ void panel_solve(const Chol3& L, const double* W, rec_t* Y, int64_t ncol, int first, int stride) {
  for (int64_t c = first; c < ncol; c += stride) panel_column(L, Y, c, W[3 * c], W[3 * c + 1], W[3 * c + 2]);
}

// ------------------------------------------------------------------ by panel column
// One wave per landmark (Optimizer.cpp:136-146 restricted to the point block, then the point part
// of the sparse elimination, Optimizer.cpp:200-231):
//   lanes over the landmark's observations: V = sum Jp^T Jp, g = sum Jp^T e (record planes 0..7,
//   64 B of each 576 B record), wave reduction; every lane then holds the damped 3 x 3 Cholesky L
//   mode 0: lanes over the Y panel columns: W(:, c) = sum over the observation slots of the column's
//   block of Jp^T J_x(:, j), Y(:, c) = L^-1 W(:, c) (no atomics: each column has one owner)
//   mode 1: g only, into gpNew (gradient pass of the bad-step path)
__device__ __forceinline__ void landmark_eliminate(const Dev& d, double lambda, int mode, int64_t l) {
  const int lane = threadIdx.x & 63;
  const rec_t* Jt = d.Jt;
  const int64_t o0 = d.lmObs[l], o1 = d.lmObs[l + 1];
  double v00 = 0, v10 = 0, v20 = 0, v11 = 0, v21 = 0, v22 = 0, g[3] = {0, 0, 0};
  for (int64_t o = o0 + lane; o < o1; o += 64) {
    const rec_t* r = Jt + o * kJA;  // planes 0..7 live in region A
    const double e0 = r[kJe], e1 = r[kJe + 1];
    const double a0 = r[kJpt + 0], a1 = r[kJpt + 1], a2 = r[kJpt + 2];
    const double b0 = r[kJpt + 3], b1 = r[kJpt + 4], b2 = r[kJpt + 5];
    g[0] += a0 * e0 + b0 * e1, g[1] += a1 * e0 + b1 * e1, g[2] += a2 * e0 + b2 * e1;
    if (mode == 0) {
      v00 += a0 * a0 + b0 * b0, v10 += a1 * a0 + b1 * b0, v20 += a2 * a0 + b2 * b0;
      v11 += a1 * a1 + b1 * b1, v21 += a2 * a1 + b2 * b1, v22 += a2 * a2 + b2 * b2;
    }
  }
  g[0] = wave_sum(g[0]), g[1] = wave_sum(g[1]), g[2] = wave_sum(g[2]);
  basemap_add_g(d, l, g);
  if (mode == 1) {
    if (lane == 0) d.gpNew[l * 3] = g[0], d.gpNew[l * 3 + 1] = g[1], d.gpNew[l * 3 + 2] = g[2];
    return;
  }
  v00 = wave_sum(v00), v10 = wave_sum(v10), v20 = wave_sum(v20);
  v11 = wave_sum(v11), v21 = wave_sum(v21), v22 = wave_sum(v22);
  basemap_add_v(d, l, v00, v10, v20, v11, v21, v22);
  bool ok;
  const Chol3 L = chol3_damped(v00, v10, v20, v11, v21, v22, lambda, ok);
  if (lane == 0) landmark_finish(d, l, L, ok, g);
  const int64_t cb = d.lmY[l] / 3, ncol = d.lmY[l + 1] / 3 - cb;
  rec_t* Y = d.Y + d.lmY[l];
  for (int64_t c = lane; c < ncol; c += 64) {
    const int32_t b = d.pcBlk[cb + c];
    const int j = (int)(c - d.blkCol[b]);
    double w0 = 0, w1 = 0, w2 = 0;
    for (int64_t e = d.bxStart[b]; e < d.bxStart[b + 1]; e++) {
      const int32_t ent = d.bxEnt[e];
      const int s = ent & 3;
      const int64_t o = ent >> 2;
      const rec_t* r = Jt + o * kJA;
      const rec_t* x = jt_plane(Jt, d.nObsPad, o, slotPlane(s) + j);
      const double x0 = x[0], x1 = x[slotStride(s)];
      w0 += r[kJpt + 0] * x0 + r[kJpt + 3] * x1;
      w1 += r[kJpt + 1] * x0 + r[kJpt + 4] * x1;
      w2 += r[kJpt + 2] * x0 + r[kJpt + 5] * x1;
    }
    panel_column(L, Y, c, w0, w1, w2);
  }
}
__global__ void __launch_bounds__(256) landmark_kernel(Dev d, double lambda, int mode, int64_t lo, int64_t hi) {
  const int64_t l = lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= hi) return;
  landmark_eliminate(d, lambda, mode, l);
}

// ------------------------------------------------------------------ by observation
// Landmark elimination by observation (mode 0, default).  One wave per landmark; each half-wave takes
// one of the landmark's observations at a time and its 32 lanes the observation's 32 slot columns
// [pose 6 | extr 6 | intr 17 | vel 3] (record planes 8..71, read once and coalesced, with the point
// Jacobian and residual of planes 0..7): the column's contribution Jp^T J_x(:, j) goes into the
// landmark's W panel in LDS at panel column obCol + j with LDS atomics (both halves may hit a shared
// calibration block), and lane 0 of the half accumulates V and g.  Then the damped 3 x 3 Cholesky,
// z, and Y = L^-1 W over the panel columns.  No per-block observation lists: every record is read
// once.  Two launches by panel width (finalize.hip lmList): landmarks with up to kLmSmallCols columns one
// per wave, their records staged in LDS (landmark_stage_kernel, below); the wider ones (long tracks) one
// per workgroup, landmark_obs_wg_kernel, whose panel is per workgroup.  Measured on config C (r01-r04):
// 1.04 + 0.72 ms against 2.63 for the per-column landmark_kernel; one 48 KB per-wave class for all ran at
// 2.9 ms and the per-workgroup kernel for all at 2.1 (occupancy vs. barriers).
constexpr int kLmBigCols = 2048;  // 3 x 2048 doubles = 48 KB of dynamic LDS per workgroup; wider: per-column path

// The narrow class with the landmark's records streamed through LDS (round 6): a landmark's observations
// are consecutive, so its records are one contiguous span of each record region; the wave copies them in
// chunks of kLmCh observations with 16 B global_load_lds (a handful of wide loads per chunk instead of
// ~10 narrow loads per observation and half-wave), double-buffered (chunk k + 1 in flight while chunk k
// is consumed), wave-private: one wave per workgroup, no barriers.  The half-waves then read their
// observation's point Jacobian, residual and slot-column planes from LDS (inline-asm ds_reads behind one
// wait: plain LDS loads would make the compiler drain the DMA in flight first, as in obs_group_kernel).
// observations per staged chunk: swept at config C (r06n, the elimination alone): fp64 2 / 3 / 4 / 6 / 8 / 16
// -> 1265 / 1249 / 1239 / 1299 / 1331 / 1555 us (the LDS per wave sets the occupancy), fp32 records 2 / 3 / 4 /
// 6 -> 1154 / 1161 / 1084 / 1070 us; the per-lane load form it replaces: 1339 / 1106 us
constexpr int kLmCh = VIBA_MIXED ? 6 : 4;
constexpr int kLmInA = (kLmCh * kJA / kRecV + 63) / 64;  // global_load_lds per chunk, region A
constexpr int kLmInB = (kLmCh * kJB / kRecV + 63) / 64;  // region B (the tail lanes land in padding)
constexpr int kLmBOff = kLmInA * 64 * kRecV;             // staged region B (rec_t offset in a buffer)
constexpr int kLmCOff = (kLmInA + kLmInB) * 64 * kRecV;  // staged obCol words of the chunk (64 int32 slots)
constexpr int kLmBuf = kLmCOff + 256 / (int)sizeof(rec_t);  // rec_t per buffer
static_assert(kLmCh * kJA <= kLmBOff, "region A of a chunk fits its DMA slots");
// the staged kernels' dynamic LDS: nbuf chunk buffers, then the W panel of `cols` columns (its offset in doubles)
constexpr int lm_panel_offset(int nbuf) { return (nbuf * kLmBuf * (int)sizeof(rec_t) + 7) / 8; }
constexpr uint32_t lm_lds_bytes(int nbuf, int cols) { return (uint32_t)((lm_panel_offset(nbuf) + 3 * cols) * sizeof(double)); }

__device__ __forceinline__ void lm_issue(const Dev& d, int64_t oa, int nv, rec_t* buf, int lane) {
  const rec_t* gA = d.Jt + oa * kJA;
  const rec_t* gB = d.Jt + d.nObsPad * kJA + oa * kJB;
  const int vA = nv * (kJA / kRecV), vB = nv * (kJB / kRecV);  // the chunk's pieces; others re-read piece 0
#pragma unroll
  for (int j = 0; j < kLmInA; j++) {
    const int p = j * 64 + lane;
    glds<16>(gA + (p < vA ? p : 0) * kRecV, buf + j * 64 * kRecV);
  }
#pragma unroll
  for (int j = 0; j < kLmInB; j++) {
    const int p = j * 64 + lane;
    glds<16>(gB + (p < vB ? p : 0) * kRecV, buf + kLmBOff + j * 64 * kRecV);
  }
  // the packed panel column / width words of the chunk's observation slots (4 per observation)
  const int32_t* gC = d.obCol + oa * 4;
  glds<4>(gC + (lane < 4 * nv ? lane : 0), buf + kLmCOff);
}
// one observation's share of a half-wave from the staged record: e (2), point Jacobian (6) at ra, the lane's
// two slot-column planes at rx and rx1
__device__ __forceinline__ void lm_read(const rec_t* ra, const rec_t* rx, const rec_t* rx1, const int32_t* rc,
                                        double (&a)[6], double& e0, double& e1, double& x0, double& x1, int32_t& pc) {
#if VIBA_MIXED
  float v[10];
  asm volatile(
      "ds_read_b32 %0, %11\n\tds_read_b32 %1, %11 offset:4\n\tds_read_b32 %2, %11 offset:8\n\t"
      "ds_read_b32 %3, %11 offset:12\n\tds_read_b32 %4, %11 offset:16\n\tds_read_b32 %5, %11 offset:20\n\t"
      "ds_read_b32 %6, %11 offset:24\n\tds_read_b32 %7, %11 offset:28\n\tds_read_b32 %8, %12\n\t"
      "ds_read_b32 %9, %13\n\tds_read_b32 %10, %14\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]),
        "=&v"(v[8]), "=&v"(v[9]), "=&v"(pc)
      : "v"(lds_addr(ra)), "v"(lds_addr(rx)), "v"(lds_addr(rx1)), "v"(lds_addr(rc))
      : "memory");
#else
  double v[10];
  asm volatile(
      "ds_read_b64 %0, %11\n\tds_read_b64 %1, %11 offset:8\n\tds_read_b64 %2, %11 offset:16\n\t"
      "ds_read_b64 %3, %11 offset:24\n\tds_read_b64 %4, %11 offset:32\n\tds_read_b64 %5, %11 offset:40\n\t"
      "ds_read_b64 %6, %11 offset:48\n\tds_read_b64 %7, %11 offset:56\n\tds_read_b64 %8, %12\n\t"
      "ds_read_b64 %9, %13\n\tds_read_b32 %10, %14\n\ts_waitcnt lgkmcnt(0)"
      : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]), "=&v"(v[4]), "=&v"(v[5]), "=&v"(v[6]), "=&v"(v[7]),
        "=&v"(v[8]), "=&v"(v[9]), "=&v"(pc)
      : "v"(lds_addr(ra)), "v"(lds_addr(rx)), "v"(lds_addr(rx1)), "v"(lds_addr(rc))
      : "memory");
#endif
  static_assert(kJe == 0 && kJpt == 2, "record planes 0..7: e, point Jacobian");
  e0 = v[0], e1 = v[1];
#pragma unroll
  for (int k = 0; k < 6; k++) a[k] = v[2 + k];
  x0 = v[8], x1 = v[9];
}

// one wave's share of a landmark's observations, from LDS: the chunks k = wave, wave + nwaves, ... of
// kLmCh observations each (double-buffered in the wave's own two buffers at stg), W panel atomics in LDS;
// v[0..8] = the lane's partial V (v00 v10 v20 v11 v21 v22) and g (lanes jj == 0 of each half only)
__device__ __forceinline__ void lm_stage_loop(const Dev& d, int64_t o0, int64_t n, rec_t* stg, double* W, int wave,
                                              int nwaves, int lane, double (&v)[9]) {
  const int nch = (int)((n + kLmCh - 1) / kLmCh);
  const int h = lane >> 5, jj = lane & 31;
  const int s = jj < 6 ? 0 : jj < 12 ? 1 : jj < 29 ? 2 : 3;
  const int j = jj - (s == 0 ? 0 : s == 1 ? 6 : s == 2 ? 12 : 29);
  const int pl = slotPlane(s) + j, st = slotStride(s);
  // the lane's planes inside a staged record (a slot's planes never straddle the regions)
  const int xo = pl < kJA ? pl : kLmBOff + (pl - kJA), xstep = pl < kJA ? kJA : kJB;
  auto nvOf = [&](int k) { return (int)min<int64_t>(n - (int64_t)k * kLmCh, kLmCh); };
  if (wave < nch) lm_issue(d, o0 + (int64_t)wave * kLmCh, nvOf(wave), stg, lane);
  for (int k = wave, b = 0; k < nch; k += nwaves, b ^= 1) {
    const int64_t ob = o0 + (int64_t)k * kLmCh;
    const int nv = nvOf(k);
    if (k + nwaves < nch) {  // the other buffer: its reads (the wave's previous chunk) completed in program order
      lm_issue(d, ob + (int64_t)nwaves * kLmCh, nvOf(k + nwaves), stg + (b ^ 1) * kLmBuf, lane);
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(kLmInA + kLmInB + 1) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    const rec_t* S = stg + b * kLmBuf;
    for (int c = h; c < nv + (nv & 1); c += 2) {  // both halves run the same trip count (odd tail: one idles)
      const int cc = min(c, nv - 1);
      double a[6], e0, e1, x0, x1;
      int32_t pc;
      lm_read(S + cc * kJA, S + xo + cc * xstep, S + xo + cc * xstep + st,
              reinterpret_cast<const int32_t*>(S + kLmCOff) + 4 * cc + s, a, e0, e1, x0, x1, pc);
      const bool valid = c < nv;
      if (valid && jj == 0) {
        v[6] += a[0] * e0 + a[3] * e1, v[7] += a[1] * e0 + a[4] * e1, v[8] += a[2] * e0 + a[5] * e1;
        v[0] += a[0] * a[0] + a[3] * a[3], v[1] += a[1] * a[0] + a[4] * a[3];
        v[2] += a[2] * a[0] + a[5] * a[3], v[3] += a[1] * a[1] + a[4] * a[4];
        v[4] += a[2] * a[1] + a[5] * a[4], v[5] += a[2] * a[2] + a[5] * a[5];
      }
      if (valid && pc >= 0 && j < (pc & 31)) {
        // LDS atomics in inline asm: as atomicAdd the compiler put an s_waitcnt vmcnt(0) before them (it
        // cannot tell W from the DMA target), draining the next chunk's loads at every observation
        const int col = (pc >> 5) + j;
        const double w0 = a[0] * x0 + a[3] * x1, w1 = a[1] * x0 + a[4] * x1, w2 = a[2] * x0 + a[5] * x1;
        asm volatile("ds_add_f64 %0, %1\n\tds_add_f64 %0, %2 offset:8\n\tds_add_f64 %0, %3 offset:16"
                     ::"v"(lds_addr(W + 3 * col)), "v"(w0), "v"(w1), "v"(w2)
                     : "memory");
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");  // every atomic into W landed
}

__global__ void __launch_bounds__(64) landmark_stage_kernel(Dev d, double lambda, int64_t first) {
  extern __shared__ __attribute__((aligned(16))) double lsm[];
  rec_t* stg = reinterpret_cast<rec_t*>(lsm);  // two chunk buffers, then the W panel
  double* W = lsm + lm_panel_offset(2);
  const int lane = threadIdx.x;
  const int64_t l = d.lmList[first + xcd_block(blockIdx.x, gridDim.x)];
  const int64_t o0 = d.lmObs[l], o1 = d.lmObs[l + 1], n = o1 - o0;
  const int64_t cb = d.lmY[l] / 3, ncol = d.lmY[l + 1] / 3 - cb;
  for (int i = lane; i < 3 * ncol; i += 64) W[i] = 0.0;
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the clear landed before the asm atomics below
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // v00 v10 v20 v11 v21 v22 g0 g1 g2
  lm_stage_loop(d, o0, n, stg, W, 0, 1, lane, v);
#pragma unroll
  for (int k = 0; k < 9; k++) v[(k + 6) % 9] = wave_sum(v[(k + 6) % 9]);  // g, then V: the order this kernel was tuned in
  basemap_add_g(d, l, v + 6), basemap_add_v(d, l, v[0], v[1], v[2], v[3], v[4], v[5]);
  bool ok;
  const Chol3 L = chol3_damped(v[0], v[1], v[2], v[3], v[4], v[5], lambda, ok);
  if (lane == 0) landmark_finish(d, l, L, ok, v + 6);
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  panel_solve(L, W, d.Y + d.lmY[l], ncol, lane, 64);
}

// the same with one workgroup per landmark (its 8 half-waves share the observations, the W panel is
// one per workgroup): for the wide class, whose per-wave panels would cap the occupancy
__global__ void __launch_bounds__(256) landmark_obs_wg_kernel(Dev d, double lambda, int64_t first) {
  // the four waves' staging buffers (lm_stage_loop: wave w takes chunks w, w + 4, ...), then the W panel
  extern __shared__ __attribute__((aligned(16))) double lsm[];
  __shared__ double part[4][9];
  __shared__ double Ls[6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  rec_t* stg = reinterpret_cast<rec_t*>(lsm) + wave * 2 * kLmBuf;
  double* W = lsm + lm_panel_offset(8);
  const int64_t l = d.lmList[first + blockIdx.x];
  const int64_t o0 = d.lmObs[l], o1 = d.lmObs[l + 1];
  const int64_t cb = d.lmY[l] / 3, ncol = d.lmY[l + 1] / 3 - cb;
  for (int i = tid; i < 3 * ncol; i += 256) W[i] = 0.0;
  __syncthreads();
  double v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // v00 v10 v20 v11 v21 v22 g0 g1 g2
  lm_stage_loop(d, o0, o1 - o0, stg, W, wave, 4, lane, v);
#pragma unroll
  for (int k = 0; k < 9; k++) v[k] = wave_sum(v[k]);
  if (lane == 0)
#pragma unroll
    for (int k = 0; k < 9; k++) part[wave][k] = v[k];
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) v[k] = part[0][k] + part[1][k] + part[2][k] + part[3][k];
    basemap_add_g(d, l, v + 6), basemap_add_v(d, l, v[0], v[1], v[2], v[3], v[4], v[5]);
    bool ok;
    const Chol3 L = chol3_damped(v[0], v[1], v[2], v[3], v[4], v[5], lambda, ok);
    landmark_finish(d, l, L, ok, v + 6);
    L.store(Ls);
  }
  __syncthreads();
  panel_solve(Chol3::load(Ls), W, d.Y + d.lmY[l], ncol, tid, 256);
}

// the wide class when its panels exceed kLmBigCols: landmark_kernel's per-column path
__global__ void __launch_bounds__(256) landmark_list_kernel(Dev d, double lambda, int64_t first, int64_t n) {
  const int64_t li = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (li >= n) return;
  landmark_eliminate(d, lambda, 0, d.lmList[first + li]);
}

// a landmark with base-map factors and no visual observation (BaseMapDev::lone): V and g are its base-map
// sums, its panel is empty; one thread per landmark
__global__ void __launch_bounds__(256) landmark_lone_kernel(Dev d, double lambda) {
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= d.bm.nLone) return;
  const int64_t l = d.bm.lone[t];
  const double* b = d.bm.Vg + l * 9;
  const double g[3] = {b[6], b[7], b[8]};
  bool ok;
  const Chol3 L = chol3_damped(b[0], b[1], b[2], b[3], b[4], b[5], lambda, ok);
  landmark_finish(d, l, L, ok, g);
}

// mode 2: zNew = L^-1 gpNew, one thread per landmark
__global__ void __launch_bounds__(256) landmark_z_kernel(Dev d, int64_t lo, int64_t hi) {
  const int64_t l = lo + (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= hi) return;
  const double* g = d.gpNew + l * 3;
  double z0 = g[0], z1 = g[1], z2 = g[2];
  chol3_fwd(Chol3::load(d.Vchol + l * 6), z0, z1, z2);
  d.zNew[l * 3] = z0, d.zNew[l * 3 + 1] = z1, d.zNew[l * 3 + 2] = z2;
}

// ------------------------------------------------------------------ launch wrapper
// this handle's landmarks [lmB, lmE): mode 0 eliminates them by panel-width class, mode 1 takes the point
// gradient alone (gpNew), mode 2 solves zNew from it
void launch_landmark(const Dev& d, double lambda, int mode, hipStream_t st) {
  const int64_t n = d.lmE - d.lmB;
  if (n <= 0) return;
  if (mode == 2) {
    launchK(landmark_z_kernel, dim3(blocks(n, 256)), dim3(256), 0, st, d, d.lmB, d.lmE);
  } else if (mode == 1) {
    launchK(landmark_kernel, dim3(blocks(n, 4)), dim3(256), 0, st, d, lambda, mode, d.lmB, d.lmE);
  } else {
    if (d.nLmSmall)
      launchK(landmark_stage_kernel, dim3((unsigned)d.nLmSmall), dim3(64), lm_lds_bytes(2, kLmSmallCols), st, d, lambda,
              (int64_t)0);
    if (d.nLmBig && d.lmBigCols <= kLmBigCols)
      launchK(landmark_obs_wg_kernel, dim3((unsigned)d.nLmBig), dim3(256), lm_lds_bytes(8, d.lmBigCols), st, d, lambda,
              d.nLmSmall);
    else if (d.nLmBig)
      launchK(landmark_list_kernel, dim3(blocks(d.nLmBig, 4)), dim3(256), 0, st, d, lambda, d.nLmSmall, d.nLmBig);
    if (d.bm.nLone) hipLaunchKernelGGL(landmark_lone_kernel, dim3(blocks(d.bm.nLone, 256)), dim3(256), 0, st, d, lambda);
  }
}
}  // namespace viba
