// Triangular solves with the tile Cholesky factor (gfx950), one persistent launch per direction:
//   fwd_fanout_kernel     y = L^-1 b, fan-out over a topologically ordered task list
//   bwd_fanout_kernel     x = L^-T y, the same over the rows descending
//   set_ready_kernel      marks the rows another rank already solved (partitioned backward pass)
#include "kernel_common.hpp"

namespace viba {

// ------------------------------------------------------------------ persistent triangular solves
// One launch per direction (instead of one per tile column).  G resident workgroups; workgroup w owns
// the tile rows J = w, w + G, .. (forward) or nT-1-w, nT-1-w-G, .. (backward) and processes them in
// order, so every dependency is on a row an earlier-or-concurrent workgroup owns: no deadlock while
// all G workgroups are resident (G <= CUs, 1 workgroup per CU).  Hand-off of a solved 64-vector
// (MI355X_MICROARCH.md / cdna_hip_programming.md §6 Guideline 16, R1): the producer stores the payload
// write-through (agent-scope relaxed atomic stores = global_store ... sc1), drains (s_waitcnt
// vmcnt(0)), then one lane sets the flag (agent-scope atomic store); consumers poll the flag relaxed
// with s_sleep and read the payload with sc1 loads only (never plain / flat loads of it).  Flags are
// zeroed by a memset before every launch; spins are bounded (error flag 16 on timeout).
typedef __attribute__((address_space(1))) double gdouble;
typedef __attribute__((address_space(1))) unsigned int guint;

__device__ __forceinline__ double ld_sc1(const double* p) {
  return __hip_atomic_load((gdouble*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_sc1(double* p, double v) {
  __hip_atomic_store((gdouble*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// one wave waits until flag == 1; returns false on timeout
__device__ __forceinline__ bool wait_flag(unsigned* flag, int lane, int32_t* err) {
  unsigned v = 0;
  if (lane == 0) {
    for (unsigned spins = 0;; spins++) {
      v = __hip_atomic_load((guint*)flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v == 1u || spins > (1u << 24)) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (v != 1u) atomicOr(err, 16);
  }
  v = (unsigned)__builtin_amdgcn_readlane((int)v, 0);  // lane 0 polled
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // keep the payload loads below the poll
  return v == 1u;
}
__device__ __forceinline__ void publish(double* dst, double v, bool valid, unsigned* flag, int lane) {
  if (valid) st_sc1(dst, v);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_store((guint*)flag, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Fan-out (right-looking) triangular solves, one persistent launch per direction.  Every wave walks
// its share of a task list in topological order (task t -> wave t mod W):
//   forward, per column K ascending: [diag K: wait until the cnt[K] = rows(K) updates of b_K landed,
//     y_K = Linv_KK b_K, publish y_K + ready[K]] then one task per off-diagonal tile (I, K):
//     wait ready[K], b_I -= L_IK y_K (agent-scope fp64 atomics), cnt[I] += 1
//   backward, per row J descending: [diag J: wait cnt[J] = (off-diagonal tiles of column J),
//     x_J = Linv_JJ^T y_J, publish] then per tile (J, K) of row J: wait ready[J], y_K -= L_JK^T x_J
// A task waits only on tasks with smaller indices, so the smallest unfinished task can always run
// (no deadlock with every wave resident: the grid is one workgroup per CU).  Tile operands are loaded
// before the wait.  The critical path is the elimination-tree depth (~110 levels at config C), not
// the longest row: a separator column's hundreds of row tiles are spread over all waves.
// Hand-offs follow the guide's G16 recipe: payload by sc1 stores / agent atomics, s_waitcnt
// vmcnt(0), then the flag or counter; consumers poll, then read the payload with sc1 loads.
__device__ __forceinline__ bool wait_count(unsigned* c, unsigned expect, int lane, int32_t* err) {
  unsigned v = 0;
  if (lane == 0) {
    for (unsigned spins = 0;; spins++) {
      v = __hip_atomic_load((guint*)c, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (v >= expect || spins > (1u << 24)) break;
      __builtin_amdgcn_s_sleep(2);
    }
    if (v < expect) atomicOr(err, 16);
  }
  v = (unsigned)__builtin_amdgcn_readlane((int)v, 0);  // lane 0 polled
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return v >= expect;
}
__device__ __forceinline__ void count_up(unsigned* c, int lane) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (lane == 0) __hip_atomic_fetch_add((guint*)c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add_agent(double* p, double v) {
  __hip_atomic_fetch_add((gdouble*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// lane r's value of x in every lane (r a compile-time constant in the unrolled GEMVs): two
// v_readlane_b32 into SGPRs, the FMA then reads the scalar operand -- no LDS crossbar round trip
__device__ __forceinline__ double bcast_lane(double x, int r) {
  const int2 w = __builtin_bit_cast(int2, x);
  return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(w.x, r), __builtin_amdgcn_readlane(w.y, r)));
}

__global__ void __launch_bounds__(256) fwd_fanout_kernel(Dev d, const int32_t* tasks, int64_t nTask,
                                                         const int32_t* colTiles, const int32_t* colRows,
                                                         const int32_t* expect, const double* linv, double* b,
                                                         double* y, unsigned* ready, unsigned* cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nTask; t += W) {
    const int K = tasks[2 * t], c = tasks[2 * t + 1];
    if (c < 0) {
      const double* Li = linv + (int64_t)K * TS * TS;
      double a[TS];
#pragma unroll
      for (int q = 0; q < TS; q++) a[q] = Li[q * TS + lane];
      if (!wait_count(cnt + K, (unsigned)expect[K], lane, d.err)) return;
      const int64_t row = (int64_t)K * TS + lane;
      const double bk = ld_sc1(b + row);
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < TS; q++) v += a[q] * bcast_lane(bk, q);
      publish(y + row, row < d.nRed ? v : 0.0, true, ready + K, lane);
    } else {
      const int I = colRows[c];
      const double* A = d.tiles + (int64_t)colTiles[c] * TS * TS;
      double a[TS];
#pragma unroll
      for (int q = 0; q < TS; q++) a[q] = A[q * TS + lane];  // L(I row lane, K col q)
      if (!wait_flag(ready + K, lane, d.err)) return;
      const double yk = ld_sc1(y + (int64_t)K * TS + lane);
      double v = 0.0;
#pragma unroll
      for (int q = 0; q < TS; q++) v += a[q] * bcast_lane(yk, q);
      add_agent(b + (int64_t)I * TS + lane, -v);
      count_up(cnt + I, lane);
    }
  }
}

__global__ void __launch_bounds__(256) bwd_fanout_kernel(Dev d, const int32_t* tasks, int64_t nTask,
                                                         const int32_t* rowTiles, const int32_t* rowCol,
                                                         const int32_t* expect, const double* linv, double* yv,
                                                         double* x, unsigned* ready, unsigned* cnt) {
  const int lane = threadIdx.x & 63;
  const int64_t W = (int64_t)gridDim.x * 4;
  for (int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); t < nTask; t += W) {
    const int J = tasks[2 * t], c = tasks[2 * t + 1];
    if (c < 0) {
      const double* Li = linv + (int64_t)J * TS * TS;
      double a[TS];
#pragma unroll
      for (int r = 0; r < TS; r++) a[r] = Li[lane * TS + r];  // Linv^T
      if (!wait_count(cnt + J, (unsigned)expect[J], lane, d.err)) return;
      const int64_t row = (int64_t)J * TS + lane;
      const double tj = ld_sc1(yv + row);
      double v = 0.0;
#pragma unroll
      for (int r = 0; r < TS; r++) v += a[r] * bcast_lane(tj, r);
      publish(x + row, row < d.nRed ? v : 0.0, true, ready + J, lane);
    } else {
      const int K = rowCol[c];
      const double* A = d.tiles + (int64_t)rowTiles[c] * TS * TS;  // tile (J, K): A[q * TS + r] = L(r, q)
      double a[TS];
#pragma unroll
      for (int r = 0; r < TS; r++) a[r] = A[lane * TS + r];  // lane = column q of K
      if (!wait_flag(ready + J, lane, d.err)) return;
      const double xj = ld_sc1(x + (int64_t)J * TS + lane);
      double v = 0.0;
#pragma unroll
      for (int r = 0; r < TS; r++) v += a[r] * bcast_lane(xj, r);
      add_agent(yv + (int64_t)K * TS + lane, -v);
      count_up(cnt + K, lane);
    }
  }
}

__global__ void set_ready_kernel(const int32_t* rows, int64_t n, unsigned* ready) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) ready[rows[i]] = 1u;
}
// rhs b (clobbered), y (clobbered) -> x; flags: 4 nT words (ready / count, forward and backward).
// phases: bit 0 forward, bit 1 backward.  pre[0..nPre): rows whose x is already in x (the backward
// pass of a partitioned solve: ROOT rows solved on rank 0), marked ready before the backward pass.
void launch_solve_fanout(const Dev& d, const int32_t* tasksF, int64_t nF, const int32_t* tasksB, int64_t nB,
                         const int32_t* expF, const int32_t* expB, const int32_t* colTiles, const int32_t* colRows,
                         const int32_t* rowTiles, const int32_t* rowCol, const double* linv, double* b, double* y,
                         double* x, unsigned* flags, int G, hipStream_t st, int phases, const int32_t* pre,
                         int64_t nPre) {
  if (phases & 1) {
    (void)hipMemsetAsync(flags, 0, 2 * (size_t)d.nT * sizeof(unsigned), st);
    if (nF > 0)
      launchK(fwd_fanout_kernel, dim3(G), dim3(256), 0, st, d, tasksF, nF, colTiles, colRows, expF, linv, b, y,
              flags, flags + d.nT);
  }
  if (phases & 2) {
    (void)hipMemsetAsync(flags + 2 * d.nT, 0, 2 * (size_t)d.nT * sizeof(unsigned), st);
    if (nPre > 0) hipLaunchKernelGGL(set_ready_kernel, dim3((unsigned)((nPre + 255) / 256)), dim3(256), 0, st, pre, nPre, flags + 2 * d.nT);
    if (nB > 0)
      launchK(bwd_fanout_kernel, dim3(G), dim3(256), 0, st, d, tasksB, nB, rowTiles, rowCol, expB, linv, y, x,
              flags + 2 * d.nT, flags + 3 * d.nT);
  }
}

}  // namespace viba
