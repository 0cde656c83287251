// Residual report (vb_factor_errors / vb_error_histogram): what the report kernels of visual.hip / small.hip (the
// factor evaluations live there) and report.hip (the generic binning, the C-ABI) share.
#pragma once
#include "engine.hpp"

namespace viba {

// caps of one histogram request: a workgroup's bin table [group][bin] of 32-bit counts is
// 64 x 33 x 4 B = 8448 B of LDS (RepTable, 9.8 KB with the per-group words and the edges)
constexpr int kRepMaxGroups = 64, kRepMaxEdges = 32;

// per-factor outputs of rows [first, first + n) of a kind (any pointer may be null); raw has the kind's
// vb_factor_error_size doubles per row
struct RepRows {
  int64_t first = 0, n = 0;
  double *raw = nullptr, *squ = nullptr, *sqw = nullptr, *cost = nullptr;
  uint8_t* valid = nullptr;
};

// one histogram request; all pointers are device memory
struct RepHist {
  int32_t which = 0, nGroups = 1, nEdges = 0;
  const uint8_t* grp = nullptr;  // group of every item in the kernel's item order (nullptr: group 0)
  const double* edges = nullptr;
  unsigned long long* counts = nullptr;    // nGroups x (nEdges + 1)
  double* cost = nullptr;                  // nGroups
  unsigned long long* nFactors = nullptr;  // nGroups
  unsigned long long* nFailing = nullptr;  // nGroups
};

// a workgroup's partial histogram in LDS
struct RepTable {
  uint32_t cnt[kRepMaxGroups * (kRepMaxEdges + 1)];
  uint32_t nFactors[kRepMaxGroups], nFailing[kRepMaxGroups];
  double cost[kRepMaxGroups];
  double edges[kRepMaxEdges];
};

#ifdef __HIPCC__
__device__ __forceinline__ void rep_clear(RepTable& t, const RepHist& H) {
  const int nb = H.nGroups * (H.nEdges + 1);
  for (int i = threadIdx.x; i < nb; i += blockDim.x) t.cnt[i] = 0;
  for (int i = threadIdx.x; i < H.nGroups; i += blockDim.x) t.nFactors[i] = 0, t.nFailing[i] = 0, t.cost[i] = 0.0;
  for (int i = threadIdx.x; i < H.nEdges; i += blockDim.x) t.edges[i] = H.edges[i];
  __syncthreads();
}
// one factor of group g: counted; binned with its cost unless it fails (Histograms.cpp:206-212).  The bin
// is the number of edges <= value, as Histogram.cpp:18-22 (std::upper_bound).
__device__ __forceinline__ void rep_add(RepTable& t, const RepHist& H, int g, bool ok, double value, double cost) {
  atomicAdd(&t.nFactors[g], 1u);
  if (!ok) {
    atomicAdd(&t.nFailing[g], 1u);
    return;
  }
  int bin = 0;
  for (int e = 0; e < H.nEdges; e++) bin += t.edges[e] <= value ? 1 : 0;
  atomicAdd(&t.cnt[g * (H.nEdges + 1) + bin], 1u);
  if (cost != 0.0) atomicAdd(&t.cost[g], cost);
}
// the workgroup's non-zero entries into the global result: 64-bit integer atomics (exact in any order)
// and one fp64 add per group with a cost
__device__ __forceinline__ void rep_flush(RepTable& t, const RepHist& H) {
  __syncthreads();
  const int nb = H.nGroups * (H.nEdges + 1);
  for (int i = threadIdx.x; i < nb; i += blockDim.x)
    if (t.cnt[i]) atomicAdd(H.counts + i, (unsigned long long)t.cnt[i]);
  for (int i = threadIdx.x; i < H.nGroups; i += blockDim.x) {
    if (t.nFactors[i]) atomicAdd(H.nFactors + i, (unsigned long long)t.nFactors[i]);
    if (t.nFailing[i]) atomicAdd(H.nFailing + i, (unsigned long long)t.nFailing[i]);
    if (t.cost[i] != 0.0) atomicAdd(H.cost + i, t.cost[i]);
  }
}
#endif

// visual.hip / small.hip
// visual kind: rows R of vb_add_factors order (posOfRow: row -> position of obCostOrder) ...
void launch_visual_rows(const Dev& d, const int32_t* posOfRow, const RepRows& R, int32_t* err, hipStream_t st);
// ... or the histogram of all observations in obCostOrder (H.grp by position); err: bit 1 = a rolling-
// shutter lookup out of range
void launch_visual_hist(const Dev& d, const RepHist& H, int32_t* err, int blocks, hipStream_t st);
// small kinds 1..13: rows R of kind fk (R.valid is not written: they never fail)
void launch_small_rows(const Dev& d, int fk, const RepRows& R, hipStream_t st);
// basemap.hip: rows R of vb_add_basemap_factors order (R.sqw is not written: equal to R.squ), or the one-group
// histogram of all base-map factors
void launch_basemap_rows(const Dev& d, const RepRows& R, hipStream_t st);
void launch_basemap_hist(const Dev& d, const RepHist& H, int blocks, hipStream_t st);

}  // namespace viba
