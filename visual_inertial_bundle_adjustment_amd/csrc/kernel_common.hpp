// Device helpers shared by the Schur-assembly kernels (landmark.hip / obs_group.hip / schur.hip) and the
// factorization / solves (chol.hip / fanin.hip / trisolve.hip / step.hip): tile geometry, fp64 MFMA, DPP wave
// sums, XCD-aware block ids, LDS staging, the landmarks' 3 x 3 Cholesky.
#pragma once
#include "device_math.hpp"
#include "engine.hpp"

namespace viba {
using namespace dev;

constexpr int TS = 64;  // tile size (rows/cols of a dense reduced-system tile)
typedef double double4_t __attribute__((ext_vector_type(4)));
typedef float float4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ double4_t mfma64(double a, double b, double4_t c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
// Hessian products of the Schur complement (observation-group Gram blocks, landmark tile products) in
// the record precision: fp64 MFMA, or v_mfma_f32_16x16x4_f32 in the VIBA_MIXED build.  The two differ
// in their C/D map: f64 D row = (lane >> 4) + 4 r, f32 D row = 4 (lane >> 4) + r (column lane & 15 in
// both; A/B maps identical), so accumulator register r of lane l sits at D row kAccL4 (l >> 4) + kAccR r.
#if VIBA_MIXED
typedef float4_t hacc4_t;
__device__ __forceinline__ hacc4_t mfma_h(float a, float b, hacc4_t c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
constexpr int kAccL4 = 4, kAccR = 1;
#else
typedef double4_t hacc4_t;
__device__ __forceinline__ hacc4_t mfma_h(double a, double b, hacc4_t c) { return mfma64(a, b, c); }
constexpr int kAccL4 = 1, kAccR = 4;
#endif

__device__ inline int rv_dim(const Dev& d, int r) { return d.rvDim[r]; }

// all-lane sum: within each 16-lane row by DPP (quad swaps, then row rotations by 4 and 8), the four
// row sums by v_readlane -- VALU-local, no LDS-crossbar ds_bpermute round trips
template <int kCtrl>
__device__ __forceinline__ double dpp_f64(double x) {
  const int2 w = __builtin_bit_cast(int2, x);
  return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_update_dpp(0, w.x, kCtrl, 0xf, 0xf, false),
                                              __builtin_amdgcn_update_dpp(0, w.y, kCtrl, 0xf, 0xf, false)));
}
__device__ __forceinline__ double lane_f64(double x, int l) {
  const int2 w = __builtin_bit_cast(int2, x);
  return __builtin_bit_cast(double, make_int2(__builtin_amdgcn_readlane(w.x, l), __builtin_amdgcn_readlane(w.y, l)));
}
__device__ __forceinline__ double wave_sum(double x) {
  x += dpp_f64<0xB1>(x);   // quad_perm [1, 0, 3, 2]
  x += dpp_f64<0x4E>(x);   // quad_perm [2, 3, 0, 1]
  x += dpp_f64<0x124>(x);  // row_ror:4
  x += dpp_f64<0x128>(x);  // row_ror:8
  return (lane_f64(x, 0) + lane_f64(x, 16)) + (lane_f64(x, 32) + lane_f64(x, 48));
}

__device__ inline double* tile_ptr(const Dev& d, int64_t r, int64_t c) {
  const int32_t ti = d.tileIdx[(r / TS) * d.nT + (c / TS)];
  if (ti < 0) return nullptr;
  return d.tiles + (int64_t)ti * TS * TS + (c % TS) * TS + (r % TS);
}

// XCD-aware block id: blocks b and b + 8 share an XCD (MI355X_MICROARCH.md §Workgroup dispatch), so
// hand each XCD a contiguous range of work (bijective for any grid size)
__device__ __forceinline__ int64_t xcd_block(int64_t b, int64_t nb) {
  const int64_t q = nb / 8, r = nb % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

__device__ __forceinline__ uint64_t uniform64(uint64_t v) {
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  return ((uint64_t)hi << 32) | lo;
}

static inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

// Staging through LDS: a pointer's LDS address for inline-asm ds_ instructions, and the asynchronous
// global -> LDS copy of kBytes (16 or 4) per lane (the wave's lanes land consecutively from `lds`)
constexpr int kRecV = 16 / (int)sizeof(rec_t);  // record elements per 16 B piece
__device__ __forceinline__ uint32_t lds_addr(const void* p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) char*)p;
}
template <int kBytes>
__device__ __forceinline__ void glds(const void* global, void* lds) {
  static_assert(kBytes == 16 || kBytes == 4, "the sizes in use");  // (the builtin takes a literal size only)
  const auto* g = (const __attribute__((address_space(1))) void*)global;
  auto* s = (__attribute__((address_space(3))) void*)lds;
  if constexpr (kBytes == 16) __builtin_amdgcn_global_load_lds(g, s, 16, 0, 0);
  else __builtin_amdgcn_global_load_lds(g, s, 4, 0, 0);
}

// The lower Cholesky factor of a landmark's damped 3 x 3 block, six doubles at Vchol + 6 l in this order
struct Chol3 {
  double l00, l10, l20, l11, l21, l22;
  static __device__ __forceinline__ Chol3 load(const double* p) { return {p[0], p[1], p[2], p[3], p[4], p[5]}; }
  __device__ __forceinline__ void store(double* p) const { p[0] = l00, p[1] = l10, p[2] = l20, p[3] = l11, p[4] = l21, p[5] = l22; }
};
// of the lower triangle v with its diagonal damped (Optimizer.cpp:136-146: v (1 + lambda) + lambda);
// ok = every pivot positive (false for a NaN)
__device__ __forceinline__ Chol3 chol3_damped(double v00, double v10, double v20, double v11, double v21, double v22,
                                              double lambda, bool& ok) {
  v00 = v00 * (1.0 + lambda) + lambda, v11 = v11 * (1.0 + lambda) + lambda, v22 = v22 * (1.0 + lambda) + lambda;
  const double l00 = sqrt(v00), l10 = v10 / l00, l20 = v20 / l00;
  const double d11 = v11 - l10 * l10, l11 = sqrt(d11), l21 = (v21 - l20 * l10) / l11;
  const double d22 = v22 - l20 * l20 - l21 * l21, l22 = sqrt(d22);
  ok = v00 > 0 && d11 > 0 && d22 > 0;
  return {l00, l10, l20, l11, l21, l22};
}
// a = L^-1 a, a = L^-T a
__device__ __forceinline__ void chol3_fwd(const Chol3& L, double& a0, double& a1, double& a2) {
  a0 = a0 / L.l00, a1 = (a1 - L.l10 * a0) / L.l11, a2 = (a2 - L.l20 * a0 - L.l21 * a1) / L.l22;
}
__device__ __forceinline__ void chol3_bwd(const Chol3& L, double& a0, double& a1, double& a2) {
  a2 = a2 / L.l22, a1 = (a1 - L.l21 * a2) / L.l11, a0 = (a0 - L.l10 * a1 - L.l20 * a2) / L.l00;
}

}  // namespace viba
