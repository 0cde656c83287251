// From the reduced solution to the updated variables (gfx950): what backSubstitute and vb_apply_step launch
//   backsub_kernel         landmark back-substitution x_p = L^-T (z - Y x_c)
//   dot_kernel, axpby_kernel   reduced-vector utilities
//   boxplus_points_kernel, boxplus_reduced_kernel   applyStep, with the step-ratio statistics
#include "kernel_common.hpp"
#include <algorithm>

namespace viba {

// ------------------------------------------------------------------ point back-substitution
// points x_p = L^-T (z - Y x_c) (Optimizer.cpp:200-231, back-substitution of the eliminated point
// range; mode 0 uses z, mode 1 uses zNew): one wave per landmark, lanes over its Y panel columns
// (coalesced 24 B per lane; pcRow maps a column to its reduced row), wave reduction, lane 0 solves the
// 3 x 3 system
__global__ void __launch_bounds__(256) backsub_kernel(Dev d, int mode, int64_t lo, int64_t hi, const double* xr,
                                                      double* xp) {
  const int lane = threadIdx.x & 63;
  const int64_t l = lo + (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (l >= hi) return;
  const int64_t cb = d.lmY[l] / 3, ncol = d.lmY[l + 1] / 3 - cb;
  const rec_t* Y = d.Y + 3 * cb;  // plane-interleaved: plane q of column c at Y[3 c + q]
  double t0 = 0, t1 = 0, t2 = 0;
  // two columns per lane and step: both row-index loads, then both gathers of x, in flight together
  for (int64_t c = lane; c < ncol; c += 128) {
    const bool two = c + 64 < ncol;
    const int32_t ra = d.pcRow[cb + c], rb = two ? d.pcRow[cb + c + 64] : ra;
    const double ya0 = Y[3 * c], ya1 = Y[3 * c + 1], ya2 = Y[3 * c + 2];
    const double yb0 = two ? (double)Y[3 * (c + 64)] : 0.0, yb1 = two ? (double)Y[3 * (c + 64) + 1] : 0.0;
    const double yb2 = two ? (double)Y[3 * (c + 64) + 2] : 0.0;
    const double va = xr[ra], vb = xr[rb];
    t0 += ya0 * va + yb0 * vb, t1 += ya1 * va + yb1 * vb, t2 += ya2 * va + yb2 * vb;
  }
  t0 = wave_sum(t0), t1 = wave_sum(t1), t2 = wave_sum(t2);
  if (lane != 0) return;
  const double* zz = mode ? d.zNew : d.z;
  t0 = zz[l * 3] - t0, t1 = zz[l * 3 + 1] - t1, t2 = zz[l * 3 + 2] - t2;
  chol3_bwd(Chol3::load(d.Vchol + l * 6), t0, t1, t2);
  xp[l * 3] = t0, xp[l * 3 + 1] = t1, xp[l * 3 + 2] = t2;
}

// ------------------------------------------------------------------ vector utilities
__global__ void dot_kernel(const double* a, const double* b, int64_t n, double* out) {
  double s = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    s += a[i] * b[i];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  __shared__ double sh[4];
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0;
    for (int w = 0; w < (int)((blockDim.x + 63) >> 6); w++) t += sh[w];
    atomicAdd(out, t);
  }
}
__global__ void axpby_kernel(double* y, const double* x, double a, double b, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    y[i] = (b == 0.0) ? a * x[i] : a * x[i] + b * y[i];
}

// ------------------------------------------------------------------ box-plus (applyStep)
// red[8] = max ratio (as uint64 bits), red[9] = sum r^2, red[10] = sum r
__device__ void ratio_accum(const Dev& d, double r) {
  double s2 = r * r, s1 = r;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s2 += __shfl_down(s2, off, 64);
    s1 += __shfl_down(s1, off, 64);
    r = fmax(r, __shfl_down(r, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax((unsigned long long*)(d.red + 8), (unsigned long long)__double_as_longlong(r));
    atomicAdd(d.red + 9, s2);
    atomicAdd(d.red + 10, s1);
  }
}

// grid-stride over the points, the step ratios reduced per block (one set of atomics per block: one
// per wave on the same three words serialised in L2, 0.18 ms for 300k points)
__global__ void __launch_bounds__(256) boxplus_points_kernel(Dev d, const double* stepPt) {
  __shared__ double red[3][4];
  double rmax = 0.0, s1 = 0.0, s2 = 0.0;
  for (int64_t h = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; h < d.nvar[0]; h += (int64_t)gridDim.x * blockDim.x) {
    const int l = d.ptLm[h];
    if (l >= d.lmB && l < d.lmE) {
      double* v = d.var[0] + h * 3;
      const double* s = stepPt + (int64_t)l * 3;
      v[0] += s[0], v[1] += s[1], v[2] += s[2];
      const double sn = fmax(fabs(s[0]), fmax(fabs(s[1]), fabs(s[2])));
      const double vn = fmax(fabs(v[0]), fmax(fabs(v[1]), fabs(v[2])));
      const double r = sn / (1.0 + vn);
      rmax = fmax(rmax, r), s1 += r, s2 += r * r;
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    s2 += __shfl_down(s2, off, 64);
    s1 += __shfl_down(s1, off, 64);
    rmax = fmax(rmax, __shfl_down(rmax, off, 64));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) red[0][wave] = rmax, red[1][wave] = s1, red[2][wave] = s2;
  __syncthreads();
  if (threadIdx.x == 0) {
    rmax = fmax(fmax(red[0][0], red[0][1]), fmax(red[0][2], red[0][3]));
    atomicMax((unsigned long long*)(d.red + 8), (unsigned long long)__double_as_longlong(rmax));
    atomicAdd(d.red + 9, red[2][0] + red[2][1] + red[2][2] + red[2][3]);
    atomicAdd(d.red + 10, red[1][0] + red[1][1] + red[1][2] + red[1][3]);
  }
}

__global__ void __launch_bounds__(256) boxplus_reduced_kernel(Dev d, const double* stepRed) {
  const int X = blockIdx.x * blockDim.x + threadIdx.x;
  double r = 0.0;
  if (X < d.nRV) {  // every shard applies the (identical) reduced step; only the root counts it
    const int kind = d.rvKind[X], h = d.rvHandle[X];
    const double* s = stepRed + d.rvOff[X];
    if (kind == 2 || kind == 3) {  // Vec3 (Variable.h:33-37)
      double* v = d.var[kind] + (int64_t)h * 3;
      v[0] += s[0], v[1] += s[1], v[2] += s[2];
      const double sn = fmax(fabs(s[0]), fmax(fabs(s[1]), fabs(s[2])));
      const double vn = fmax(fabs(v[0]), fmax(fabs(v[1]), fabs(v[2])));
      r = sn / (1.0 + vn);
    } else if (kind == 1 || kind == 5 || kind == 7) {  // SE3: exp(step) * value (Variable.h:104-110)
      double* v = d.var[kind] + (int64_t)h * 7;
      se3 T = se3_mul(se3_exp(s), se3_load(v));
      se3_store(T, v);
      const double un = fmax(fabs(s[0]), fmax(fabs(s[1]), fabs(s[2])));
      const double rn = fmax(fabs(s[3]), fmax(fabs(s[4]), fabs(s[5])));
      const double tn = fmax(fabs(T.t.x), fmax(fabs(T.t.y), fabs(T.t.z)));
      r = fmax(rn, un / (1.0 + tn));
    } else if (kind == 4) {  // CameraModelParam.cpp:54-67
      double* c = d.var[4] + (int64_t)h * 24;
      int n = (int)c[1];
      const int td = d.rvDim[X];
      for (int i = 0; i < n; i++) c[9 + i] += s[i];
      if (c[7] != 0.0) {
        const double ro = c[4] != 0.0 ? c[5] : 0.0;
        c[5] = ro + s[n++];
        c[4] = 1.0;
      }
      if (c[8] != 0.0) c[6] += s[n++];
      for (int i = 0; i < td; i++) r = fmax(r, fabs(s[i]));
    } else if (kind == 6) {  // ImuCalibParam::boxPlus (ImuCalibParam.cpp:55-116)
      double* m = d.var[6] + (int64_t)h * 32;
      const ImuIdx& J = d.jac;
      if (J.gB >= 0) for (int i = 0; i < 3; i++) m[6 + i] += s[J.gB + i];
      if (J.aB >= 0) for (int i = 0; i < 3; i++) m[9 + i] += s[J.aB + i];
      if (J.gS >= 0) for (int i = 0; i < 3; i++) m[i] = 1.0 / (1.0 / m[i] + s[J.gS + i]);
      if (J.aS >= 0) for (int i = 0; i < 3; i++) m[3 + i] = 1.0 / (1.0 / m[3 + i] + s[J.aS + i]);
      if (J.gN >= 0) {
        double* g = m + 12;  // col-major (i, j) -> 3 j + i
        g[3] += s[J.gN], g[6] += s[J.gN + 1], g[1] += s[J.gN + 2];
        g[7] += s[J.gN + 3], g[2] += s[J.gN + 4], g[5] += s[J.gN + 5];
        g[0] = sqrt(1.0 - (g[3] * g[3] + g[6] * g[6]));
        g[4] = sqrt(1.0 - g[1] * g[1] - g[7] * g[7]);
        g[8] = sqrt(1.0 - (g[2] * g[2] + g[5] * g[5]));
      }
      if (J.aN >= 0) {
        double* a = m + 21;
        a[3] += s[J.aN], a[6] += s[J.aN + 1], a[7] += s[J.aN + 2];
        a[0] = sqrt(1.0 - (a[3] * a[3] + a[6] * a[6]));
        a[4] = sqrt(1.0 - a[7] * a[7]);
        a[8] = 1.0;
      }
      if (J.rT >= 0) m[31] += s[J.rT], m[30] += s[J.rT];
      if (J.gaT >= 0) m[30] += s[J.gaT];
      for (int i = 0; i < J.size; i++) r = fmax(r, fabs(s[i]));
    }
  }
  ratio_accum(d, d.root ? r : 0.0);
}

// ------------------------------------------------------------------ launch wrappers
void launch_backsub(const Dev& d, int mode, int64_t lo, int64_t hi, const double* xr, double* xp, hipStream_t st) {
  if (hi > lo)
    launchK(backsub_kernel, dim3(blocks(hi - lo, 4)), dim3(256), 0, st, d, mode, lo, hi, xr, xp);
}
void launch_dot(const double* a, const double* b, int64_t n, double* out, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(dot_kernel, dim3((unsigned)std::min<int64_t>(1024, blocks(n, 256))), dim3(256), 0, st, a, b,
                       n, out);
}
void launch_axpby(double* y, const double* x, double a, double b, int64_t n, hipStream_t st) {
  if (n > 0)
    hipLaunchKernelGGL(axpby_kernel, dim3((unsigned)std::min<int64_t>(4096, blocks(n, 256))), dim3(256), 0, st, y,
                       x, a, b, n);
}
void launch_boxplus(const Dev& d, const double* stepRed, const double* stepPt, hipStream_t st) {
  if (d.nvar[0])
    hipLaunchKernelGGL(boxplus_points_kernel, dim3((unsigned)std::min<int64_t>(blocks(d.nvar[0], 256), 256)), dim3(256), 0, st, d,
                       stepPt);
  if (d.nRV) hipLaunchKernelGGL(boxplus_reduced_kernel, dim3(blocks(d.nRV, 256)), dim3(256), 0, st, d, stepRed);
}

}  // namespace viba
