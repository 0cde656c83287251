// Per-lane pieces of the initial landmark triangulation (triangulate.hip), usable from host code as well:
// tests/cpp/triang_check.cpp compiles this header alone and checks it against the standard library.
//
//   Mt19937 / bounded_draw   std::mt19937 + std::uniform_int_distribution<int> as findTriangulationCandidate
//                            uses them (Triangulation.cpp:40-47), bit for bit
//   unproject                CameraCalibration::unprojectNoChecks, as csrc/session.cpp states it
//   pair_candidate           the two-ray midpoint of findTriangulationCandidate (Triangulation.cpp:48-66)
//   ray_angle                the angle between a ray and the direction to a candidate (:70-72)
//
// Nothing here needs a wave, shared memory or the engine's headers.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace viba {
namespace triang {

#define TRI_HD __host__ __device__ inline

struct V3 {
  double x, y, z;
};
TRI_HD V3 add3(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
TRI_HD V3 sub3(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
TRI_HD V3 scl3(double s, V3 a) { return {s * a.x, s * a.y, s * a.z}; }
TRI_HD double dot3(V3 a, V3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
TRI_HD V3 cross3(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
TRI_HD double norm3(V3 a) { return sqrt(dot3(a, a)); }

// Triangulation.h constants
constexpr int kNumRansac = 10;
constexpr double kOutlierObservationRads = 0.4 * 3.14159265358979323846 / 180.0;
constexpr int kMinNumInliersInTriangulation = 2;
constexpr int kMinInlierObs = 3;
constexpr int kMinNumInliersAfterRefinement = 3;

// ------------------------------------------------------------------ std::mt19937
// The state lives in caller memory (624 words: an array on the host, shared memory on the device).  The
// twist is done one word per draw, in index order: word i is regenerated from words i, i + 1 and i + 397
// (mod 624) just before it is tempered, which reads and writes exactly what the standard's whole-state
// twist reads and writes for that word, so any number of draws follows the standard sequence.
constexpr int kMtN = 624, kMtM = 397;

struct Mt19937 {
  uint32_t* s;
  int i;
};

// std::mt19937 mt(int seed): the seed is reduced mod 2^32
TRI_HD void mt_seed(Mt19937& g, uint32_t* state, int32_t seed) {
  g.s = state, g.i = 0;
  uint32_t x = (uint32_t)seed;
  state[0] = x;
  for (int k = 1; k < kMtN; k++) {
    x = 1812433253u * (x ^ (x >> 30)) + (uint32_t)k;
    state[k] = x;
  }
}

TRI_HD uint32_t mt_next(Mt19937& g) {
  const int i = g.i, i1 = i + 1 < kMtN ? i + 1 : 0, im = i + kMtM < kMtN ? i + kMtM : i + kMtM - kMtN;
  const uint32_t y = (g.s[i] & 0x80000000u) | (g.s[i1] & 0x7fffffffu);
  uint32_t z = g.s[im] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  g.s[i] = z;
  g.i = i1;
  z ^= z >> 11;
  z ^= (z << 7) & 0x9d2c5680u;
  z ^= (z << 15) & 0xefc60000u;
  z ^= z >> 18;
  return z;
}

// std::uniform_int_distribution<int>(lo, hi)(mt) as libstdc++ (GCC 11, bits/uniform_int_dist.h) evaluates
// it for a 32-bit generator: Lemire's nearly divisionless method, _S_nd<uint64_t>.  hi - lo + 1 < 2^32.
TRI_HD int32_t bounded_draw(Mt19937& g, int32_t lo, int32_t hi) {
  const uint32_t range = (uint32_t)hi - (uint32_t)lo + 1u;
  uint64_t product = (uint64_t)mt_next(g) * (uint64_t)range;
  uint32_t low = (uint32_t)product;
  if (low < range) {
    const uint32_t threshold = (0u - range) % range;
    while (low < threshold) {
      product = (uint64_t)mt_next(g) * (uint64_t)range;
      low = (uint32_t)product;
    }
  }
  return (int32_t)((uint32_t)(product >> 32) + (uint32_t)lo);
}

// one RANSAC iteration's pair of n rays (Triangulation.cpp:46-47): a in [0, n - 1], b = (a + offset) % n
// with offset in [1, n - 1]
TRI_HD void draw_pair(Mt19937& g, int32_t n, int32_t& a, int32_t& b) {
  a = bounded_draw(g, 0, n - 1);
  const int32_t off = bounded_draw(g, 1, n - 1);
  b = (int32_t)(((int64_t)a + off) % n);
}

// ------------------------------------------------------------------ unprojection
// unprojectNoChecks (projectaria_tools FisheyeRadTanThinPrism::unproject, published algorithm), as
// csrc/session.cpp: undo the tangential + thin-prism terms by Newton on (xr, yr), then invert
// r_d = theta R(theta) by Newton; the ray is (xr, yr) tan(theta) / r_d, 1.
// Linear: ((u - cx) / fx, (v - cy) / fy, 1).  cam: camera record (include/viba_hip.h VB_CAM_DATA)
TRI_HD V3 unproject(const double* cam, double u, double v) {
  const double* p = cam + 9;
  if (cam[0] == 0.0) return {(u - p[2]) / p[0], (v - p[3]) / p[1], 1.0};
  const double f = p[0], p0 = p[9], p1 = p[10];
  const double ud = (u - p[1]) / f, vd = (v - p[2]) / f;
  double xr = ud, yr = vd;
  for (int it = 0; it < 50; it++) {
    const double rr2 = xr * xr + yr * yr, rr4 = rr2 * rr2, tmp = 2.0 * (xr * p0 + yr * p1);
    const double eu = xr + tmp * xr + rr2 * p0 + p[11] * rr2 + p[12] * rr4 - ud;
    const double ev = yr + tmp * yr + rr2 * p1 + p[13] * rr2 + p[14] * rr4 - vd;
    const double a0 = p[11] + 2.0 * p[12] * rr2, a1 = p[13] + 2.0 * p[14] * rr2;
    const double D00 = 1.0 + 6.0 * xr * p0 + 2.0 * yr * p1 + 2.0 * xr * a0;
    const double D01 = 2.0 * p1 * xr + 2.0 * yr * p0 + 2.0 * yr * a0;
    const double D10 = 2.0 * p0 * yr + 2.0 * xr * p1 + 2.0 * xr * a1;
    const double D11 = 1.0 + 2.0 * xr * p0 + 6.0 * yr * p1 + 2.0 * yr * a1;
    const double det = D00 * D11 - D01 * D10;
    const double sx = (D11 * eu - D01 * ev) / det, sy = (-D10 * eu + D00 * ev) / det;
    xr -= sx, yr -= sy;
    if (sx * sx + sy * sy < 1e-24) break;
  }
  const double rd = sqrt(xr * xr + yr * yr);
  if (rd < 1e-12) return {xr, yr, 1.0};
  double th = rd;
  for (int it = 0; it < 50; it++) {
    const double th2 = th * th;
    double R = 1.0, dR = 0.0, t2 = th2;
    for (int i = 0; i < 6; i++) R += p[3 + i] * t2, dR += p[3 + i] * (2.0 * (i + 1) + 1.0) * t2, t2 *= th2;
    const double step = (th * R - rd) / (1.0 + dR);  // d(th R)/dth = 1 + sum (2i+3) k_i th^(2i+2)
    th -= step;
    if (fabs(step) < 1e-15) break;
  }
  const double s = tan(th) / rd;
  return {xr * s, yr * s, 1.0};
}

// ------------------------------------------------------------------ rays and candidates
struct Ray {
  V3 s, d;  // camera centre and unit direction, world frame
};

// the ray of an observation: T_cam_world row (qx qy qz qw tx ty tz), camera record, pixel
// (T_world_cam.translation(), T_world_cam.so3() * unproject(uv).normalized(); Triangulation.cpp:176-190)
TRI_HD Ray observation_ray(const double* Tcw, const double* cam, double u, double v) {
  const double x = Tcw[0], y = Tcw[1], z = Tcw[2], w = Tcw[3];
  const double R00 = 1 - 2 * (y * y + z * z), R01 = 2 * (x * y - z * w), R02 = 2 * (x * z + y * w);
  const double R10 = 2 * (x * y + z * w), R11 = 1 - 2 * (x * x + z * z), R12 = 2 * (y * z - x * w);
  const double R20 = 2 * (x * z - y * w), R21 = 2 * (y * z + x * w), R22 = 1 - 2 * (x * x + y * y);
  const V3 t = {Tcw[4], Tcw[5], Tcw[6]};
  const V3 r = unproject(cam, u, v);
  const V3 n = scl3(1.0 / norm3(r), r);
  Ray o;
  o.d = {R00 * n.x + R10 * n.y + R20 * n.z, R01 * n.x + R11 * n.y + R21 * n.z, R02 * n.x + R12 * n.y + R22 * n.z};
  o.s = {-(R00 * t.x + R10 * t.y + R20 * t.z), -(R01 * t.x + R11 * t.y + R21 * t.z),
         -(R02 * t.x + R12 * t.y + R22 * t.z)};
  return o;
}

// the candidate of a pair of rays: false when the rays are (nearly) parallel (|ortho| < 1e-4) or the
// closest approach lies behind either camera (aFact or bFact negative)
TRI_HD bool pair_candidate(const Ray& a, const Ray& b, V3& cand) {
  const V3 ortho = cross3(a.d, b.d);
  const double on = norm3(ortho);
  if (on < 1e-4) return false;
  const V3 o = scl3(1.0 / on, ortho);
  const V3 aLat = cross3(o, a.d), bLat = cross3(o, b.d);
  const double bFact = dot3(aLat, sub3(a.s, b.s)) / dot3(aLat, b.d);
  const double aFact = dot3(bLat, sub3(b.s, a.s)) / dot3(bLat, a.d);
  if (bFact < 0.0 || aFact < 0.0) return false;
  cand = add3(add3(a.s, scl3(aFact, a.d)), scl3(0.5 * dot3(o, sub3(b.s, a.s)), o));
  return true;
}

// angle between ray r and the direction from its centre to cand
TRI_HD double ray_angle(const Ray& r, V3 cand) {
  const V3 v = sub3(cand, r.s);
  const V3 alt = scl3(1.0 / norm3(v), v);
  return 2.0 * asin(norm3(sub3(r.d, alt)) * 0.5);
}

// HuberLoss::jet2 (lib/small_thing/SoftLoss.h:64-113): the derivative
TRI_HD double huber_der(double a, double s) { return s > a * a ? a / sqrt(s) : 1.0; }

}  // namespace triang
}  // namespace viba
