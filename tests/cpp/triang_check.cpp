// Host-side check of csrc/triang_core.hpp, the per-lane pieces of the device triangulation
// (tests/test_triangulate.py builds this as host code under AddressSanitizer and UBSan and runs it).
//
//   1. Mt19937 / bounded_draw / draw_pair against std::mt19937 + std::uniform_int_distribution<int>: every
//      value equal, over seeds, ranges (one where the redraw loop fires on about half the draws) and enough
//      draws to cross the state twist several times.
//   2. unproject against a file of (camera record, camera point, projected pixel) cases:
//      unproject(uv) = pc / pc.z within 1e-9.
//
// usage: triang_check CASES      exit 0 when everything holds, 1 with the failed property on stderr.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../visual_inertial_bundle_adjustment_amd/csrc/triang_core.hpp"

using namespace viba::triang;

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::fprintf(stderr, "FAILED: " __VA_ARGS__); \
      std::fprintf(stderr, "\n");              \
      if (++failures > 20) std::exit(1);       \
    }                                          \
  } while (0)

static void check_generator() {
  std::vector<int32_t> seeds = {0, 1, 1729, 0x7fffffff, -1 /* 0xffffffff */};
  std::mt19937_64 pick(20240229);
  for (int i = 0; i < 200; i++) seeds.push_back((int32_t)(uint32_t)pick());
  const int32_t ranges[] = {2, 3, 5, 64, 65, 1000, 3 * (1 << 29)};
  constexpr int kDraws = 2000;
  uint32_t state[kMtN];
  long redraw_probe = 0;
  for (int32_t seed : seeds) {
    {  // the raw generator
      std::mt19937 ref(seed);
      Mt19937 g;
      mt_seed(g, state, seed);
      for (int k = 0; k < kDraws; k++) {
        const uint32_t want = (uint32_t)ref(), got = mt_next(g);
        CHECK(want == got, "mt19937 seed %d draw %d: %u != %u", seed, k, got, want);
      }
    }
    for (int32_t range : ranges) {
      std::mt19937 ref(seed);
      std::uniform_int_distribution<int> d0(0, range - 1);
      Mt19937 g;
      mt_seed(g, state, seed);
      for (int k = 0; k < kDraws; k++) {
        const int want = d0(ref), got = bounded_draw(g, 0, range - 1);
        CHECK(want == got, "uniform_int(0, %d) seed %d draw %d: %d != %d", range - 1, seed, k, got, want);
      }
      // both generators must have consumed the same number of words (redraws included)
      CHECK((uint32_t)ref() == mt_next(g), "uniform_int(0, %d) seed %d: generators out of step", range - 1, seed);
      if (range == 3 * (1 << 29)) redraw_probe++;
    }
    // the pair sequence of findTriangulationCandidate: a, then an offset, from one generator
    for (int32_t n : {3, 4, 63, 64, 65, 130, 1000}) {
      std::mt19937 ref(seed);
      std::uniform_int_distribution<> aDist(0, n - 1), offsetDist(1, n - 1);
      Mt19937 g;
      mt_seed(g, state, seed);
      for (int k = 0; k < 400; k++) {
        const int a = aDist(ref);
        const int b = (a + offsetDist(ref)) % n;
        int32_t ga, gb;
        draw_pair(g, n, ga, gb);
        CHECK(a == ga && b == gb, "pair n %d seed %d iteration %d: (%d, %d) != (%d, %d)", n, seed, k, ga, gb, a, b);
        CHECK(ga >= 0 && ga < n && gb >= 0 && gb < n && ga != gb, "pair n %d out of range", n);
      }
    }
  }
  CHECK(redraw_probe == (long)seeds.size(), "the redraw range was not exercised");
}

static void check_unproject(const char* path) {
  std::FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  int64_t n = 0;
  if (std::fread(&n, sizeof(n), 1, f) != 1 || n <= 0 || n > 100000) {
    std::fprintf(stderr, "bad case file\n");
    std::exit(2);
  }
  int nLinear = 0, nFisheye = 0;
  for (int64_t i = 0; i < n; i++) {
    double rec[24 + 3 + 2];
    if (std::fread(rec, sizeof(double), 29, f) != 29) {
      std::fprintf(stderr, "short case file\n");
      std::exit(2);
    }
    const double *cam = rec, *pc = rec + 24, *uv = rec + 27;
    (cam[0] == 0.0 ? nLinear : nFisheye)++;
    const V3 r = unproject(cam, uv[0], uv[1]);
    const double ex = std::fabs(r.x / r.z - pc[0] / pc[2]), ey = std::fabs(r.y / r.z - pc[1] / pc[2]);
    CHECK(ex < 1e-9 && ey < 1e-9, "unproject case %" PRId64 " (model %g): off by %.3e, %.3e", i, cam[0], ex, ey);
    // the ray of an identity pose is the normalised unprojection, from the origin
    const double T[7] = {0, 0, 0, 1, 0, 0, 0};
    const Ray ray = observation_ray(T, cam, uv[0], uv[1]);
    const double nr = norm3(r);
    CHECK(std::fabs(ray.d.x - r.x / nr) < 1e-15 && std::fabs(ray.d.y - r.y / nr) < 1e-15 &&
              std::fabs(ray.d.z - r.z / nr) < 1e-15 && ray.s.x == 0 && ray.s.y == 0 && ray.s.z == 0,
          "observation_ray case %" PRId64, i);
    // and the candidate of that ray with a second one through the same point from 1 m aside is the point
    Ray r2;
    r2.s = {1.0, 0, 0};
    const V3 v2 = {pc[0] - 1.0, pc[1], pc[2]};
    r2.d = scl3(1.0 / norm3(v2), v2);
    V3 cand;
    const bool ok = pair_candidate(ray, r2, cand);
    CHECK(ok, "pair_candidate case %" PRId64 " rejected", i);
    if (ok) {
      // a direction good to 1e-9 moves the intersection by at most 1e-9 depth^2 / baseline < 1e-7 m here
      // (depth <= 6.4 m, baseline 1 m); 1e-6 leaves room for the conditioning of the pair
      const double ec = norm3(sub3(cand, V3{pc[0], pc[1], pc[2]}));
      CHECK(ec < 1e-6, "pair_candidate case %" PRId64 ": %.3e from the point", i, ec);
      CHECK(ray_angle(r2, cand) < 1e-6, "ray_angle case %" PRId64, i);
    }
  }
  std::fclose(f);
  CHECK(nLinear > 0 && nFisheye > 0, "the cases must cover both camera models (%d linear, %d fisheye)", nLinear, nFisheye);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: triang_check CASES\n");
    return 2;
  }
  check_generator();
  check_unproject(argv[1]);
  // the skip rules of the pair geometry
  {
    const Ray a{{0, 0, 0}, {0, 0, 1}}, par{{1, 0, 0}, {0, 0, 1}};
    V3 c;
    CHECK(!pair_candidate(a, par, c), "parallel rays must give no candidate");
    // rays that diverge: their closest approach lies behind both cameras
    const double s = std::sqrt(0.5);
    const Ray l{{-1, 0, 0}, {-s, 0, s}}, r{{1, 0, 0}, {s, 0, s}};
    CHECK(!pair_candidate(l, r, c), "diverging rays must give no candidate");
    const Ray l2{{-1, 0, 0}, {s, 0, s}}, r2{{1, 0, 0}, {-s, 0, s}};
    CHECK(pair_candidate(l2, r2, c) && std::fabs(c.x) < 1e-12 && std::fabs(c.z - 1.0) < 1e-12, "converging rays");
  }
  if (failures) return 1;
  std::printf("triang_check: ok\n");
  return 0;
}
