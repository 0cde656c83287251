// Stand-alone check of the class order inside the dissection's parts (csrc/symbolic.hip, Knobs::kindOrder):
// reads a flat dump of a problem (tests/test_symbolic.py writes it), runs analyze() with the knob off and
// on, and checks what the order promises, one message per failed property, exit 1 on the first violation:
//   - both orders cut the system into the same parts: same boundaries, same owners, same variable sets;
//   - with the knob on, classes ascend inside every part and time positions ascend inside a class;
//   - with the knob off, time positions ascend inside every part;
//   - a single undivided part is in the same (time) order under both.
// Then one "counts" line per order: what the order is for.
//
//   kind_order_check DUMP [--leaf N] [--cutwin X]
#include <cstring>
#include <set>

#include "../../visual_inertial_bundle_adjustment_amd/csrc/symbolic.hpp"

using namespace viba_host;

#define CHECK(cond, ...)                  \
  do {                                    \
    if (!(cond)) {                        \
      fprintf(stderr, "VIOLATION ");      \
      fprintf(stderr, __VA_ARGS__);       \
      fprintf(stderr, "  (%s)\n", #cond); \
      exit(1);                            \
    }                                     \
  } while (0)

// the classes as the order is specified (the table in symbolic.hip is the implementation's own):
// omega, IMU calibration, IMU extrinsics first; pose, velocity; camera intrinsics, camera extrinsics last
static int classOf(int kind) {
  switch (kind) {
    case VB_VAR_OMEGA: case VB_VAR_IMU_CALIB: case VB_VAR_IMU_EXTR: return 0;
    case VB_VAR_POSE: case VB_VAR_VEL: return 1;
    case VB_VAR_CAM_INTR: case VB_VAR_CAM_EXTR: return 2;
    default: return -1;  // points and gravity are never registered
  }
}

struct Problem {
  std::vector<double> data[9];
  std::vector<uint8_t> cst[9];
  std::vector<int32_t> fvars[14], fint[14];
  std::vector<double> fconst[14];
  int64_t imuCalibOptions = 0xFF, nRS = 0;
  std::vector<PreintSrc> piSrc;
  std::vector<int64_t> imuT;
  std::vector<double> imuV, piNoise;
  std::vector<std::vector<int64_t>> piT;
  std::vector<std::vector<double>> piV;
};

template <typename T>
static void readVec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) fprintf(stderr, "short dump\n"), exit(2);
}

static void readDump(const char* path, Problem& p) {
  FILE* f = fopen(path, "rb");
  if (!f) fprintf(stderr, "cannot open %s\n", path), exit(2);
  std::vector<int64_t> head;
  readVec(f, head, 3);
  if (head[0] != 0x314d59534256) fprintf(stderr, "not a problem dump\n"), exit(2);  // "VBSYM1"
  p.imuCalibOptions = head[1], p.nRS = head[2];
  for (int k = 0; k < 9; k++) {
    std::vector<int64_t> n;
    readVec(f, n, 1);
    readVec(f, p.data[k], (size_t)n[0] * kVarData[k]);
    readVec(f, p.cst[k], (size_t)n[0]);
  }
  for (int fk = 0; fk < 14; fk++) {
    std::vector<int64_t> n;
    readVec(f, n, 1);
    readVec(f, p.fvars[fk], (size_t)n[0] * kNumVars[fk]);
    readVec(f, p.fint[fk], (size_t)n[0]);
    readVec(f, p.fconst[fk], (size_t)n[0] * kNumConsts[fk]);
  }
  fclose(f);
}

static void run(const Problem& p, const Knobs& knobs, Symbolic& S) {
  const Input in{p.data, p.cst, p.fvars, p.fint, p.fconst, (int)p.imuCalibOptions, (int32_t)p.nRS, false, 0, -1, true,
                 false,  0,     1,       p.piSrc, p.imuT, p.imuV, p.piT, p.piV, p.piNoise, knobs};
  if (Status e = analyze(in, S)) fprintf(stderr, "VIOLATION analysis failed: %d '%s'\n", e.code, e.msg), exit(1);
}

static size_t partEnd(const Symbolic& S, size_t part) {
  return part + 1 < S.nd.partBegin.size() ? S.nd.partBegin[part + 1] : S.nd.order.size();
}

// distinct tile rows of every small factor (small_assemble_kernel's per-wave table holds kAsmTiles = 7):
// the largest count and how many factors exceed the table
static void smallFactorTileRows(const Problem& p, const Symbolic& S, int& most, int64_t& over, int64_t& total) {
  const Layout& L = S.lay;
  most = 0, over = 0, total = 0;
  for (int fk = 1; fk < 14; fk++)
    for (size_t f = 0; f < p.fint[fk].size(); f++) {
      std::set<int64_t> rows;
      for (int s = 0; s < kNumVars[fk]; s++) {
        const int kind = kFK[fk][s], hh = p.fvars[fk][f * kNumVars[fk] + s];
        if (hh < 0 || kind == 0 || kind == 8 || L.redOf[kind][hh] < 0) continue;
        const int i = L.redOf[kind][hh];
        for (int64_t t = L.rvOff[i] / TS; t <= (L.rvOff[i] + L.rvDim[i] - 1) / TS; t++) rows.insert(t);
      }
      most = std::max(most, (int)rows.size());
      over += rows.size() > 7, total++;
    }
}

static void counts(const char* name, const Problem& p, const Symbolic& S) {
  int most;
  int64_t over, total;
  smallFactorTileRows(p, S, most, over, total);
  printf("counts %s: parts %zu nT %d tiles %lld contributions %lld column_levels %d sn_contributions %lld sn_levels %d "
         "schur_items %zu schur_entries %zu small_tile_rows_max %d small_over_7 %lld small_factors %lld\n",
         name, S.nd.partBegin.size(), S.lay.nT, (long long)S.pat.nTiles, (long long)S.sch[0].nPairs, S.sch[0].nLevels,
         (long long)S.sn[0].nPairs, S.sn[0].nLevels, S.schur.works.size(), S.schur.ents.size(), most, (long long)over,
         (long long)total);
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: kind_order_check DUMP [--leaf N] [--cutwin X]\n"), 2;
  Problem p;
  readDump(argv[1], p);
  Knobs knobs;
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--leaf" && i + 1 < argc) knobs.leafDims = std::max<int64_t>(64, atoll(argv[++i]));
    else if (a == "--cutwin" && i + 1 < argc) knobs.cutWin = std::max(0.0, std::min(0.45, atof(argv[++i])));
    else return fprintf(stderr, "unknown option %s\n", a.c_str()), 2;
  }
  Symbolic off, on;
  knobs.kindOrder = false;
  run(p, knobs, off);
  knobs.kindOrder = true;
  run(p, knobs, on);

  // the same parts
  CHECK(off.nd.partBegin == on.nd.partBegin, "the orders cut the system at different places\n");
  CHECK(off.nd.partOwner == on.nd.partOwner, "the orders give a part different owners\n");
  CHECK(off.nd.order.size() == on.nd.order.size() && off.reg.reg == on.reg.reg, "the orders register different variables\n");
  CHECK(off.time.pos == on.time.pos, "the time order depends on the knob\n");
  const std::vector<int>& tp = on.time.pos;
  const size_t nParts = on.nd.partBegin.size();
  for (size_t part = 0; part < nParts; part++) {
    const size_t b = on.nd.partBegin[part], e = partEnd(on, part);
    std::vector<int> a(off.nd.order.begin() + b, off.nd.order.begin() + e), c(on.nd.order.begin() + b, on.nd.order.begin() + e);
    std::sort(a.begin(), a.end()), std::sort(c.begin(), c.end());
    CHECK(a == c, "part %zu holds different variables under the two orders\n", part);
    for (size_t i = b + 1; i < e; i++) {
      const int r0 = on.nd.order[i - 1], r1 = on.nd.order[i];
      const int c0 = classOf(on.reg.reg[r0].first), c1 = classOf(on.reg.reg[r1].first);
      CHECK(c0 >= 0 && c1 >= 0, "part %zu holds a variable of no class at %zu\n", part, i);
      if (nParts > 1) {
        CHECK(c0 <= c1, "part %zu: class %d follows class %d at %zu\n", part, c1, c0, i);
        if (c0 == c1) CHECK(tp[r0] < tp[r1], "part %zu: time positions descend inside class %d at %zu\n", part, c0, i);
      }
      CHECK(tp[off.nd.order[i - 1]] < tp[off.nd.order[i]], "knob off, part %zu: time positions descend at %zu\n", part, i);
    }
  }
  // a single undivided part: the band the reference factors, in time order under both
  if (nParts == 1) CHECK(off.nd.order == on.nd.order && on.nd.order == on.time.order, "a single part is not in time order under both\n");

  counts("off", p, off);
  counts("on", p, on);
  printf("ok: %zu parts\n", nParts);
  return 0;
}
