// Stand-alone check of the finalize stage of the base-map visual factors (csrc/symbolic.hip: the landmark
// numbering of points that only base-map factors see, Shard::loneList, baseMapOrder): reads the flat problem
// dump of tests/test_symbolic.py followed by the base-map factors' points (int64 count, int32 handles; tests/
// test_basemap.py writes both), runs analyze() and checks what the kernels of csrc/basemap.hip and the landmark
// hooks take on trust.  One message per failed property, exit 1 on the first violation.
//
//   basemap_check DUMP [--expect CODE]
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
  std::vector<int32_t> bmPoint;
};

template <typename T>
static void readVec(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) fprintf(stderr, "short dump\n"), exit(2);
}

static void readDump(const char* path, Problem& p) {
  FILE* f = fopen(path, "rb");
  if (!f) fprintf(stderr, "cannot open %s\n", path), exit(2);
  std::vector<int64_t> head, n;
  readVec(f, head, 3);
  if (head[0] != 0x314d59534256) fprintf(stderr, "not a problem dump\n"), exit(2);
  p.imuCalibOptions = head[1], p.nRS = head[2];
  for (int k = 0; k < 9; k++) {
    readVec(f, n, 1);
    readVec(f, p.data[k], (size_t)n[0] * kVarData[k]);
    readVec(f, p.cst[k], (size_t)n[0]);
  }
  for (int fk = 0; fk < 14; fk++) {
    readVec(f, n, 1);
    readVec(f, p.fvars[fk], (size_t)n[0] * kNumVars[fk]);
    readVec(f, p.fint[fk], (size_t)n[0]);
    readVec(f, p.fconst[fk], (size_t)n[0] * kNumConsts[fk]);
  }
  readVec(f, n, 1);
  readVec(f, p.bmPoint, (size_t)n[0]);
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: basemap_check DUMP [--expect CODE]\n"), 2;
  int expect = 0;
  for (int i = 2; i < argc; i++)
    if (!strcmp(argv[i], "--expect") && i + 1 < argc) expect = atoi(argv[++i]);
  Problem p;
  readDump(argv[1], p);
  const Input in{p.data, p.cst, p.fvars, p.fint, p.fconst, (int)p.imuCalibOptions, (int32_t)p.nRS, false, 0, -1, true,
                 false,  0,     1,       p.piSrc, p.imuT, p.imuV, p.piT, p.piV, p.piNoise, Knobs(), &p.bmPoint};
  Symbolic S;
  const Status st = analyze(in, S);
  if (expect) {
    CHECK(st.code == expect, "analyze returned %d (%s), expected %d\n", st.code, st.msg, expect);
    printf("ok: %d (%s)\n", st.code, st.msg);
    return 0;
  }
  CHECK(st.code == 0, "analyze failed: %d (%s)\n", st.code, st.msg);

  const BaseMapOrder& B = S.bm;
  const int64_t n = (int64_t)p.bmPoint.size(), nPts = S.reg.nPts;
  const std::vector<int32_t>& lmOf = S.reg.lmOfPoint;
  CHECK(B.n == n, "%lld factors in the order, %lld given\n", (long long)B.n, (long long)n);
  if (n == 0) {
    CHECK(B.start.empty() && B.rowOfPos.empty() && B.posOfRow.empty() && B.lmWith.empty() && S.shard.loneList.empty(),
          "a problem without base-map factors has base-map tables\n");
    printf("ok: no base-map factors\n");
    return 0;
  }
  // bmStart: monotone over the landmark order, from 0 to the number of free-point factors
  CHECK((int64_t)B.start.size() == nPts + 1 && B.start[0] == 0, "bmStart has %zu entries for %lld landmarks\n", B.start.size(), (long long)nPts);
  for (int64_t l = 0; l < nPts; l++) CHECK(B.start[l] <= B.start[l + 1], "bmStart decreases at landmark %lld\n", (long long)l);
  CHECK(B.start[nPts] == B.nFree && B.nFree <= n, "bmStart ends at %lld, nFree %lld\n", (long long)B.start[nPts], (long long)B.nFree);
  // the row map is a permutation, its inverse is posOfRow
  CHECK((int64_t)B.rowOfPos.size() == n && (int64_t)B.posOfRow.size() == n, "row maps have the wrong size\n");
  std::vector<uint8_t> seen(n, 0);
  for (int64_t i = 0; i < n; i++) {
    const int32_t r = B.rowOfPos[i];
    CHECK(r >= 0 && r < n && !seen[r], "rowOfPos is not a permutation at position %lld\n", (long long)i);
    seen[r] = 1;
    CHECK(B.posOfRow[r] == i, "posOfRow does not invert rowOfPos at position %lld\n", (long long)i);
  }
  // every free-point factor exactly once inside its landmark's range; constant-point factors last
  int64_t freeRows = 0;
  for (int64_t r = 0; r < n; r++) freeRows += lmOf[p.bmPoint[r]] >= 0;
  CHECK(freeRows == B.nFree, "%lld free-point factors, nFree %lld\n", (long long)freeRows, (long long)B.nFree);
  for (int64_t l = 0; l < nPts; l++)
    for (int64_t i = B.start[l]; i < B.start[l + 1]; i++) {
      CHECK(lmOf[p.bmPoint[B.rowOfPos[i]]] == l, "position %lld is not a factor of landmark %lld\n", (long long)i, (long long)l);
      CHECK(i == B.start[l] || B.rowOfPos[i - 1] < B.rowOfPos[i], "rows of landmark %lld are out of order\n", (long long)l);
    }
  for (int64_t i = B.nFree; i < n; i++) {
    const int32_t pt = p.bmPoint[B.rowOfPos[i]];
    CHECK(p.cst[0][pt] && lmOf[pt] < 0, "position %lld of the tail is not a constant point's factor\n", (long long)i);
    CHECK(i == B.nFree || B.rowOfPos[i - 1] < B.rowOfPos[i], "the constant-point tail is out of order\n");
  }
  // lmWith: exactly the landmarks with a non-empty range, ascending
  std::vector<int32_t> with;
  for (int64_t l = 0; l < nPts; l++)
    if (B.start[l + 1] > B.start[l]) with.push_back((int32_t)l);
  CHECK(with == B.lmWith, "lmWith is not the list of landmarks with base-map factors\n");
  // every free point a base-map factor names is a landmark; a constant one is none
  for (int64_t r = 0; r < n; r++) {
    const int32_t pt = p.bmPoint[r];
    CHECK(p.cst[0][pt] ? lmOf[pt] < 0 : (lmOf[pt] >= 0 && lmOf[pt] < nPts), "point %d of row %lld has the wrong landmark\n", pt, (long long)r);
  }
  // the lone list: exactly the landmarks with an empty observation range, each with base-map factors and an
  // empty panel, disjoint from lmList; together the two lists are every landmark once
  const Shard& sh = S.shard;
  std::set<int32_t> lone(sh.loneList.begin(), sh.loneList.end()), staged(sh.lmList.begin(), sh.lmList.end());
  CHECK(lone.size() == sh.loneList.size() && staged.size() == sh.lmList.size(), "a landmark list names a landmark twice\n");
  CHECK((int64_t)sh.lmList.size() == sh.nLmSmall + sh.nLmBig, "lmList does not hold its two classes\n");
  for (int64_t l = 0; l < nPts; l++) {
    const bool empty = S.obs.lmObs[l + 1] == S.obs.lmObs[l];
    CHECK(lone.count((int32_t)l) == (empty ? 1u : 0u), "landmark %lld: lone list and observation range disagree\n", (long long)l);
    CHECK(staged.count((int32_t)l) == (empty ? 0u : 1u), "landmark %lld: a record-staging list holds an empty range (or misses one)\n", (long long)l);
    if (empty) {
      CHECK(B.start[l + 1] > B.start[l], "lone landmark %lld has no base-map factor\n", (long long)l);
      CHECK(S.pan.lmY[l + 1] == S.pan.lmY[l] && S.pan.lmBlk[l + 1] == S.pan.lmBlk[l], "lone landmark %lld has a panel\n", (long long)l);
    }
  }
  CHECK(std::is_sorted(sh.loneList.begin(), sh.loneList.end()), "the lone list is not ascending\n");
  for (const TileEnt& e : S.schur.ents) CHECK(!lone.count((int32_t)e.lm), "a Schur entry names lone landmark %u\n", e.lm);
  printf("ok: %lld base-map factors, %lld of free points, %zu landmarks with factors, %zu lone\n", (long long)n,
         (long long)B.nFree, B.lmWith.size(), sh.loneList.size());
  return 0;
}
