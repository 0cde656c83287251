// Stand-alone check of vb_finalize's host-only analysis (csrc/symbolic.hip): reads a flat dump of a
// problem (tests/test_symbolic.py writes it), runs analyze() and checks the invariants the kernels take
// on trust, one message per failed property, exit 1 on the first violation.
//
//   symbolic_check DUMP [--shard BEGIN END ROOT] [--world W] [--cutwin X] [--leaf N] [--streams N]
//                       [--nosn] [--expect CODE MESSAGE] [--digest]
//
// --world W checks every rank of a W-rank partition and the properties that span the ranks.
// --digest prints (element size, count, FNV-1a) of every array of the analysis, sorted.
#include <cstring>
#include <map>
#include <set>

#include "../../visual_inertial_bundle_adjustment_amd/csrc/symbolic.hpp"

using namespace viba_host;

#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      fprintf(stderr, "VIOLATION [%s] ", g_case.c_str()); \
      fprintf(stderr, __VA_ARGS__);                       \
      fprintf(stderr, "  (%s)\n", #cond);                 \
      exit(1);                                            \
    }                                                     \
  } while (0)

static std::string g_case = "single";

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

struct Request {
  bool sharded = false;
  int64_t lmBegin = 0, lmEnd = -1;
  bool isRoot = true;
  bool partSet = false;
  int rank = 0, world = 1;
  Knobs knobs;
};

static Status run(const Problem& p, const Request& r, Symbolic& S) {
  const Input in{p.data,    p.cst,     p.fvars, p.fint, p.fconst, (int)p.imuCalibOptions, (int32_t)p.nRS, r.sharded, r.lmBegin,
                 r.lmEnd,   r.isRoot,  r.partSet, r.rank, r.world, p.piSrc, p.imuT, p.imuV, p.piT, p.piV, p.piNoise, r.knobs};
  return analyze(in, S);
}

// ---------------------------------------------------------------- layout
static void checkLayout(const Problem& p, const Request& r, const Symbolic& S) {
  const Layout& L = S.lay;
  int64_t sum = 0;
  for (int i = 0; i < L.nRV; i++) {
    CHECK(L.rvDim[i] > 0 && L.rvOff[i] + L.rvDim[i] <= L.rvOff[i + 1], "reduced block %d overlaps the next\n", i);
    CHECK(L.redOf[L.rvKind[i]][L.rvHandle[i]] == i, "redOf does not invert (rvKind, rvHandle) at %d\n", i);
    sum += L.rvDim[i];
  }
  CHECK(sum == L.nRedReal, "nRedReal %lld is not the sum of the dims %lld\n", (long long)L.nRedReal, (long long)sum);
  for (int k = 0; k < 9; k++)
    for (size_t h = 0; h < L.redOf[k].size(); h++)
      if (L.redOf[k][h] >= 0)
        CHECK(L.rvKind[L.redOf[k][h]] == k && L.rvHandle[L.redOf[k][h]] == (int32_t)h, "redOf[%d][%zu] names another variable\n", k, h);
  // pad rows: exactly the rows no block covers (pad_diag_kernel puts 1 on their diagonal)
  std::vector<uint8_t> covered((size_t)L.nT * TS, 0);
  for (int i = 0; i < L.nRV; i++)
    for (int64_t q = L.rvOff[i]; q < L.rvOff[i] + L.rvDim[i]; q++) covered[q] = 1;
  std::vector<int64_t> pads;
  for (size_t q = 0; q < covered.size(); q++)
    if (!covered[q]) pads.push_back((int64_t)q);
  CHECK(pads == L.padRows, "pad rows are not the uncovered rows\n");
  // parts on tile boundaries; one part per tile column
  std::vector<int> partOfCol(L.nT, -1);
  for (size_t part = 0; part < S.nd.partBegin.size(); part++) {
    const size_t b = S.nd.partBegin[part], e = part + 1 < S.nd.partBegin.size() ? S.nd.partBegin[part + 1] : (size_t)L.nRV;
    CHECK(L.rvOff[b] % TS == 0, "part %zu does not start on a tile boundary\n", part);
    for (size_t i = b; i < e; i++)
      for (int64_t t = L.rvOff[i] / TS; t <= (L.rvOff[i] + L.rvDim[i] - 1) / TS; t++) {
        CHECK(partOfCol[t] < 0 || partOfCol[t] == (int)part, "tile column %lld holds two parts\n", (long long)t);
        partOfCol[t] = (int)part;
        CHECK(L.colOwner[t] == S.nd.partOwner[part], "colOwner of tile column %lld is not its part's owner\n", (long long)t);
      }
  }
  if (!r.partSet)
    for (int8_t o : L.colOwner) CHECK(o == 0, "a single handle owns every column\n");
}

// ---------------------------------------------------------------- landmarks
static void checkLandmarks(const Problem& p, const Request& r, const Symbolic& S) {
  const int64_t nPts = S.reg.nPts, nObs = S.obs.nObs;
  std::vector<uint8_t> observed(p.cst[0].size(), 0);
  for (size_t f = 0; f < p.fint[0].size(); f++) observed[p.fvars[0][f * 5]] = 1;
  std::vector<int> hit(nPts, 0);
  for (size_t h = 0; h < S.reg.lmOfPoint.size(); h++) {
    const int32_t l = S.reg.lmOfPoint[h];
    CHECK((l >= 0) == (observed[h] && !p.cst[0][h]), "point %zu: landmark number without a free observed point, or none with\n", h);
    if (l >= 0) {
      CHECK(l < nPts, "landmark number out of range\n");
      hit[l]++;
    }
  }
  for (int64_t l = 0; l < nPts; l++) CHECK(hit[l] == 1, "landmark %lld is the image of %d points\n", (long long)l, hit[l]);
  // lmObs: the prefix count of the observations sorted by landmark (landmark kernels walk [lmObs[l], lmObs[l + 1]))
  CHECK(S.obs.lmObs[0] == 0, "lmObs[0]\n");
  for (int64_t l = 0; l < nPts; l++)
    for (int64_t o = S.obs.lmObs[l]; o < S.obs.lmObs[l + 1]; o++)
      CHECK(o < nObs && S.reg.lmOfPoint[S.obs.obPt[o]] == l, "observation %lld is not landmark %lld's\n", (long long)o, (long long)l);
  for (int64_t o = S.obs.lmObs[nPts]; o < nObs; o++) CHECK(S.reg.lmOfPoint[S.obs.obPt[o]] < 0, "a free point's observation past lmObs[nPts]\n");
  std::vector<int64_t> sortedPerm(S.obs.perm);
  std::sort(sortedPerm.begin(), sortedPerm.end());
  for (int64_t o = 0; o < nObs; o++) CHECK(sortedPerm[o] == o, "perm is not a permutation\n");
  if (r.partSet) {
    for (int64_t l = 0; l + 1 < nPts; l++) CHECK(S.lmRank[l] <= S.lmRank[l + 1], "a rank's landmarks are not contiguous at %lld\n", (long long)l);
    for (int64_t l = 0; l < nPts; l++)
      for (int64_t b = S.pan.lmBlk[l]; b < S.pan.lmBlk[l + 1]; b++) {
        const int o = S.lay.colOwner[S.lay.rvOff[S.pan.blkRed[b]] / TS];
        CHECK(o == S.lmRank[l] || o == r.world, "landmark %lld of rank %d touches a block of rank %d\n", (long long)l, S.lmRank[l], o);
      }
    for (int64_t l = S.shard.lmBegin; l < S.shard.lmEnd; l++) CHECK(S.lmRank[l] == r.rank, "shard holds another rank's landmark\n");
  }
}

// ---------------------------------------------------------------- pattern
struct TileRC {
  std::vector<int32_t> row, col;
};
static TileRC tileRowCol(const Symbolic& S) {
  TileRC rc;
  rc.row.assign(S.pat.nTiles, -1), rc.col.assign(S.pat.nTiles, -1);
  for (int32_t J = 0; J < S.lay.nT; J++)
    for (int64_t c = S.pat.colStart[J]; c < S.pat.colStart[J + 1]; c++) rc.row[S.pat.colTiles[c]] = S.pat.colRows[c], rc.col[S.pat.colTiles[c]] = J;
  return rc;
}

static void checkPattern(const Problem& p, const Request& r, const Symbolic& S) {
  const Pattern& P = S.pat;
  const Layout& L = S.lay;
  const int32_t nT = L.nT;
  auto idx = [&](int64_t I, int64_t J) { return P.tileIdx[(size_t)I * nT + J]; };
  // the three descriptions agree; the row lists are the transpose
  int64_t count = 0;
  for (int32_t I = 0; I < nT; I++)
    for (int32_t J = 0; J < nT; J++) {
      if (idx(I, J) < 0) continue;
      CHECK(I >= J, "tile above the diagonal\n");
      count++;
    }
  CHECK(count == P.nTiles && (int64_t)P.colTiles.size() == P.nTiles, "tile count\n");
  for (int32_t J = 0; J < nT; J++) {
    CHECK(P.colStart[J] < P.colStart[J + 1] && P.colRows[P.colStart[J]] == J, "column %d does not start with its diagonal tile\n", J);
    for (int64_t c = P.colStart[J]; c < P.colStart[J + 1]; c++) {
      CHECK(idx(P.colRows[c], J) == P.colTiles[c], "column list of %d disagrees with tileIdx\n", J);
      if (c > P.colStart[J]) CHECK(P.colRows[c] > P.colRows[c - 1], "column %d rows do not ascend\n", J);
    }
    for (int64_t c = P.rowStart[J]; c < P.rowStart[J + 1]; c++) {
      CHECK(P.rowCol[c] < J && idx(J, P.rowCol[c]) == P.rowTiles[c], "row list of %d disagrees with tileIdx\n", J);
      if (c > P.rowStart[J]) CHECK(P.rowCol[c] > P.rowCol[c - 1], "row %d columns do not ascend\n", J);
    }
  }
  CHECK(P.rowStart[nT] == P.nTiles - nT, "row lists do not hold every off-diagonal tile\n");
  // every coupling has a tile; fill is exactly the rest
  std::vector<uint8_t> coupled((size_t)nT * nT, 0);
  auto couple = [&](int a, int b) {
    if (L.rvOff[a] < L.rvOff[b]) std::swap(a, b);
    for (int64_t I = L.rvOff[a] / TS; I <= (L.rvOff[a] + L.rvDim[a] - 1) / TS; I++)
      for (int64_t J = L.rvOff[b] / TS; J <= (L.rvOff[b] + L.rvDim[b] - 1) / TS; J++)
        if (I >= J) {
          CHECK(idx(I, J) >= 0, "coupling of reduced blocks %d, %d has no tile (%lld, %lld)\n", a, b, (long long)I, (long long)J);
          coupled[I * nT + J] = 1;
        }
  };
  for (int i = 0; i < L.nRV; i++) couple(i, i);
  for (int64_t o = 0; o < S.obs.nObs; o++)
    for (int s = 0; s < 4; s++)
      for (int t = 0; t <= s; t++)
        if (S.obs.obRed[o * 4 + s] >= 0 && S.obs.obRed[o * 4 + t] >= 0) couple(S.obs.obRed[o * 4 + s], S.obs.obRed[o * 4 + t]);
  for (int64_t l = 0; l < S.reg.nPts; l++)
    for (int64_t a = S.pan.lmBlk[l]; a < S.pan.lmBlk[l + 1]; a++)
      for (int64_t b = S.pan.lmBlk[l]; b <= a; b++) couple(S.pan.blkRed[a], S.pan.blkRed[b]);
  for (int fk = 1; fk < 14; fk++)
    for (size_t f = 0; f < p.fint[fk].size(); f++)
      for (int s = 0; s < kNumVars[fk]; s++)
        for (int t = 0; t <= s; t++) {
          const int ks = kFK[fk][s], kt = kFK[fk][t], hs = p.fvars[fk][f * kNumVars[fk] + s], ht = p.fvars[fk][f * kNumVars[fk] + t];
          if (hs < 0 || ht < 0 || ks == 8 || kt == 8 || ks == 0 || kt == 0 || L.redOf[ks][hs] < 0 || L.redOf[kt][ht] < 0) continue;
          couple(L.redOf[ks][hs], L.redOf[kt][ht]);
        }
  for (int32_t I = 0; I < nT; I++)
    for (int32_t J = 0; J <= I; J++)
      if (idx(I, J) >= 0)
        CHECK(P.tileFill[idx(I, J)] == (I != J && !coupled[(size_t)I * nT + J] ? 1 : 0), "tileFill wrong on tile (%d, %d)\n", I, J);
  // closed under the symbolic Cholesky (fanin_kernel's targets exist)
  for (int32_t K = 0; K < nT; K++)
    for (int64_t a = P.colStart[K] + 1; a < P.colStart[K + 1]; a++)
      for (int64_t b = P.colStart[K] + 1; b <= a; b++)
        CHECK(idx(P.colRows[a], P.colRows[b]) >= 0, "fill missing: column %d rows %d, %d\n", K, P.colRows[a], P.colRows[b]);
  if (r.partSet)
    for (int32_t J = 0; J < nT; J++)
      for (int64_t c = P.colStart[J]; c < P.colStart[J + 1]; c++) {
        const int a = L.colOwner[J], b = L.colOwner[P.colRows[c]];
        CHECK(a == b || a == r.world || b == r.world, "tile (%d, %d) couples ranks %d and %d\n", P.colRows[c], J, b, a);
      }
}

// ---------------------------------------------------------------- Schur work (schur_run4_kernel, obs_group_kernel)
static void checkSchur(const Problem& p, const Request& r, const Symbolic& S) {
  const SchurWork& W = S.schur;
  const Pattern& P = S.pat;
  const int32_t nT = S.lay.nT;
  // every (landmark, tile) entry once
  std::set<std::pair<int32_t, uint32_t>> expected, seen;
  for (int64_t l = S.shard.lmBegin; l < S.shard.lmEnd; l++) {
    std::set<int64_t> tiles;
    for (int64_t c = S.pan.lmY[l] / 3; c < S.pan.lmY[l + 1] / 3; c++) tiles.insert(S.pan.pcRow[c] / TS);
    for (int64_t a : tiles)
      for (int64_t b : tiles)
        if (a >= b) expected.insert({P.tileIdx[(size_t)a * nT + b], (uint32_t)l});
  }
  // items: in order they partition the entries; an item's entries lie in its tile
  std::vector<int> itemsOfTile(P.nTiles, 0);
  int64_t at = 0;
  for (const TileWork& w : W.works) {
    CHECK(w.start == at && w.count > 0 && w.count <= 256, "item of tile %d leaves a gap or overlaps at entry %lld\n", w.tile, (long long)at);
    CHECK(P.tileIdx[(size_t)w.I * nT + w.J] == w.tile, "item names tile %d but (I, J) = (%d, %d)\n", w.tile, w.I, w.J);
    at += w.count;
    itemsOfTile[w.tile]++;
    for (int e = 0; e < w.count; e++) {
      const TileEnt& en = W.ents[w.start + e];
      CHECK(S.pan.pcRow[en.colI] / TS == w.I && S.pan.pcRow[en.colJ] / TS == w.J, "entry %lld is not in its item's tile\n", (long long)(w.start + e));
      CHECK(seen.insert({w.tile, en.lm}).second, "(landmark %u, tile %d) entered twice\n", en.lm, w.tile);
      uint64_t mI = 0, mJ = 0;
      for (int c = 0; c < en.nI; c++) mI |= 1ull << (S.pan.pcRow[en.colI + c] % TS);
      for (int c = 0; c < en.nJ; c++) mJ |= 1ull << (S.pan.pcRow[en.colJ + c] % TS);
      CHECK(mI == en.maskI && mJ == en.maskJ, "entry masks do not match its panel columns\n");
    }
  }
  CHECK(at == (int64_t)W.ents.size(), "items do not cover the entries\n");
  CHECK(seen == expected, "the (landmark, tile) entries are not the landmarks' tile pairs (%zu against %zu)\n", seen.size(), expected.size());
  const bool single = !r.sharded && !r.partSet;
  std::vector<uint8_t> stored(P.nTiles, 0);
  for (size_t k = 0; k < W.works.size(); k++) {
    const TileWork& w = W.works[k];
    if (k) CHECK(W.works[k - 1].tile <= w.tile, "items are not in tile order\n");
    CHECK((w.kind == 1) == (itemsOfTile[w.tile] > 1), "item kind %d on a tile with %d items\n", w.kind, itemsOfTile[w.tile]);
    CHECK((w.kind == 2) == (single && itemsOfTile[w.tile] == 1 && !P.tileDirect[w.tile]), "kind 2 where the item is not the tile's only writer (tile %d)\n", w.tile);
    if (w.kind == 2) stored[w.tile] = 1;
  }
  CHECK(W.hasClear == single, "clear list on a shard\n");
  if (single) {
    std::vector<int32_t> clr;
    for (int64_t t = 0; t < P.nTiles; t++)
      if (!stored[t]) clr.push_back((int32_t)t);
    CHECK(clr == W.clearTiles, "the clear list is not the complement of the kind-2 tiles\n");
  }
  // runs and tasks cover the item's (entry, compact block row) exactly once
  for (const TileWork& w : W.works) {
    std::vector<int> runOf(w.count), runBegin;
    for (int e = 0; e < w.count; e++) {
      const TileEnt &a = W.ents[w.start + e];
      if (e == 0 || a.maskI != W.ents[w.start + e - 1].maskI || a.maskJ != W.ents[w.start + e - 1].maskJ) runBegin.push_back(e);
      runOf[e] = (int)runBegin.size() - 1;
    }
    CHECK((int)runBegin.size() == w.nRuns, "item of tile %d: %d runs listed, %zu in its entries\n", w.tile, w.nRuns, runBegin.size());
    for (int q = 0; q < w.nRuns; q++) {
      const TileEnt& a = W.ents[w.start + runBegin[q]];
      CHECK(W.runs[2 * ((size_t)w.runFirst + q)] == a.maskI && W.runs[2 * ((size_t)w.runFirst + q) + 1] == (w.I == w.J ? a.maskI : a.maskJ), "run masks\n");
    }
    std::vector<std::array<int, 4>> cover(w.count, {0, 0, 0, 0});
    CHECK(w.wOff[0] == 0, "wOff[0]\n");
    for (int k = 0; k < 4; k++) CHECK(w.wOff[k] <= w.wOff[k + 1], "wOff descends\n");
    for (int t = 0; t < w.wOff[4]; t++) {
      const uint32_t code = W.tasks[(size_t)w.taskFirst + t];
      const int q = code & 255, c0 = (code >> 8) & 255, nl = (code >> 16) & 63, a0 = (code >> 22) & 3;
      CHECK(q < w.nRuns && nl > 0 && c0 + nl <= w.count, "task out of its item\n");
      const int nbJ = (__builtin_popcountll(W.runs[2 * ((size_t)w.runFirst + q) + 1]) + 15) / 16;
      for (int e = c0; e < c0 + nl; e++) {
        CHECK(runOf[e] == q, "task crosses a run boundary\n");
        for (int a = a0; a < std::min(nbJ, a0 + kSchurTR); a++) cover[e][a]++;
      }
    }
    for (int e = 0; e < w.count; e++) {
      const int nbJ = (__builtin_popcountll(W.runs[2 * ((size_t)w.runFirst + runOf[e]) + 1]) + 15) / 16;
      for (int a = 0; a < 4; a++) CHECK(cover[e][a] == (a < nbJ ? 1 : 0), "tasks cover entry %d block row %d of tile %d %d times\n", e, a, w.tile, cover[e][a]);
    }
  }
  // groups partition the shard's observations; one key per group
  std::vector<int32_t> mine;
  for (int64_t o = 0; o < S.obs.nObs; o++)
    if ((o >= S.shard.obB && o < S.shard.obE) || (o >= S.shard.fB && o < S.shard.fE)) mine.push_back((int32_t)o);
  std::vector<int32_t> listed(W.grpObs);
  std::sort(listed.begin(), listed.end());
  CHECK(listed == mine, "the groups do not partition the shard's observations\n");
  const size_t nG = W.grpRed.size() / 4;
  CHECK(W.grpStart.size() == nG + 1 && W.grpStart[0] == 0 && W.grpStart[nG] == (int64_t)W.grpObs.size(), "group offsets\n");
  for (size_t g = 0; g < nG; g++) {
    CHECK(W.grpStart[g] < W.grpStart[g + 1], "empty group\n");
    for (int64_t i = W.grpStart[g]; i < W.grpStart[g + 1]; i++)
      for (int s = 0; s < 4; s++) CHECK(S.obs.obRed[(size_t)W.grpObs[i] * 4 + s] == W.grpRed[4 * g + s], "group %zu holds an observation of other blocks\n", g);
    if (g) CHECK(!std::equal(&W.grpRed[4 * g], &W.grpRed[4 * g] + 4, &W.grpRed[4 * (g - 1)]), "two groups share their key\n");
  }
}

// ---------------------------------------------------------------- fan-in lists, shared by both schedules
// expected contributions (target tile, tile a, tile b) of the selected sources into the selected targets
static std::vector<std::array<int32_t, 3>> expectedContributions(const Symbolic& S, const Select& sel, const std::vector<int8_t>* role) {
  const Pattern& P = S.pat;
  std::vector<std::array<int32_t, 3>> out;
  for (int32_t K = 0; K < S.lay.nT; K++) {
    if (!sel.src[K]) continue;
    for (int64_t a = P.colStart[K] + 1; a < P.colStart[K + 1]; a++)
      for (int64_t b = P.colStart[K] + 1; b <= a; b++) {
        if (!sel.tgt[P.colRows[b]]) continue;
        if (role && (*role)[K] == 1 && P.colRows[b] == K + 1) continue;  // inside the pair
        out.push_back({P.tileIdx[(size_t)P.colRows[a] * S.lay.nT + P.colRows[b]], P.colTiles[a], P.colTiles[b]});
      }
  }
  std::sort(out.begin(), out.end());
  return out;
}

// chunks (tile, first, count, split) of the segments [lv[s], lv[s + 1]): tile every target's range, split
// flag iff several chunks (fanin_kernel: atomics on split targets), target in segment levelOfSeg, sources
// earlier.  levelOf: per column.
static void checkFanIn(const char* what, const Symbolic& S, const Select& sel, const std::vector<int8_t>* role,
                       const std::vector<int32_t>& upd, const std::vector<int32_t>& pairs, const std::vector<int64_t>& lv,
                       const std::vector<int32_t>& levelOfSeg, const std::vector<int32_t>& levelOf, int64_t nPairs) {
  const TileRC rc = tileRowCol(S);
  CHECK((int64_t)pairs.size() == 2 * nPairs, "%s: pair list length\n", what);
  std::map<int32_t, std::vector<std::array<int32_t, 3>>> byTile;  // tile -> (first, count, split)
  for (size_t s = 0; s + 1 < lv.size(); s++)
    for (int64_t u = lv[s]; u < lv[s + 1]; u++) {
      const int32_t t = upd[4 * u];
      CHECK(sel.tgt[rc.col[t]], "%s: chunk on a tile outside the selected targets\n", what);
      CHECK(levelOf[rc.col[t]] == levelOfSeg[s], "%s: target tile %d of column level %d in a segment of level %d\n", what, t, levelOf[rc.col[t]], levelOfSeg[s]);
      byTile[t].push_back({upd[4 * u + 1], upd[4 * u + 2], upd[4 * u + 3]});
    }
  CHECK(lv.back() * 4 == (int64_t)upd.size(), "%s: chunk list length\n", what);
  int64_t at = 0;
  std::vector<std::array<int32_t, 3>> listed;
  for (auto& [t, chunks] : byTile) {
    std::sort(chunks.begin(), chunks.end());
    for (const auto& c : chunks) {
      CHECK(c[0] == at && c[1] > 0, "%s: chunks of target tile %d leave a gap or overlap at contribution %lld\n", what, t, (long long)at);
      CHECK(c[2] == (chunks.size() > 1 ? 1 : 0), "%s: split flag %d on target tile %d with %zu chunks\n", what, c[2], t, chunks.size());
      for (int64_t q = c[0]; q < c[0] + c[1]; q++) {
        const int32_t a = pairs[2 * q], b = pairs[2 * q + 1];
        CHECK(rc.col[a] == rc.col[b] && rc.row[a] == rc.row[t] && rc.row[b] == rc.col[t], "%s: contribution %lld is not two tiles of one column with the target's rows\n", what, (long long)q);
        CHECK(levelOf[rc.col[a]] < levelOf[rc.col[t]], "%s: source column %d (level %d) is not factored before target column %d (level %d)\n", what, rc.col[a], levelOf[rc.col[a]], rc.col[t], levelOf[rc.col[t]]);
        listed.push_back({t, a, b});
      }
      at += c[1];
    }
  }
  CHECK(at == nPairs, "%s: chunks cover %lld of %lld contributions\n", what, (long long)at, (long long)nPairs);
  std::sort(listed.begin(), listed.end());
  const auto expected = expectedContributions(S, sel, role);
  CHECK(listed.size() == expected.size(), "%s: %zu contributions listed, %zu expected\n", what, listed.size(), expected.size());
  CHECK(listed == expected, "%s: the contributions listed are not the expected ones\n", what);
}

// ---------------------------------------------------------------- column schedule (factorSeq, fwd/bwd_fanout_kernel)
static void checkColumnSchedule(const Symbolic& S, const Select& sel, const SchedHost& C, int64_t ptFuseMax) {
  const Pattern& P = S.pat;
  const int32_t nT = S.lay.nT;
  const int32_t nLev = C.nLevels;
  std::vector<int32_t> levelOf(nT, -1), segLevel(nLev);
  std::iota(segLevel.begin(), segLevel.end(), 0);
  for (int32_t L = 0; L < nLev; L++)
    for (int64_t i = C.lvP[L]; i < C.lvP[L + 1]; i++) {
      const int32_t J = C.potrfCol[i];
      CHECK(sel.col[J] && levelOf[J] < 0, "column %d is in two levels, or not selected\n", J);
      CHECK(C.potrfTile[i] == P.colTiles[P.colStart[J]], "potrf tile of column %d\n", J);
      levelOf[J] = L;
    }
  for (int32_t J = 0; J < nT; J++) CHECK((levelOf[J] >= 0) == (bool)sel.col[J], "selected column %d is in no level\n", J);
  // columns this schedule does not factor keep the pattern's level (sources of other ranks, ROOT targets)
  for (int32_t J = 0; J < nT; J++)
    if (levelOf[J] < 0) levelOf[J] = P.level[J];
  for (int32_t J = 0; J < nT; J++)
    for (int64_t c = P.rowStart[J]; c < P.rowStart[J + 1]; c++)
      CHECK(levelOf[J] > levelOf[P.rowCol[c]], "column %d (level %d) does not come after column %d of its row list (level %d)\n", J, levelOf[J], P.rowCol[c], levelOf[P.rowCol[c]]);
  checkFanIn("column schedule", S, sel, nullptr, C.upd, C.fanPairs, C.lvU, segLevel, levelOf, C.nPairs);
  // trsm: each off-diagonal tile of a selected column once, in its column's level
  std::vector<int> hit(P.nTiles, 0);
  for (int32_t L = 0; L < nLev; L++)
    for (int64_t i = C.lvT[L]; i < C.lvT[L + 1]; i++) {
      const int32_t t = C.trsmTarget[i], J = C.trsmCol[i];
      CHECK(levelOf[J] == L && sel.col[J] && P.tileIdx[(size_t)C.trsmRow[i] * nT + J] == t && C.trsmDiag[i] == P.colTiles[P.colStart[J]], "trsm item %lld\n", (long long)i);
      hit[t]++;
    }
  for (int32_t J = 0; J < nT; J++)
    for (int64_t c = P.colStart[J] + 1; c < P.colStart[J + 1]; c++)
      CHECK(hit[P.colTiles[c]] == (sel.col[J] ? 1 : 0), "off-diagonal tile %d is in the trsm list %d times\n", P.colTiles[c], hit[P.colTiles[c]]);
  // fused levels (potrf_trsm_kernel): iff the level has at most ptFuseMax off-diagonal tiles; one writer per column
  int64_t nDiag = 0;
  for (int32_t L = 0; L < nLev; L++) {
    const bool fused = C.lvPF[L + 1] > C.lvPF[L];
    const bool want = ptFuseMax > 0 && C.lvP[L + 1] > C.lvP[L] && C.lvT[L + 1] - C.lvT[L] <= ptFuseMax;
    CHECK(fused == want, "level %d fused %d with %lld off-diagonal tiles\n", L, fused, (long long)(C.lvT[L + 1] - C.lvT[L]));
    std::map<int32_t, int> writers, items;
    for (int64_t i = C.lvPF[L]; i < C.lvPF[L + 1]; i++) writers[C.ptf[5 * i + 1]] += C.ptf[5 * i + 4], items[C.ptf[5 * i + 1]]++;
    if (fused)
      for (int64_t i = C.lvP[L]; i < C.lvP[L + 1]; i++) {
        const int32_t J = C.potrfCol[i];
        CHECK(writers[J] == 1, "fused level %d: column %d has %d writers\n", L, J, writers[J]);
        CHECK(items[J] == std::max<int64_t>(1, P.colStart[J + 1] - P.colStart[J] - 1), "fused level %d: items of column %d\n", L, J);
        nDiag++;
      }
  }
  CHECK(nDiag == C.nPtfDiag && (int64_t)C.ptfDiag.size() == 2 * nDiag, "fused diagonal list\n");
  // solve task lists: the counts the kernels wait for; a column's diagonal task before its tile tasks
  std::vector<int32_t> inF(nT, 0), inB(nT, 0);
  std::vector<uint8_t> diagF(nT, 0), diagB(nT, 0);
  CHECK((int64_t)C.tasksF.size() == 2 * C.nF && (int64_t)C.tasksB.size() == 2 * C.nB, "task counts\n");
  for (int64_t i = 0; i < C.nF; i++) {
    const int32_t K = C.tasksF[2 * i], c = C.tasksF[2 * i + 1];
    CHECK(sel.col[K], "forward task of an unselected column\n");
    if (c < 0) {
      CHECK(!diagF[K], "two forward diagonal tasks of column %d\n", K);
      diagF[K] = 1;
    } else {
      CHECK(diagF[K], "forward tile task of column %d before its diagonal task\n", K);
      CHECK(c > P.colStart[K] && c < P.colStart[K + 1], "forward tile task outside its column\n");
      inF[P.colRows[c]]++;
    }
  }
  for (int64_t i = 0; i < C.nB; i++) {
    const int32_t J = C.tasksB[2 * i], c = C.tasksB[2 * i + 1];
    if (c < 0) {
      CHECK(sel.col[J] && !diagB[J], "backward diagonal task of column %d\n", J);
      diagB[J] = 1;
    } else {
      CHECK(diagB[J] || sel.pre[J], "backward tile task of row %d before its diagonal task\n", J);
      CHECK(c >= P.rowStart[J] && c < P.rowStart[J + 1] && sel.col[P.rowCol[c]], "backward tile task outside its row\n");
      inB[P.rowCol[c]]++;
    }
  }
  for (int32_t K = 0; K < nT; K++) {
    if (!sel.col[K]) continue;
    CHECK(diagF[K] && diagB[K], "column %d lacks a diagonal solve task\n", K);
    CHECK(C.expF[K] == inF[K], "expF[%d] = %d but %d forward tasks write the row\n", K, C.expF[K], inF[K]);
    CHECK(C.expB[K] == inB[K], "expB[%d] = %d but %d backward tasks write the column\n", K, C.expB[K], inB[K]);
  }
  std::vector<int32_t> pre;
  for (int32_t J = 0; J < nT; J++)
    if (sel.pre[J]) pre.push_back(J);
  std::vector<int32_t> listed(C.preReady);
  std::sort(listed.begin(), listed.end());
  CHECK(listed == pre, "preReady is not the rows known before the backward solve\n");
}

// ---------------------------------------------------------------- supernode schedule (factorSeqSn)
static void checkSupernodes(const Symbolic& S, const Select& sel, const SnSchedHost& N) {
  const Pattern& P = S.pat;
  const int32_t nT = S.lay.nT;
  const size_t nSeg = N.segG.size();
  CHECK(N.lvU.size() == nSeg + 1 && N.lvS.size() == nSeg + 1 && N.lvR.size() == nSeg + 1 && N.lvF.size() == nSeg + 1, "segment offsets\n");
  // supernodes partition the selected columns; a pair satisfies the pair condition (sntrsm_kernel: the rows of
  // a pair are the rows of its second column)
  std::vector<int> hit(nT, 0), rowsHit(P.nTiles, 0);
  std::vector<int32_t> firstOf(nT, -1), segOf(nT, -1);
  int64_t nSuper = 0, nTwo = 0;
  auto supernode = [&](int32_t J0, int32_t t11, int32_t t21, int32_t t22, size_t seg) {
    const bool two = t21 >= 0;
    CHECK(t11 == P.tileIdx[(size_t)J0 * nT + J0], "supernode %d: diagonal tile\n", J0);
    hit[J0]++, firstOf[J0] = J0, segOf[J0] = (int)seg, nSuper++;
    if (!two) return;
    const int32_t J2 = J0 + 1;
    CHECK(J2 < nT && t21 == P.tileIdx[(size_t)J2 * nT + J0] && t22 == P.tileIdx[(size_t)J2 * nT + J2], "pair %d: its tiles\n", J0);
    hit[J2]++, firstOf[J2] = J0, segOf[J2] = (int)seg, nTwo++;
    CHECK(P.colStart[J0 + 1] - P.colStart[J0] >= 2 && P.colRows[P.colStart[J0] + 1] == J2, "pair %d: %d is not its first off-diagonal row\n", J0, J2);
    for (int64_t c = P.colStart[J0] + 2; c < P.colStart[J0 + 1]; c++)
      CHECK(P.tileIdx[(size_t)P.colRows[c] * nT + J2] >= 0, "pair %d: row %d of its first column is not a row of its second\n", J0, P.colRows[c]);
    CHECK(S.lay.colOwner[J0] == S.lay.colOwner[J2], "pair %d spans two parts' owners\n", J0);
  };
  for (size_t s = 0; s < nSeg; s++) {
    for (int64_t i = N.lvS[s]; i < N.lvS[s + 1]; i++) supernode(N.pot[4 * i + 1], N.pot[4 * i], N.pot[4 * i + 2], N.pot[4 * i + 3], s);
    for (int64_t i = N.lvF[s]; i < N.lvF[s + 1]; i++)
      if (N.fus[8 * i + 7] == 1) supernode(N.fus[8 * i + 1], N.fus[8 * i], N.fus[8 * i + 2], N.fus[8 * i + 3], s);
  }
  for (int32_t J = 0; J < nT; J++) CHECK(hit[J] == (sel.col[J] ? 1 : 0), "column %d is in %d supernodes\n", J, hit[J]);
  CHECK(nSuper == N.nSuper && nTwo == N.nTwo, "supernode counts\n");
  // row items cover each row of each supernode once
  auto rowItem = [&](int32_t J0, int32_t tA, int32_t tB, int32_t I) {
    const bool two = firstOf[J0 + (J0 + 1 < nT ? 1 : 0)] == J0 && J0 + 1 < nT && hit[J0 + 1] && firstOf[J0 + 1] == J0;
    const int32_t Jl = two ? J0 + 1 : J0;
    CHECK((two ? tB : tA) == P.tileIdx[(size_t)I * nT + Jl], "row item (%d, %d): tile of the last column\n", I, J0);
    if (two) CHECK(tA == P.tileIdx[(size_t)I * nT + J0], "row item (%d, %d): tile of the first column (may be -1: not in the pattern)\n", I, J0);
    rowsHit[P.tileIdx[(size_t)I * nT + Jl]]++;
  };
  for (size_t s = 0; s < nSeg; s++) {
    for (int64_t i = N.lvR[s]; i < N.lvR[s + 1]; i++) rowItem(N.row[8 * i + 2], N.row[8 * i], N.row[8 * i + 1], N.row[8 * i + 4]);
    for (int64_t i = N.lvF[s]; i < N.lvF[s + 1]; i++)
      if (N.fus[8 * i + 6] >= 0) rowItem(N.fus[8 * i + 1], N.fus[8 * i + 4], N.fus[8 * i + 5], N.fus[8 * i + 6]);
  }
  for (int32_t J = 0; J < nT; J++) {
    if (!sel.col[J]) continue;
    const bool firstOfPair = J + 1 < nT && firstOf[J + 1] == J && firstOf[J] == J && hit[J + 1];
    if (firstOfPair) continue;  // a pair's rows are its second column's
    for (int64_t c = P.colStart[J] + 1; c < P.colStart[J + 1]; c++)
      CHECK(rowsHit[P.colTiles[c]] == 1, "row %d of the supernode ending in column %d is covered %d times\n", P.colRows[c], J, rowsHit[P.colTiles[c]]);
  }
  // levels: segments are level-major; a supernode's level exceeds its sources'
  std::vector<int32_t> levelOf(nT);
  for (int32_t J = 0; J < nT; J++) levelOf[J] = segOf[J] >= 0 ? N.segL[segOf[J]] : N.level[J];
  for (size_t s = 1; s < nSeg; s++) CHECK(N.segL[s] > N.segL[s - 1] || (N.segL[s] == N.segL[s - 1] && N.segG[s] > N.segG[s - 1]), "segments are not level-major\n");
  std::vector<int32_t> segLevel(N.segL.begin(), N.segL.end());
  checkFanIn("supernode schedule", S, sel, &N.pairRole, N.upd, N.fanPairs, N.lvU, segLevel, levelOf, N.nPairs);
  for (int32_t J = 0; J < nT; J++) CHECK(N.pairRole[J] == (firstOf[J] < 0 ? N.pairRole[J] : firstOf[J] != J ? 2 : (J + 1 < nT && firstOf[J + 1] == J && hit[J + 1]) ? 1 : 0), "pair roles and the supernode lists disagree at column %d\n", J);
  // inverse lists: disjoint, together every selected column
  std::vector<int> inv(nT, 0);
  for (int32_t J : N.invEarly) inv[J]++;
  for (int32_t J : N.invLate) inv[J]++;
  for (int32_t J = 0; J < nT; J++) CHECK(inv[J] == (sel.col[J] ? 1 : 0), "column %d is in the inverse lists %d times\n", J, inv[J]);
  CHECK((int64_t)N.invEarly.size() == N.nInvEarly && (int64_t)N.invLate.size() == N.nInvLate, "inverse list counts\n");
  // streams: a segment waits for the stream of every child supernode that runs on another stream
  for (int32_t J0 = 0; J0 < nT; J0++) {
    if (!sel.col[J0] || firstOf[J0] != J0) continue;
    const int32_t Jl = (J0 + 1 < nT && firstOf[J0 + 1] == J0 && hit[J0 + 1]) ? J0 + 1 : J0;
    if (P.colStart[Jl + 1] - P.colStart[Jl] < 2) continue;
    const int32_t parentCol = P.colRows[P.colStart[Jl] + 1];
    if (segOf[parentCol] < 0) continue;
    const int sp = segOf[parentCol], sc = segOf[J0];
    CHECK(N.segL[sp] > N.segL[sc], "supernode %d is not before its parent\n", J0);
    if (N.segG[sp] != N.segG[sc])
      CHECK((N.segDep[sp] >> N.segG[sc]) & 1, "segment %d (stream %d, level %d) does not wait for stream %d of child supernode %d\n", sp, N.segG[sp], N.segL[sp], N.segG[sc], J0);
  }
  for (size_t s = 0; s < nSeg; s++) CHECK(N.segG[s] >= 0 && N.segG[s] < N.nGroups && !((N.segDep[s] >> N.segG[s]) & 1), "segment %zu stream\n", s);
}

// ---------------------------------------------------------------- all checks of one handle
static void checkAll(const Problem& p, const Request& r, const Symbolic& S) {
  checkLayout(p, r, S);
  checkLandmarks(p, r, S);
  checkPattern(p, r, S);
  checkSchur(p, r, S);
  const int32_t nT = S.lay.nT;
  const Select sel0 = r.partSet ? selectRank(S.lay.colOwner, r.rank, r.world) : selectAll(nT);
  const Select sel1 = selectRoot(S.lay.colOwner, r.world);
  checkColumnSchedule(S, sel0, S.sch[0], r.knobs.ptFuseMax);
  if (r.partSet && r.rank == 0) checkColumnSchedule(S, sel1, S.sch[1], r.knobs.ptFuseMax);
  CHECK(S.sn[0].built == r.knobs.useSn, "supernode schedule built against the knob\n");
  if (r.knobs.useSn) {
    checkSupernodes(S, sel0, S.sn[0]);
    CHECK(S.sn[0].nGroups == (r.partSet ? 1 : std::max(1, r.knobs.snStreams)), "stream count\n");
    if (r.partSet && r.rank == 0) checkSupernodes(S, sel1, S.sn[1]);
  }
  if (r.partSet) {  // the tiles a rank's lists write lie in its zeroRuns; a non-root's Schur targets in shardTiles
    std::vector<uint8_t> zeroed(S.pat.nTiles, 0);
    for (auto [a, b] : S.part.zeroRuns)
      for (int64_t c = a; c < b; c++) zeroed[S.pat.colTiles[c]] = 1;
    for (int i = 0; i < 2; i++) {
      if (!S.sch[i].built) continue;
      for (size_t u = 0; u < S.sch[i].upd.size(); u += 4) CHECK(zeroed[S.sch[i].upd[u]], "fan-in target outside zeroRuns\n");
      for (int32_t t : S.sch[i].potrfTile) CHECK(zeroed[t], "potrf tile outside zeroRuns\n");
      for (int32_t t : S.sch[i].trsmTarget) CHECK(zeroed[t], "trsm tile outside zeroRuns\n");
    }
    for (const TileWork& w : S.schur.works) CHECK(zeroed[w.tile], "Schur item on a tile outside zeroRuns\n");
  }
  if (!S.shard.isRoot) {
    std::set<int32_t> mine(S.schur.shardTiles.begin(), S.schur.shardTiles.end());
    for (const TileWork& w : S.schur.works) CHECK(mine.count(w.tile), "Schur item on a tile outside shardTiles\n");
    for (int32_t t : S.schur.shardTiles) CHECK(t >= S.schur.tileFirst && t < S.schur.tileFirst + S.schur.tileCount, "shardTiles outside the tile range\n");
  }
}

// ---------------------------------------------------------------- digest
struct Digest {
  uint64_t size, count, hash;
  bool operator<(const Digest& o) const { return size != o.size ? size < o.size : count != o.count ? count < o.count : hash < o.hash; }
};
static std::vector<Digest> g_digest;
template <typename T>
static void add(const std::vector<T>& v, size_t use = sizeof(T)) {
  uint64_t h = 1469598103934665603ull;
  for (const T& x : v)
    for (size_t k = 0; k < use; k++) h = (h ^ ((const unsigned char*)&x)[k]) * 1099511628211ull;
  g_digest.push_back({sizeof(T), v.size(), h});
}
static void digest(const Problem& p, const Symbolic& S) {
  for (int k = 0; k < 9; k++) add(p.data[k]), add(S.lay.redOf[k]);
  add(S.lay.rvKind), add(S.lay.rvHandle), add(S.lay.rvDim), add(S.lay.rvOff), add(S.pat.rowEnd), add(S.lay.padRows), add(S.lay.colOwner);
  add(S.cost.order), add(S.cost.pack), add(S.cost.cp);
  add(S.obs.obPose), add(S.obs.obExtr), add(S.obs.obIntr), add(S.obs.obVel), add(S.obs.obRS), add(S.obs.obPt), add(S.obs.obRed), add(S.pan.obCol), add(S.obs.obC);
  add(S.shard.lmList), add(S.obs.lmObs), add(S.pan.lmY), add(S.pan.lmBlk), add(S.pan.blkRed), add(S.pan.blkCol), add(S.reg.lmOfPoint);
  add(S.pan.pcRow), add(S.pan.pcBlk), add(S.pan.bxStart), add(S.pan.bxEnt);
  add(S.pan.oxStart), add(S.pan.oxObs), add(S.pan.oxSlot), add(S.pan.lxStart), add(S.pan.lxLm), add(S.pan.lxCol), add(S.pan.lxChunk);
  add(S.schur.grpStart), add(S.schur.grpObs), add(S.schur.grpRed), add(S.schur.runs), add(S.schur.tasks), add(S.schur.works, 52), add(S.schur.ents);
  if (S.schur.hasClear) add(S.schur.clearTiles);
  if (!S.schur.shardTiles.empty()) add(S.schur.shardTiles);
  add(S.pat.tileIdx), add(S.pat.colStart), add(S.pat.rowStart), add(S.pat.colTiles), add(S.pat.colRows), add(S.pat.rowTiles), add(S.pat.rowCol);
  for (int i = 0; i < 2; i++) {
    const SchedHost& C = S.sch[i];
    if (C.built)
      add(C.potrfTile), add(C.potrfCol), add(C.trsmDiag), add(C.trsmTarget), add(C.trsmCol), add(C.trsmRow), add(C.upd), add(C.fanPairs),
          add(C.tasksF), add(C.tasksB), add(C.expF), add(C.expB), add(C.preReady), add(C.ptf), add(C.ptfDiag);
    const SnSchedHost& N = S.sn[i];
    if (N.built) add(N.upd), add(N.fanPairs), add(N.pot), add(N.row), add(N.fus), add(N.copy), add(N.invEarly), add(N.invLate);
  }
  for (int fk = 1; fk < 14; fk++) add(p.fvars[fk]), add(S.small.consts[fk]);
  std::sort(g_digest.begin(), g_digest.end());
  printf("digest %zu\n", g_digest.size());
  for (const Digest& d : g_digest) printf("%llu %llu %016llx\n", (unsigned long long)d.size, (unsigned long long)d.count, (unsigned long long)d.hash);
}

int main(int argc, char** argv) {
  if (argc < 2) return fprintf(stderr, "usage: symbolic_check DUMP [options]\n"), 2;
  Problem p;
  readDump(argv[1], p);
  Request r;
  int world = 0, expectCode = 0;
  const char* expectMsg = nullptr;
  bool wantDigest = false;
  for (int i = 2; i < argc; i++) {
    const std::string a = argv[i];
    if (a == "--shard" && i + 3 < argc) r.sharded = true, r.lmBegin = atoll(argv[i + 1]), r.lmEnd = atoll(argv[i + 2]), r.isRoot = atoi(argv[i + 3]) != 0, i += 3;
    else if (a == "--world" && i + 1 < argc) world = atoi(argv[++i]);
    else if (a == "--cutwin" && i + 1 < argc) r.knobs.cutWin = std::max(0.0, std::min(0.45, atof(argv[++i])));
    else if (a == "--leaf" && i + 1 < argc) r.knobs.leafDims = std::max<int64_t>(64, atoll(argv[++i]));
    else if (a == "--streams" && i + 1 < argc) r.knobs.snStreams = std::max(1, std::min(4, atoi(argv[++i])));
    else if (a == "--nosn") r.knobs.useSn = false;
    else if (a == "--expect" && i + 2 < argc) expectCode = atoi(argv[i + 1]), expectMsg = argv[i + 2], i += 2;
    else if (a == "--digest") wantDigest = true;
    else return fprintf(stderr, "unknown option %s\n", a.c_str()), 2;
  }
  Symbolic single;
  const Status st = run(p, r, single);
  if (expectMsg) {
    if (st.code != expectCode || strcmp(st.msg, expectMsg)) return fprintf(stderr, "VIOLATION expected error %d '%s', got %d '%s'\n", expectCode, expectMsg, st.code, st.msg), 1;
    return printf("ok: error %d '%s'\n", st.code, st.msg), 0;
  }
  if (st) return fprintf(stderr, "VIOLATION analysis failed: %d '%s'\n", st.code, st.msg), 1;
  checkAll(p, r, single);
  printf("ok single: nRV %d nT %d tiles %lld parts %zu levels %d contributions %lld; supernodes %lld (%lld two-column) levels %d segments %zu; "
         "items %zu entries %zu groups %zu\n",
         single.lay.nRV, single.lay.nT, (long long)single.pat.nTiles, single.nd.partBegin.size(), single.sch[0].nLevels,
         (long long)single.sch[0].nPairs, (long long)single.sn[0].nSuper, (long long)single.sn[0].nTwo, single.sn[0].nLevels,
         single.sn[0].segG.size(), single.schur.works.size(), single.schur.ents.size(), single.schur.grpRed.size() / 4);
  if (wantDigest && !world) digest(p, single);
  if (world) {
    // the same problem partitioned (the ordering is the single handle's: same knobs), every rank
    Request base = r;
    base.sharded = false, base.lmBegin = 0, base.lmEnd = -1;
    Symbolic whole;  // world > 1 changes the owners only, world 1 none: the contribution count to compare with
    if (Status e = run(p, base, whole)) return fprintf(stderr, "VIOLATION analysis failed\n"), 1;
    std::vector<int> factored;
    int64_t contributions = 0, landmarks = 0;
    for (int rank = 0; rank < world; rank++) {
      Request q = base;
      q.partSet = true, q.rank = rank, q.world = world;
      g_case = "rank " + std::to_string(rank) + "/" + std::to_string(world);
      Symbolic S;
      if (Status e = run(p, q, S)) return fprintf(stderr, "VIOLATION [%s] analysis failed: %d '%s'\n", g_case.c_str(), e.code, e.msg), 1;
      checkAll(p, q, S);
      CHECK(S.lay.nT == whole.lay.nT && S.pat.nTiles == whole.pat.nTiles, "a partition changes the pattern\n");
      factored.resize(S.lay.nT, 0);
      for (int i = 0; i < 2; i++)
        if (S.sch[i].built) {
          for (int32_t J : S.sch[i].potrfCol) factored[J]++;
          contributions += S.sch[i].nPairs;
        }
      CHECK(S.shard.lmBegin == landmarks, "ranks' landmark ranges do not abut\n");
      landmarks = S.shard.lmEnd;
      if (rank == world - 1) CHECK(landmarks == S.reg.nPts, "ranks' landmark ranges do not cover the landmarks\n");
      printf("ok %s: own columns %zu, contributions %lld + %lld, landmarks [%lld, %lld)\n", g_case.c_str(), S.sch[0].potrfCol.size(),
             (long long)S.sch[0].nPairs, (long long)S.sch[1].nPairs, (long long)S.shard.lmBegin, (long long)S.shard.lmEnd);
      if (wantDigest) g_digest.clear(), digest(p, S);
    }
    g_case = "world " + std::to_string(world);
    for (size_t J = 0; J < factored.size(); J++) CHECK(factored[J] == 1, "column %zu is factored %d times over all ranks and ROOT\n", J, factored[J]);
    CHECK(contributions == whole.sch[0].nPairs, "ranks' contributions %lld differ from the single handle's %lld\n", (long long)contributions, (long long)whole.sch[0].nPairs);
  }
  return 0;
}
