// vb_finalize's symbolic analysis, host-only (symbolic.hpp): nested-dissection order of the reduced
// variables, tile pattern and symbolic fill (≙ Optimizer::initSolver, Optimizer.cpp:166-207), the landmark /
// observation-group layouts, the Schur work lists, the factorization schedules (level-scheduled columns,
// two-column supernodes on streams) and the solve task lists.  No HIP API call, no handle, no getenv.
#include "symbolic.hpp"

namespace viba_host {

void psdSqrt(const double* Pm, int m, double* U) {
  std::vector<double> A(Pm, Pm + m * m), V(m * m, 0.0);
  for (int i = 0; i < m; i++) V[i * m + i] = 1.0;
  for (int sweep = 0; sweep < 60; sweep++) {
    double off = 0;
    for (int p = 0; p < m; p++)
      for (int q = p + 1; q < m; q++) off += A[p * m + q] * A[p * m + q];
    if (off < 1e-30) break;
    for (int p = 0; p < m; p++)
      for (int q = p + 1; q < m; q++) {
        const double apq = A[p * m + q];
        if (std::abs(apq) < 1e-300) continue;
        const double th = 0.5 * (A[q * m + q] - A[p * m + p]) / apq;
        const double t = (th >= 0 ? 1.0 : -1.0) / (std::abs(th) + std::sqrt(th * th + 1.0));
        const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < m; k++) {
          const double akp = A[k * m + p], akq = A[k * m + q];
          A[k * m + p] = c * akp - s * akq, A[k * m + q] = s * akp + c * akq;
        }
        for (int k = 0; k < m; k++) {
          const double apk = A[p * m + k], aqk = A[q * m + k];
          A[p * m + k] = c * apk - s * aqk, A[q * m + k] = s * apk + c * aqk;
        }
        for (int k = 0; k < m; k++) {
          const double vkp = V[k * m + p], vkq = V[k * m + q];
          V[k * m + p] = c * vkp - s * vkq, V[k * m + q] = s * vkp + c * vkq;
        }
      }
  }
  // U = diag(sqrt(lambda)) V^T  (rows = eigenvectors scaled)
  for (int i = 0; i < m; i++) {
    const double l = std::sqrt(std::max(0.0, A[i * m + i]));
    for (int j = 0; j < m; j++) U[i * m + j] = l * V[j * m + i];
  }
}

bool precisionChol(const double* cov, int m, double* U) {
  std::vector<double> A(cov, cov + m * m), Pi(m * m, 0.0);
  // invert via Gauss-Jordan with partial pivoting
  std::vector<double> I(m * m, 0.0);
  for (int i = 0; i < m; i++) I[i * m + i] = 1.0;
  std::vector<double> M(m * m);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) M[i * m + j] = A[j * m + i];  // row-major
  for (int c = 0; c < m; c++) {
    int piv = c;
    for (int r = c + 1; r < m; r++)
      if (std::abs(M[r * m + c]) > std::abs(M[piv * m + c])) piv = r;
    if (std::abs(M[piv * m + c]) < 1e-300) return false;
    for (int k = 0; k < m; k++) std::swap(M[c * m + k], M[piv * m + k]), std::swap(I[c * m + k], I[piv * m + k]);
    const double inv = 1.0 / M[c * m + c];
    for (int k = 0; k < m; k++) M[c * m + k] *= inv, I[c * m + k] *= inv;
    for (int r = 0; r < m; r++) {
      if (r == c) continue;
      const double f = M[r * m + c];
      if (f == 0.0) continue;
      for (int k = 0; k < m; k++) M[r * m + k] -= f * M[c * m + k], I[r * m + k] -= f * I[c * m + k];
    }
  }
  // symmetrize P and Cholesky (lower L, row-major), U = L^T
  std::vector<double> L(m * m, 0.0);
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) Pi[i * m + j] = 0.5 * (I[i * m + j] + I[j * m + i]);
  for (int j = 0; j < m; j++) {
    double dd = Pi[j * m + j];
    for (int k = 0; k < j; k++) dd -= L[j * m + k] * L[j * m + k];
    if (!(dd > 0)) return false;
    dd = std::sqrt(dd);
    L[j * m + j] = dd;
    for (int i = j + 1; i < m; i++) {
      double s = Pi[i * m + j];
      for (int k = 0; k < j; k++) s -= L[i * m + k] * L[j * m + k];
      L[i * m + j] = s / dd;
    }
  }
  for (int i = 0; i < m; i++)
    for (int j = 0; j < m; j++) U[i * m + j] = L[j * m + i];
  return true;
}

namespace {
// first and last tile of reduced block r
inline int64_t tileLo(const Layout& lay, int r) { return lay.rvOff[r] / TS; }
inline int64_t tileHi(const Layout& lay, int r) { return (lay.rvOff[r] + lay.rvDim[r] - 1) / TS; }

// owner of the tile column a variable's block starts in, -1 when it has none
int redOwner(const Layout& lay, int kind, int32_t handle) {
  if (handle < 0 || kind == 8 || lay.redOf[kind][handle] < 0) return -1;
  return lay.colOwner[lay.rvOff[lay.redOf[kind][handle]] / TS];
}
// partition mode: an observation goes to the rank whose subtree interior it touches -- never two (a
// variable coupled across a cut is in that cut's separator); one touching only ROOT columns, to rank 0
int obsOwner(const Input& in, const Layout& lay, int64_t f) {
  const int32_t* v = &in.fvars[0][f * 5];
  const int owners[4] = {redOwner(lay, 1, v[1]), redOwner(lay, 5, v[2]), redOwner(lay, 4, v[3]),
                         in.fint[0][f] >= 0 ? redOwner(lay, 2, v[4]) : -1};
  for (int o : owners)
    if (o >= 0 && o < in.partWorld) return o;
  return 0;  // ROOT columns only (or none): rank 0
}
}  // namespace

// ---------------------------------------------------------------- 1. registration (registerAllVariables;
// points = elimination range) and landmark numbering
Status registerVariables(const Input& in, Registration& reg) {
  reg.jacSize = makeJac(in.imuCalibOptions).size;
  for (int k = 0; k < 9; k++) {
    reg.nvar[k] = (int64_t)in.cst[k].size();
    if ((int64_t)in.data[k].size() != reg.nvar[k] * kVarData[k]) return {VB_E_ARG, "variable data size mismatch"};
  }
  for (int k = 0; k < 9; k++) reg.regOf[k].assign(reg.nvar[k], -1);
  std::vector<int32_t>& lmOf = reg.lmOfPoint;
  lmOf.assign(reg.nvar[0], -1);
  reg.reg.clear();
  for (int fk = 0; fk < 14; fk++) {
    const int nv = kNumVars[fk];
    const int64_t n = (int64_t)in.fint[fk].size();
    for (int64_t f = 0; f < n; f++)
      for (int s = 0; s < nv; s++) {
        const int kind = kFK[fk][s], hh = in.fvars[fk][f * nv + s];
        if (hh < 0) continue;
        if (hh >= reg.nvar[kind]) return {VB_E_ARG, "factor references an unknown variable handle"};
        if (in.cst[kind][hh]) continue;
        if (kind == 8) return {VB_E_UNSUPPORTED, "non-constant gravity is not supported"};
        if (kind == 0) {
          if (lmOf[hh] < 0) lmOf[hh] = -2;  // mark; numbered below
          continue;
        }
        if (reg.regOf[kind][hh] < 0) {
          reg.regOf[kind][hh] = (int32_t)reg.reg.size();
          reg.reg.push_back({kind, hh});
        }
      }
  }
  // a free point that a base-map factor names is a landmark too (with no visual row: an empty observation
  // range, numbered after the observed ones)
  if (in.bmPoint)
    for (const int32_t hh : *in.bmPoint) {
      if (hh < 0 || hh >= reg.nvar[0]) return {VB_E_ARG, "base-map factor references an unknown point"};
      if (!in.cst[0][hh] && lmOf[hh] < 0) lmOf[hh] = -2;
    }
  // landmark numbering: by the earliest rig that observes the point (time-banded landmark shards
  // and locality of the Schur lists), ties by handle
  reg.nPts = 0;
  std::vector<int64_t> firstRig(reg.nvar[0], INT64_MAX);
  const int64_t nVisual = (int64_t)in.fint[0].size();
  for (int64_t f = 0; f < nVisual; f++) {
    const int32_t pt = in.fvars[0][f * 5], pose = in.fvars[0][f * 5 + 1];
    if (lmOf[pt] == -2) firstRig[pt] = std::min<int64_t>(firstRig[pt], pose);
  }
  std::vector<int64_t> pts;
  for (int64_t p = 0; p < reg.nvar[0]; p++)
    if (lmOf[p] == -2) pts.push_back(p);
  std::stable_sort(pts.begin(), pts.end(), [&](int64_t a, int64_t b) { return firstRig[a] < firstRig[b]; });
  for (int64_t p : pts) lmOf[p] = (int32_t)reg.nPts++;
  // tangent sizes
  reg.tdims.resize(reg.reg.size());
  for (size_t r = 0; r < reg.reg.size(); r++) {
    const auto [kind, hh] = reg.reg[r];
    switch (kind) {
      case 0: case 2: case 3: reg.tdims[r] = 3; break;
      case 1: case 5: case 7: reg.tdims[r] = 6; break;
      case 4: {
        const double* c = &in.data[4][(size_t)hh * 24];
        reg.tdims[r] = (int)c[1] + (c[7] != 0 ? 1 : 0) + (c[8] != 0 ? 1 : 0);
        break;
      }
      case 6: reg.tdims[r] = reg.jacSize; break;
      default: reg.tdims[r] = 2;
    }
  }
  return {};
}

// ---------------------------------------------------------------- 2. time order (mean pose ordinal of the
// co-occurring poses) and, per variable, the span of time positions it is coupled to
void timeOrder(const Input& in, const Registration& reg, TimeOrder& time) {
  const int nRV = (int)reg.reg.size();
  std::vector<double> poseSum(nRV, 0.0), poseCnt(nRV, 0.0);
  for (int fk = 0; fk < 14; fk++) {
    const int nv = kNumVars[fk];
    const int64_t n = (int64_t)in.fint[fk].size();
    for (int64_t f = 0; f < n; f++) {
      double ps = 0;
      int pc = 0;
      for (int s = 0; s < nv; s++)
        if (kFK[fk][s] == 1 && in.fvars[fk][f * nv + s] >= 0) ps += in.fvars[fk][f * nv + s], pc++;
      if (!pc) continue;
      for (int s = 0; s < nv; s++) {
        const int kind = kFK[fk][s], hh = in.fvars[fk][f * nv + s];
        if (hh < 0 || kind == 0 || kind == 8 || reg.regOf[kind][hh] < 0) continue;
        poseSum[reg.regOf[kind][hh]] += ps, poseCnt[reg.regOf[kind][hh]] += pc;
      }
    }
  }
  std::vector<int>& ord = time.order;
  ord.resize(nRV);
  std::iota(ord.begin(), ord.end(), 0);
  auto key = [&](int r) {
    return reg.reg[r].first == 1 ? (double)reg.reg[r].second : (poseCnt[r] > 0 ? poseSum[r] / poseCnt[r] : 1e30);
  };
  std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) {
    const double ka = key(a), kb = key(b);
    if (ka != kb) return ka < kb;
    if (reg.reg[a].first != reg.reg[b].first) return reg.reg[a].first < reg.reg[b].first;
    return reg.reg[a].second < reg.reg[b].second;
  });
  std::vector<int>& tp = time.pos;
  tp.resize(nRV);
  for (int i = 0; i < nRV; i++) tp[ord[i]] = i;
  std::vector<int>&hiP = time.hiP, &loP = time.loP;
  hiP = tp, loP = tp;
  const std::vector<int32_t>& lmOf = reg.lmOfPoint;
  auto regPos = [&](int kind, int hh) -> int {
    if (hh < 0 || kind == 0 || kind == 8 || reg.regOf[kind][hh] < 0) return -1;
    return tp[reg.regOf[kind][hh]];
  };
  std::vector<int> lmLo(reg.nPts, INT32_MAX), lmHi(reg.nPts, -1);
  const int64_t nVisual = (int64_t)in.fint[0].size();
  auto obsPos = [&](int64_t f, int* ps) {
    const int32_t* v = &in.fvars[0][f * 5];
    ps[0] = regPos(1, v[1]), ps[1] = regPos(5, v[2]), ps[2] = regPos(4, v[3]);
    ps[3] = in.fint[0][f] >= 0 ? regPos(2, v[4]) : -1;
  };
  for (int64_t f = 0; f < nVisual; f++) {
    int ps[4];
    obsPos(f, ps);
    const int l = lmOf[in.fvars[0][f * 5]];
    int lo = INT32_MAX, hi = -1;
    for (int k = 0; k < 4; k++)
      if (ps[k] >= 0) lo = std::min(lo, ps[k]), hi = std::max(hi, ps[k]);
    if (hi < 0) continue;
    if (l >= 0) {
      lmLo[l] = std::min(lmLo[l], lo), lmHi[l] = std::max(lmHi[l], hi);
    } else {
      for (int k = 0; k < 4; k++)
        if (ps[k] >= 0) {
          const int r = ord[ps[k]];
          hiP[r] = std::max(hiP[r], hi), loP[r] = std::min(loP[r], lo);
        }
    }
  }
  for (int64_t f = 0; f < nVisual; f++) {
    const int l = lmOf[in.fvars[0][f * 5]];
    if (l < 0 || lmHi[l] < 0) continue;
    int ps[4];
    obsPos(f, ps);
    for (int k = 0; k < 4; k++)
      if (ps[k] >= 0) {
        const int r = ord[ps[k]];
        hiP[r] = std::max(hiP[r], lmHi[l]), loP[r] = std::min(loP[r], lmLo[l]);
      }
  }
  for (int fk = 1; fk < 14; fk++) {
    const int nv = kNumVars[fk];
    const int64_t n = (int64_t)in.fint[fk].size();
    for (int64_t f = 0; f < n; f++) {
      int lo = INT32_MAX, hi = -1;
      for (int sl = 0; sl < nv; sl++) {
        const int q = regPos(kFK[fk][sl], in.fvars[fk][f * nv + sl]);
        if (q >= 0) lo = std::min(lo, q), hi = std::max(hi, q);
      }
      for (int sl = 0; sl < nv; sl++) {
        const int q = regPos(kFK[fk][sl], in.fvars[fk][f * nv + sl]);
        if (q >= 0) hiP[ord[q]] = std::max(hiP[ord[q]], hi), loP[ord[q]] = std::min(loP[ord[q]], lo);
      }
    }
  }
}

// ---------------------------------------------------------------- 3. nested dissection over the time order
// (the ordering is ours).  The time-ordered reduced system is a band (landmark tracks span
// up to ~60 rigs), whose Cholesky is a chain as long as the matrix.  Recursive bisection: cut the time
// order at half its dimension; the variables coupled across the cut form the separator, ordered after
// both halves; each part starts on a tile boundary so that parts stay independent tile columns and the
// factorization runs level by level (factorSeq).  Any symmetric order is a valid Cholesky order: the
// separators only need to be sufficient, not minimal.
namespace {
struct Dissector {
  const std::vector<int>& tdims;
  const TimeOrder& time;
  const double cutWin;
  const int64_t leafDims;
  // partitioned factorization (vb_set_partition, world = 2^k): the parts below depth k belong to the
  // subtree (= rank) they descend from; the separators above, and any part emitted there, are ROOT
  // parts (factored by rank 0)
  const int world, partK;
  Dissection& out;

  // a separator above depth k is ROOT; an undivided set above depth k is a whole subtree, so it goes to
  // the first rank of the ranks below it
  void emit(const std::vector<int>& part, bool separator, int depth, int sub, int own) {
    if (part.empty()) return;
    out.partBegin.push_back(out.order.size());
    out.partOwner.push_back(own >= 0 ? own : separator ? world : (sub << (partK - depth)) % world);
    out.order.insert(out.order.end(), part.begin(), part.end());
  }

  // cut: the thinnest separator -- the left variables coupled across the cut, or the right ones --
  // among the cuts within +-cutWin of the part's median `median` (config C: 954k -> 701k tile
  // contributions, 110 -> 89 levels against the median cut with left separators; wider windows unbalance
  // the parts: 0.1: 746k, 0.25: 880k; an imbalance penalty was tried and dropped).
  // Returns the cut; right: the separator is taken from the right half.
  size_t chooseCut(const std::vector<int>& vs, size_t median, bool& right) const {
    const std::vector<int>&tp = time.pos, &hiP = time.hiP, &loP = time.loP;
    const int nRV = (int)tp.size();
    const size_t w = (size_t)(cutWin * (double)vs.size());
    const size_t k0 = median > w + 1 ? median - w : 1, k1 = std::min(vs.size() - 1, median + w);
    // separator widths of every candidate cut c (vs ascends in tp): sl(c) = dims of the i < c with
    // hiP >= tp(c), sr(c) = dims of the i >= c with loP < tp(c); two sweeps over Fenwick trees keyed
    // by time position, O(|vs| log nRV) per part instead of a rescan per candidate
    const size_t nc = k1 - k0 + 1;
    std::vector<int64_t> sepLeft(nc, 0), sepRight(nc, 0), bit(nRV + 1, 0);
    auto bitAdd = [&](int pos, int64_t v) { for (int x = std::min(pos, nRV - 1) + 1; x <= nRV; x += x & -x) bit[x] += v; };
    auto bitSum = [&](int pos) { int64_t r = 0; for (int x = pos; x > 0; x -= x & -x) r += bit[x]; return r; };  // keys < pos
    int64_t tot = 0;
    for (size_t i = 0; i < k0; i++) bitAdd(hiP[vs[i]], tdims[vs[i]]), tot += tdims[vs[i]];
    for (size_t c = k0; c <= k1; c++) {
      sepLeft[c - k0] = tot - bitSum(tp[vs[c]]);
      bitAdd(hiP[vs[c]], tdims[vs[c]]), tot += tdims[vs[c]];
    }
    std::fill(bit.begin(), bit.end(), 0);
    for (size_t i = vs.size(); i-- > k1 + 1;) bitAdd(loP[vs[i]], tdims[vs[i]]);
    for (size_t c = k1 + 1; c-- > k0;) {
      bitAdd(loP[vs[c]], tdims[vs[c]]);
      sepRight[c - k0] = bitSum(tp[vs[c]]);
    }
    double best = 1e300;
    size_t bestCut = median;
    right = false;
    for (size_t c = k0; c <= k1; c++) {
      if ((double)sepLeft[c - k0] < best) best = (double)sepLeft[c - k0], bestCut = c, right = false;
      if ((double)sepRight[c - k0] < best) best = (double)sepRight[c - k0], bestCut = c, right = true;
    }
    return bestCut;
  }

  void run(const std::vector<int>& vs, int depth, int sub, int own) {
    if (own < 0 && depth == partK) own = sub % world;
    int64_t dims = 0;
    for (int r : vs) dims += tdims[r];
    if (dims <= leafDims || vs.size() < 4) return emit(vs, false, depth, sub, own);
    int64_t acc = 0;
    size_t k = 0;
    while (k < vs.size() && acc + tdims[vs[k]] <= dims / 2) acc += tdims[vs[k++]];
    if (k == 0 || k >= vs.size()) return emit(vs, false, depth, sub, own);
    // cutWin 0: the round-1 order, the median cut with left separators (tests/test_ordering_gpu.py)
    bool right = false;
    if (cutWin > 0.0) k = chooseCut(vs, k, right);
    const int cut = time.pos[vs[k]];
    std::vector<int> left, rightPart, sep;
    int64_t sepDims = 0;
    if (!right) {  // separator: the left variables coupled across the cut
      rightPart.assign(vs.begin() + k, vs.end());
      for (size_t i = 0; i < k; i++) {
        if (time.hiP[vs[i]] >= cut) sep.push_back(vs[i]), sepDims += tdims[vs[i]];
        else left.push_back(vs[i]);
      }
    } else {  // the right variables coupled across it
      left.assign(vs.begin(), vs.begin() + k);
      for (size_t i = k; i < vs.size(); i++) {
        if (time.loP[vs[i]] < cut) sep.push_back(vs[i]), sepDims += tdims[vs[i]];
        else rightPart.push_back(vs[i]);
      }
    }
    if (left.empty() || rightPart.empty() || 2 * sepDims > dims) return emit(vs, false, depth, sub, own);  // no useful separator
    run(left, depth + 1, 2 * sub, own);
    run(rightPart, depth + 1, 2 * sub + 1, own);
    emit(sep, true, depth, sub, own);
  }
};

// Class of every variable kind in a part's order (Knobs::kindOrder).  The landmark band's fill couples
// only the kinds a visual factor names (kFK[0]); the other kinds couple along the time chain alone, so
// rows of theirs interleaved by time carry that fill as structural zeros.  Grouped, their tiles stay out
// of the band (config C: 701k -> 604k fan-in contributions).
//   0: omega, IMU calibration, IMU extrinsics -- in no visual factor: chain-only, eliminated first
//   1: pose, velocity                         -- one per rig: the band proper
//   2: camera intrinsics, camera extrinsics   -- few, coupled to every rig that observes through them:
//                                                dense rows, last, so their fill stays in the part's corner
//  -1: points are eliminated before the reduced system and gravity is constant: neither is registered
constexpr int kKindClass[9] = {-1, 1, 1, 0, 2, 2, 0, 0, -1};

// stable-sort every part (leaf or separator) by class: time order inside a class.  A single undivided
// part keeps the plain time order: that is the band the reference factors (bench.py's banded count,
// VIBA_ND_LEAF above the system).
void classOrder(const Registration& reg, Dissection& nd) {
  if (nd.partBegin.size() < 2) return;
  for (size_t p = 0; p < nd.partBegin.size(); p++) {
    const size_t e = p + 1 < nd.partBegin.size() ? nd.partBegin[p + 1] : nd.order.size();
    std::stable_sort(nd.order.begin() + nd.partBegin[p], nd.order.begin() + e,
                     [&](int a, int b) { return kKindClass[reg.reg[a].first] < kKindClass[reg.reg[b].first]; });
  }
}
}  // namespace

void dissect(const Input& in, const Registration& reg, const TimeOrder& time, Dissection& nd) {
  int partK = 0;
  while ((1 << partK) < in.partWorld) partK++;
  // world 1: the top separator is still the ROOT part, both subtrees below it are rank 0's (so a
  // one-rank partitioned run takes every exchange of the protocol, e.g. over RCCL with one GPU)
  if (in.partSet && partK == 0) partK = 1;
  nd.order.clear(), nd.partBegin.clear(), nd.partOwner.clear();
  Dissector d{reg.tdims, time, in.knobs.cutWin, in.knobs.leafDims, in.partWorld, partK, nd};
  d.run(time.order, 0, 0, -1);
  if (in.knobs.kindOrder) classOrder(reg, nd);
}

// ---------------------------------------------------------------- 4. reduced layout: blocks in the
// dissection's order, every part on a tile boundary; pad rows; owner of every tile column
Status reducedLayout(const Registration& reg, const Dissection& nd, Layout& lay) {
  const int nRV = (int)reg.reg.size();
  lay.nRV = nRV;
  lay.rvKind.resize(nRV), lay.rvHandle.resize(nRV), lay.rvDim.resize(nRV), lay.rvOff.resize(nRV + 1);
  for (int k = 0; k < 9; k++) lay.redOf[k] = reg.regOf[k];
  lay.padRows.clear();
  int64_t off = 0;
  lay.nRedReal = 0;
  size_t part = 0;
  for (int i = 0; i < nRV; i++) {
    if (part < nd.partBegin.size() && nd.partBegin[part] == (size_t)i) {  // parts start on a tile boundary
      const int64_t aligned = (off + TS - 1) / TS * TS;
      for (int64_t r = off; r < aligned; r++) lay.padRows.push_back(r);
      off = aligned, part++;
    }
    const auto [kind, hh] = reg.reg[nd.order[i]];
    lay.rvKind[i] = kind, lay.rvHandle[i] = hh, lay.rvDim[i] = reg.tdims[nd.order[i]], lay.rvOff[i] = off;
    off += lay.rvDim[i], lay.nRedReal += lay.rvDim[i];
    lay.redOf[kind][hh] = i;
  }
  const int64_t aligned = (off + TS - 1) / TS * TS;
  for (int64_t r = off; r < aligned; r++) lay.padRows.push_back(r);
  lay.rvOff[nRV] = off;
  lay.nRed = off;
  // the small-factor assembly packs a reduced row with 5 more bits into an int32 (small.hip)
  if (lay.nRed >= ((int64_t)1 << 26)) return {VB_E_ARG, "reduced system order must stay below 2^26"};
  lay.nT = (int32_t)((lay.nRed + TS - 1) / TS);
  // owner of every tile column (trailing padding joins the last part).  Parts start on tile boundaries
  // and a part's alignment padding shares a tile with its last rows, so every tile column holds
  // variables of exactly one part.
  lay.colOwner.assign(lay.nT, (int8_t)(nd.partOwner.empty() ? 0 : nd.partOwner.back()));
  part = 0;
  for (int i = 0; i < nRV; i++) {
    while (part + 1 < nd.partBegin.size() && nd.partBegin[part + 1] <= (size_t)i) part++;
    for (int64_t t = tileLo(lay, i); t <= tileHi(lay, i); t++) lay.colOwner[t] = (int8_t)nd.partOwner[part];
  }
  return {};
}

// ---------------------------------------------------------------- 5. partition mode: landmarks go to the
// rank that owns their observations (obsOwner) and are renumbered so every rank's are contiguous
// (stable: time order within a rank)
void landmarkOwners(const Input& in, const Layout& lay, Registration& reg, std::vector<int>& lmRank) {
  const int64_t nPts = reg.nPts;
  const int64_t nVisual = (int64_t)in.fint[0].size();
  std::vector<int> owner(nPts, -1);
  for (int64_t f = 0; f < nVisual; f++) {
    const int l = reg.lmOfPoint[in.fvars[0][f * 5]];
    if (l < 0) continue;
    owner[l] = std::max(owner[l], obsOwner(in, lay, f));
  }
  std::vector<int32_t> byRank(nPts);
  std::iota(byRank.begin(), byRank.end(), 0);
  std::vector<int> rankOld(nPts);
  for (int64_t l = 0; l < nPts; l++) rankOld[l] = std::max(0, owner[l]);
  std::stable_sort(byRank.begin(), byRank.end(), [&](int32_t a, int32_t b) { return rankOld[a] < rankOld[b]; });
  std::vector<int32_t> newIdx(nPts);
  for (int64_t i = 0; i < nPts; i++) newIdx[byRank[i]] = (int32_t)i;
  for (auto& x : reg.lmOfPoint)
    if (x >= 0) x = newIdx[x];
  lmRank.assign(nPts, 0);
  for (int64_t l = 0; l < nPts; l++) lmRank[newIdx[l]] = rankOld[l];
}

// ---------------------------------------------------------------- 6. visual observations, sorted by
// landmark (constant-point observations at the end, by owner when partitioned)
Status sortObservations(const Input& in, const Registration& reg, const Layout& lay, Observations& obs) {
  const int64_t nObs = (int64_t)in.fint[0].size(), nPts = reg.nPts;
  const std::vector<int32_t>& lmOf = reg.lmOfPoint;
  obs.perm.resize(nObs);
  std::iota(obs.perm.begin(), obs.perm.end(), 0);
  auto lmKey = [&](int64_t f) -> int64_t {
    const int l = lmOf[in.fvars[0][f * 5]];
    return l < 0 ? (in.partSet ? INT64_MAX - in.partWorld + obsOwner(in, lay, f) : INT64_MAX) : l;
  };
  std::stable_sort(obs.perm.begin(), obs.perm.end(), [&](int64_t a, int64_t b) { return lmKey(a) < lmKey(b); });
  obs.nObs = nObs;
  obs.nObsPad = ((nObs + 255) / 256) * 256;
  obs.obPose.resize(nObs), obs.obExtr.resize(nObs), obs.obIntr.resize(nObs), obs.obVel.resize(nObs);
  obs.obRS.resize(nObs), obs.obPt.resize(nObs);
  obs.obRed.assign(nObs * 4, -1);
  obs.obC.resize(nObs * 6);
  obs.lmObs.assign(nPts + 1, 0);
  for (int64_t i = 0; i < nObs; i++) {
    const int64_t f = obs.perm[i];
    const int32_t* v = &in.fvars[0][f * 5];
    obs.obPt[i] = v[0], obs.obPose[i] = v[1], obs.obExtr[i] = v[2], obs.obIntr[i] = v[3];
    obs.obRS[i] = in.fint[0][f];
    obs.obVel[i] = obs.obRS[i] >= 0 ? v[4] : 0;
    if (obs.obRS[i] >= in.nRS) return {VB_E_ARG, "visual factor references an unknown RS table"};
    if (obs.obRS[i] >= 0 && (v[4] < 0 || v[4] >= reg.nvar[2])) return {VB_E_ARG, "RS visual factor needs a velocity"};
    obs.obRed[i * 4 + 0] = lay.redOf[1][v[1]];
    obs.obRed[i * 4 + 1] = lay.redOf[5][v[2]];
    obs.obRed[i * 4 + 2] = lay.redOf[4][v[3]];
    obs.obRed[i * 4 + 3] = obs.obRS[i] >= 0 ? lay.redOf[2][v[4]] : -1;
    std::copy(&in.fconst[0][f * 6], &in.fconst[0][f * 6] + 6, &obs.obC[i * 6]);
    const int l = lmOf[v[0]];
    if (l >= 0) obs.lmObs[l + 1]++;
  }
  for (int64_t l = 0; l < nPts; l++) obs.lmObs[l + 1] += obs.lmObs[l];
  return {};
}

// ---------------------------------------------------------------- 7. landmark blocks D(l), Y panel columns,
// block -> observation slots (landmark_kernel), incidence lists O(X), L(X)
Status landmarkPanels(const Registration& reg, const Layout& lay, const Observations& obs, Panels& pan) {
  const int64_t nPts = reg.nPts, nObs = obs.nObs;
  const int nRV = lay.nRV;
  const std::vector<int32_t>& obRed = obs.obRed;
  const std::vector<int64_t>& lmObs = obs.lmObs;
  std::vector<int64_t>&lmBlk = pan.lmBlk, &lmY = pan.lmY;
  std::vector<int32_t>&blkRed = pan.blkRed, &blkCol = pan.blkCol;
  lmBlk.assign(nPts + 1, 0), lmY.assign(nPts + 1, 0);
  blkRed.clear(), blkCol.clear();
  pan.obCol.assign(nObs * 4, -1);
  std::vector<int32_t> blocks;
  for (int64_t l = 0; l < nPts; l++) {
    blocks.clear();
    for (int64_t o = lmObs[l]; o < lmObs[l + 1]; o++)
      for (int s = 0; s < 4; s++)
        if (obRed[o * 4 + s] >= 0) blocks.push_back(obRed[o * 4 + s]);
    std::sort(blocks.begin(), blocks.end());
    blocks.erase(std::unique(blocks.begin(), blocks.end()), blocks.end());
    int32_t col = 0;
    for (int32_t r : blocks) {
      blkRed.push_back(r);
      blkCol.push_back(col);
      col += lay.rvDim[r];
    }
    lmBlk[l + 1] = (int64_t)blkRed.size();
    lmY[l + 1] = lmY[l] + 3 * (int64_t)col;
    for (int64_t o = lmObs[l]; o < lmObs[l + 1]; o++)
      for (int s = 0; s < 4; s++) {
        const int32_t r = obRed[o * 4 + s];
        if (r < 0) continue;
        const int64_t q = std::lower_bound(blkRed.begin() + lmBlk[l], blkRed.begin() + lmBlk[l + 1], r) - blkRed.begin();
        pan.obCol[o * 4 + s] = (blkCol[q] << 5) | lay.rvDim[r];  // panel column and width (<= 17) in one word
      }
  }
  // reduced row and landmark block of every landmark panel column
  pan.nYcol = lmY[nPts] / 3;
  pan.pcRow.assign(pan.nYcol, 0), pan.pcBlk.assign(pan.nYcol, 0);
  for (int64_t l = 0; l < nPts; l++)
    for (int64_t b = lmBlk[l]; b < lmBlk[l + 1]; b++) {
      const int32_t r = blkRed[b];
      for (int j = 0; j < lay.rvDim[r]; j++) {
        pan.pcRow[lmY[l] / 3 + blkCol[b] + j] = (int32_t)(lay.rvOff[r] + j);
        pan.pcBlk[lmY[l] / 3 + blkCol[b] + j] = (int32_t)b;
      }
    }
  // landmark block -> its observation slots
  pan.bxStart.assign(blkRed.size() + 1, 0);
  auto blockOf = [&](int64_t l, int64_t o, int s) {
    return std::lower_bound(blkRed.begin() + lmBlk[l], blkRed.begin() + lmBlk[l + 1], obRed[o * 4 + s]) - blkRed.begin();
  };
  for (int64_t l = 0; l < nPts; l++)
    for (int64_t o = lmObs[l]; o < lmObs[l + 1]; o++)
      for (int s = 0; s < 4; s++)
        if (obRed[o * 4 + s] >= 0) pan.bxStart[blockOf(l, o, s) + 1]++;
  for (size_t b = 0; b < blkRed.size(); b++) pan.bxStart[b + 1] += pan.bxStart[b];
  pan.bxEnt.assign(pan.bxStart[blkRed.size()], 0);
  {
    std::vector<int64_t> fill(pan.bxStart.begin(), pan.bxStart.end() - 1);
    if (nObs >= (int64_t(1) << 29)) return {VB_E_ARG, "too many visual observations (2^29)"};
    for (int64_t l = 0; l < nPts; l++)
      for (int64_t o = lmObs[l]; o < lmObs[l + 1]; o++)
        for (int s = 0; s < 4; s++)
          if (obRed[o * 4 + s] >= 0) pan.bxEnt[fill[blockOf(l, o, s)]++] = (int32_t)((o << 2) | s);
  }
  // incidence lists O(X), L(X)
  std::vector<int64_t>&oxStart = pan.oxStart, &lxStart = pan.lxStart;
  oxStart.assign(nRV + 1, 0), lxStart.assign(nRV + 1, 0);
  for (int64_t o = 0; o < nObs; o++)
    for (int s = 0; s < 4; s++)
      if (obRed[o * 4 + s] >= 0) oxStart[obRed[o * 4 + s] + 1]++;
  for (int64_t b = 0; b < (int64_t)blkRed.size(); b++) lxStart[blkRed[b] + 1]++;
  for (int i = 0; i < nRV; i++) oxStart[i + 1] += oxStart[i], lxStart[i + 1] += lxStart[i];
  pan.oxObs.assign(oxStart[nRV], 0), pan.oxSlot.assign(oxStart[nRV], 0);
  pan.lxLm.assign(lxStart[nRV], 0), pan.lxCol.assign(lxStart[nRV], 0);
  {
    std::vector<int64_t> fo(oxStart.begin(), oxStart.end() - 1), fl(lxStart.begin(), lxStart.end() - 1);
    for (int64_t o = 0; o < nObs; o++)
      for (int s = 0; s < 4; s++) {
        const int32_t r = obRed[o * 4 + s];
        if (r < 0) continue;
        pan.oxObs[fo[r]] = (int32_t)o, pan.oxSlot[fo[r]] = s, fo[r]++;
      }
    for (int64_t l = 0; l < nPts; l++)
      for (int64_t b = lmBlk[l]; b < lmBlk[l + 1]; b++) {
        const int32_t r = blkRed[b];
        pan.lxLm[fl[r]] = (int32_t)l, pan.lxCol[fl[r]] = blkCol[b], fl[r]++;
      }
  }
  // L(X) in chunks of <= 1024 landmarks (reduced_rhs_kernel)
  pan.lxChunk.clear();
  for (int i = 0; i < nRV; i++)
    for (int64_t b = lxStart[i]; b < lxStart[i + 1]; b += 1024)
      pan.lxChunk.insert(pan.lxChunk.end(), {i, b, std::min<int64_t>(b + 1024, lxStart[i + 1])});
  return {};
}

// ---------------------------------------------------------------- 8. this handle's landmark shard
Status shardRanges(const Input& in, const Layout& lay, const std::vector<int>& lmRank, const Observations& obs,
                   const Panels& pan, Shard& shard) {
  const int64_t nPts = (int64_t)obs.lmObs.size() - 1, nObs = obs.nObs;
  shard.lmBegin = in.lmBegin, shard.lmEnd = in.lmEnd, shard.isRoot = in.isRoot;
  if (in.partSet) {  // partition mode: this rank's landmarks and constant-point observations
    int64_t a = 0;
    while (a < nPts && lmRank[a] < in.partRank) a++;
    int64_t b = a;
    while (b < nPts && lmRank[b] == in.partRank) b++;
    shard.lmBegin = a, shard.lmEnd = b, shard.isRoot = in.partRank == 0;
  }
  if (shard.lmEnd < 0) shard.lmBegin = 0, shard.lmEnd = nPts;
  if (shard.lmBegin < 0 || shard.lmEnd > nPts || shard.lmBegin > shard.lmEnd) return {VB_E_ARG, "bad landmark shard range"};
  // landmark lists by panel width (landmark.hip landmark_stage_kernel)
  std::vector<int32_t> big;
  int64_t bigCols = 0;
  shard.lmList.clear(), shard.loneList.clear();
  for (int64_t l = shard.lmBegin; l < shard.lmEnd; l++) {
    if (obs.lmObs[l + 1] == obs.lmObs[l]) {  // only base-map factors see it
      shard.loneList.push_back((int32_t)l);
      continue;
    }
    const int64_t nc = (pan.lmY[l + 1] - pan.lmY[l]) / 3;
    if (nc <= kLmSmallCols) shard.lmList.push_back((int32_t)l);
    else big.push_back((int32_t)l), bigCols = std::max(bigCols, nc);
  }
  shard.nLmSmall = (int64_t)shard.lmList.size(), shard.nLmBig = (int64_t)big.size(), shard.lmBigCols = (int32_t)bigCols;
  shard.lmList.insert(shard.lmList.end(), big.begin(), big.end());
  shard.obB = obs.lmObs[shard.lmBegin], shard.obE = obs.lmObs[shard.lmEnd], shard.obFree = obs.lmObs[nPts];
  // constant-point observations of this handle: [fB, fE) (the root's whole tail unless partitioned)
  shard.fB = shard.obFree, shard.fE = shard.isRoot ? nObs : shard.obFree;
  if (in.partSet) {
    int64_t a = shard.obFree;
    while (a < nObs && obsOwner(in, lay, obs.perm[a]) < in.partRank) a++;
    int64_t b = a;
    while (b < nObs && obsOwner(in, lay, obs.perm[b]) == in.partRank) b++;
    shard.fB = a, shard.fE = b;
  }
  return {};
}

// ---------------------------------------------------------------- 9. couplings: row ends, the tile pattern,
// its symbolic Cholesky fill, the tile index by column and by row, the columns' elimination levels
void tilePattern(const Input& in, const Layout& lay, const Observations& obs, const Panels& pan, Pattern& pat) {
  const int nRV = lay.nRV;
  const int32_t nT = lay.nT;
  const int64_t nPts = (int64_t)obs.lmObs.size() - 1;
  pat.rowEnd.resize(nRV);
  for (int i = 0; i < nRV; i++) pat.rowEnd[i] = lay.rvOff[i] + lay.rvDim[i];
  // per tile: 3 written by a direct term (damping, visual groups, small factors), 1 landmark (Schur)
  // terms only, 2 fill (zero in S; the PCG product skips it)
  std::vector<uint8_t> mark((size_t)nT * nT, 0);
  auto coupleBlocks = [&](int a, int b) {  // reduced ids; a, b any order
    if (lay.rvOff[a] < lay.rvOff[b]) std::swap(a, b);
    pat.rowEnd[b] = std::max(pat.rowEnd[b], lay.rvOff[a] + lay.rvDim[a]);
    for (int64_t I = tileLo(lay, a); I <= tileHi(lay, a); I++)
      for (int64_t J = tileLo(lay, b); J <= tileHi(lay, b); J++)
        if (I >= J) mark[I * nT + J] = 3;
  };
  for (int i = 0; i < nRV; i++) coupleBlocks(i, i);
  for (int64_t o = 0; o < obs.nObs; o++)
    for (int s = 0; s < 4; s++)
      for (int t = 0; t <= s; t++)
        if (obs.obRed[o * 4 + s] >= 0 && obs.obRed[o * 4 + t] >= 0) coupleBlocks(obs.obRed[o * 4 + s], obs.obRed[o * 4 + t]);
  for (int64_t l = 0; l < nPts; l++) {
    const int64_t b0 = pan.lmBlk[l], b1 = pan.lmBlk[l + 1];
    if (b1 == b0) continue;
    // row end: the suffix partner with the largest offset is the last block
    const int last = pan.blkRed[b1 - 1];
    for (int64_t b = b0; b < b1; b++)
      pat.rowEnd[pan.blkRed[b]] = std::max(pat.rowEnd[pan.blkRed[b]], lay.rvOff[last] + lay.rvDim[last]);
    // tile pattern over the distinct tiles touched
    std::vector<int64_t> touched;
    for (int64_t b = b0; b < b1; b++)
      for (int64_t t = tileLo(lay, pan.blkRed[b]); t <= tileHi(lay, pan.blkRed[b]); t++) touched.push_back(t);
    std::sort(touched.begin(), touched.end());
    touched.erase(std::unique(touched.begin(), touched.end()), touched.end());
    for (size_t a = 0; a < touched.size(); a++)
      for (size_t b = 0; b <= a; b++) {
        uint8_t& q = mark[touched[a] * nT + touched[b]];
        q = q ? q : 1;
      }
  }
  for (int fk = 1; fk < 14; fk++) {
    const int nv = kNumVars[fk];
    const int64_t n = (int64_t)in.fint[fk].size();
    for (int64_t f = 0; f < n; f++)
      for (int s = 0; s < nv; s++)
        for (int t = 0; t <= s; t++) {
          const int kindS = kFK[fk][s], kindT = kFK[fk][t];
          const int hs = in.fvars[fk][f * nv + s], ht = in.fvars[fk][f * nv + t];
          if (hs < 0 || ht < 0 || kindS == 8 || kindT == 8 || kindS == 0 || kindT == 0) continue;
          if (lay.redOf[kindS][hs] < 0 || lay.redOf[kindT][ht] < 0) continue;
          coupleBlocks(lay.redOf[kindS][hs], lay.redOf[kindT][ht]);
        }
  }
  // symbolic tile Cholesky (fill)
  for (int32_t J = 0; J < nT; J++) {
    std::vector<int32_t> rows;
    for (int32_t I = J + 1; I < nT; I++)
      if (mark[(size_t)I * nT + J]) rows.push_back(I);
    for (size_t a = 0; a < rows.size(); a++)
      for (size_t b = 0; b <= a; b++) {
        uint8_t& q = mark[(size_t)rows[a] * nT + rows[b]];
        q = q ? q : 2;
      }
  }
  pat.tileIdx.assign((size_t)nT * nT, -1);
  pat.tileFill.clear(), pat.tileDirect.clear();
  pat.colStart.assign(nT + 1, 0);
  pat.colTiles.clear(), pat.colRows.clear();
  pat.nTiles = 0;
  for (int32_t J = 0; J < nT; J++) {
    for (int32_t I = J; I < nT; I++)
      if (I == J || mark[(size_t)I * nT + J]) {
        pat.tileIdx[(size_t)I * nT + J] = (int32_t)pat.nTiles;
        pat.tileFill.push_back(I != J && mark[(size_t)I * nT + J] == 2 ? 1 : 0);
        pat.tileDirect.push_back(I == J || mark[(size_t)I * nT + J] == 3 ? 1 : 0);
        pat.colTiles.push_back((int32_t)pat.nTiles++);
        pat.colRows.push_back(I);
      }
    pat.colStart[J + 1] = (int64_t)pat.colTiles.size();
  }
  pat.rowStart.assign(nT + 1, 0);
  pat.rowTiles.clear(), pat.rowCol.clear();
  for (int32_t J = 0; J < nT; J++) {
    for (int32_t K = 0; K < J; K++)
      if (pat.tileIdx[(size_t)J * nT + K] >= 0) pat.rowTiles.push_back(pat.tileIdx[(size_t)J * nT + K]), pat.rowCol.push_back(K);
    pat.rowStart[J + 1] = (int64_t)pat.rowTiles.size();
  }
  // level schedule of the tile Cholesky: a column's level is one more than the levels of the columns
  // that update it (its row tiles); the columns of one level are independent
  pat.level.assign(nT, 0);
  pat.nLevels = 0;
  for (int32_t J = 0; J < nT; J++) {
    for (int64_t i = pat.rowStart[J]; i < pat.rowStart[J + 1]; i++) pat.level[J] = std::max(pat.level[J], pat.level[pat.rowCol[i]] + 1);
    pat.nLevels = std::max(pat.nLevels, pat.level[J] + 1);
  }
  pat.levelCols.assign(pat.nLevels, {});
  for (int32_t J = 0; J < nT; J++) pat.levelCols[pat.level[J]].push_back(J);
}

// ---------------------------------------------------------------- 10. Schur assembly work by target tile
// (this shard's landmarks and observations)
namespace {
// landmark entries by target tile, a tile's in runs of identical (maskI, maskJ) (schur.hip
// schur_run4_kernel), by landmark within a run; entStart: per tile into ents
Status tileEntries(const Layout& lay, const Panels& pan, const Shard& shard, const Pattern& pat,
                   std::vector<int64_t>& entStart, std::vector<TileEnt>& ents) {
  const int32_t nT = lay.nT;
  struct Seg { int64_t t, c0, c1; };
  std::vector<Seg> segs;
  auto segments = [&](int64_t l) {  // panel columns split by the tile their reduced row falls in
    segs.clear();
    const int64_t cb = pan.lmY[l] / 3, nc = (pan.lmY[l + 1] - pan.lmY[l]) / 3;
    for (int64_t c = 0; c < nc; c++) {
      const int64_t t = pan.pcRow[cb + c] / TS;
      if (segs.empty() || segs.back().t != t) segs.push_back({t, c, c + 1});
      else segs.back().c1 = c + 1;
    }
  };
  entStart.assign(pat.nTiles + 1, 0);
  for (int64_t l = shard.lmBegin; l < shard.lmEnd; l++) {
    segments(l);
    for (size_t a = 0; a < segs.size(); a++)
      for (size_t b = 0; b <= a; b++) {
        const int32_t ti = pat.tileIdx[(size_t)segs[a].t * nT + segs[b].t];
        if (ti < 0) return {VB_E_STATE, "internal: landmark tile outside the symbolic structure"};
        entStart[ti + 1]++;
      }
  }
  for (int64_t t = 0; t < pat.nTiles; t++) entStart[t + 1] += entStart[t];
  ents.assign(entStart[pat.nTiles], TileEnt());
  std::vector<int64_t> cur(entStart.begin(), entStart.end() - 1);
  for (int64_t l = shard.lmBegin; l < shard.lmEnd; l++) {
    segments(l);
    const int64_t cb = pan.lmY[l] / 3;
    for (size_t a = 0; a < segs.size(); a++)
      for (size_t b = 0; b <= a; b++) {
        const int32_t ti = pat.tileIdx[(size_t)segs[a].t * nT + segs[b].t];
        TileEnt& e = ents[cur[ti]++];
        e.colI = (uint32_t)(cb + segs[a].c0), e.nI = (uint16_t)(segs[a].c1 - segs[a].c0);
        e.colJ = (uint32_t)(cb + segs[b].c0), e.nJ = (uint16_t)(segs[b].c1 - segs[b].c0);
        e.lm = (uint32_t)l;
        e.maskI = e.maskJ = 0;
        for (int64_t c = segs[a].c0; c < segs[a].c1; c++) e.maskI |= 1ull << (pan.pcRow[cb + c] % TS);
        for (int64_t c = segs[b].c0; c < segs[b].c1; c++) e.maskJ |= 1ull << (pan.pcRow[cb + c] % TS);
      }
  }
  for (int64_t t = 0; t < pat.nTiles; t++)
    std::sort(ents.begin() + entStart[t], ents.begin() + entStart[t + 1], [](const TileEnt& a, const TileEnt& b) {
      if (a.maskI != b.maskI) return a.maskI < b.maskI;
      if (a.maskJ != b.maskJ) return a.maskJ < b.maskJ;
      return a.lm < b.lm;
    });
  return {};
}

// observation groups: this shard's observations by their 4 reduced blocks (rig, camera); touched: the
// tiles a group writes
void observationGroups(const Layout& lay, const Observations& obs, const Shard& shard, const Pattern& pat,
                       SchurWork& schur, std::vector<uint8_t>& touched) {
  const int32_t nT = lay.nT;
  std::vector<int32_t>& grpObs = schur.grpObs;
  grpObs.clear(), schur.grpStart.clear(), schur.grpRed.clear();
  for (int64_t o = 0; o < obs.nObs; o++)
    if ((o >= shard.obB && o < shard.obE) || (o >= shard.fB && o < shard.fE)) grpObs.push_back((int32_t)o);
  auto key = [&](int32_t o, int s) { return obs.obRed[(int64_t)o * 4 + s]; };
  std::stable_sort(grpObs.begin(), grpObs.end(), [&](int32_t a, int32_t b) {
    for (int s = 0; s < 4; s++)
      if (key(a, s) != key(b, s)) return key(a, s) < key(b, s);
    return false;
  });
  for (size_t i = 0; i < grpObs.size(); i++) {
    bool fresh = i == 0;
    for (int s = 0; s < 4 && !fresh; s++) fresh = key(grpObs[i], s) != key(grpObs[i - 1], s);
    if (!fresh) continue;
    schur.grpStart.push_back((int64_t)i);
    for (int s = 0; s < 4; s++) schur.grpRed.push_back(key(grpObs[i], s));
    for (int s = 0; s < 4; s++)  // tiles the group touches (for the shard's tile band)
      for (int t = 0; t <= s; t++) {
        int32_t A = key(grpObs[i], s), B = key(grpObs[i], t);
        if (A < 0 || B < 0) continue;
        if (lay.rvOff[A] < lay.rvOff[B]) std::swap(A, B);
        for (int64_t I = tileLo(lay, A); I <= tileHi(lay, A); I++)
          for (int64_t J = tileLo(lay, B); J <= std::min<int64_t>(I, tileHi(lay, B)); J++) {
            const int32_t tile = pat.tileIdx[(size_t)I * nT + J];
            if (tile >= 0) touched[tile] = 1;
          }
      }
  }
  schur.grpStart.push_back((int64_t)grpObs.size());
}

// per item: its runs of identical (maskI, maskJ) and its tasks (run, chunk of <= kSchurCh landmarks,
// kSchurTR compact block rows), dealt to the 4 waves longest-first by an MFMA + gather cost model and
// kept in (run, chunk) order per wave, so a wave rebuilds its row maps only when its run changes
// (schur_run4_kernel: no run scan, no per-run global mask reads, balanced waves)
void runsAndTasks(SchurWork& schur) {
  const std::vector<TileEnt>& ents = schur.ents;
  schur.runs.clear(), schur.tasks.clear();
  for (TileWork& w : schur.works) {
    const bool diag = w.I == w.J;
    std::vector<int> runBegin;
    for (int e = 0; e < w.count; e++) {
      const TileEnt& a = ents[w.start + e];
      if (e == 0 || a.maskI != ents[w.start + e - 1].maskI || a.maskJ != ents[w.start + e - 1].maskJ) runBegin.push_back(e);
    }
    runBegin.push_back(w.count);
    w.runFirst = (int32_t)(schur.runs.size() / 2), w.nRuns = (uint16_t)(runBegin.size() - 1);
    struct Task {
      uint32_t code;
      double cost;
    };
    std::vector<Task> itemTasks;
    for (size_t r = 0; r + 1 < runBegin.size(); r++) {
      const uint64_t mI = ents[w.start + runBegin[r]].maskI, mJ = diag ? mI : ents[w.start + runBegin[r]].maskJ;
      schur.runs.push_back(mI), schur.runs.push_back(mJ);
      const int nbI = (__builtin_popcountll(mI) + 15) / 16, nbJ = (__builtin_popcountll(mJ) + 15) / 16;
      for (int c0 = runBegin[r]; c0 < runBegin[r + 1]; c0 += kSchurCh)
        for (int a0 = 0; a0 < nbJ; a0 += kSchurTR) {
          const int nl = std::min(kSchurCh, runBegin[r + 1] - c0), nr = std::min(kSchurTR, nbJ - a0);
          // plane groups of four landmarks (schur_task): three k-steps and two loads per operand block each
          const int ng = (nl + 3) / 4;
          int mf = 0;
          for (int i = 0; i < nr; i++)
            for (int b = 0; b < nbI; b++) mf += (!diag || a0 + i <= b) ? 1 : 0;
          const double cost = ng * (48.0 * mf + 6.0 * (nr + nbI)) + 6.0 * mf + 24.0 + (diag && a0 == 0 ? 6.0 * nl : 0.0);
          itemTasks.push_back({(uint32_t)r | ((uint32_t)c0 << 8) | ((uint32_t)nl << 16) | ((uint32_t)a0 << 22), cost});
        }
    }
    std::stable_sort(itemTasks.begin(), itemTasks.end(), [](const Task& a, const Task& b) { return a.cost > b.cost; });
    std::vector<uint32_t> perWave[4];
    double load[4] = {0, 0, 0, 0};
    for (const Task& t : itemTasks) {
      const int k = (int)(std::min_element(load, load + 4) - load);
      load[k] += t.cost, perWave[k].push_back(t.code);
    }
    w.taskFirst = (int32_t)schur.tasks.size();
    for (int k = 0; k < 4; k++) {
      std::sort(perWave[k].begin(), perWave[k].end(), [](uint32_t a, uint32_t b) {
        return (a & 0xffffu) != (b & 0xffffu) ? (a & 0xffffu) < (b & 0xffffu) : a < b;  // run, chunk, row
      });
      w.wOff[k] = (uint16_t)(schur.tasks.size() - w.taskFirst);
      schur.tasks.insert(schur.tasks.end(), perWave[k].begin(), perWave[k].end());
    }
    w.wOff[4] = (uint16_t)(schur.tasks.size() - w.taskFirst);
  }
}

// diagnostics: compact widths, MFMA padding, runs, tasks
void printSchurStats(const SchurWork& schur) {
  const std::vector<TileEnt>& ents = schur.ents;
  const std::vector<uint64_t>& runsH = schur.runs;
  const std::vector<uint32_t>& tasksH = schur.tasks;
  int64_t hI[5] = {0}, hJ[5] = {0}, nRun = 0, nTask = 0, runLm = 0;
  double useful = 0, issued = 0, issued4 = 0, gathered = 0, segBytes = 0;
  double nlHist[17] = {0}, kDense = 0, kGroup = 0, gDense = 0, gGroup = 0;
  auto bin = [](int n) { return n <= 4 ? 0 : n <= 8 ? 1 : n <= 16 ? 2 : n <= 32 ? 3 : 4; };
  for (const TileWork& w : schur.works) {
    const bool diag = w.I == w.J;
    std::vector<int> rlen(w.nRuns, 0);
    for (int e = 0, k = -1; e < w.count; e++) {
      const TileEnt& a = ents[w.start + e];
      if (e == 0 || a.maskI != ents[w.start + e - 1].maskI || a.maskJ != ents[w.start + e - 1].maskJ) k++;
      rlen[k]++;
    }
    for (int r = 0; r < w.nRuns; r++) {
      const uint64_t mI = runsH[2 * ((size_t)w.runFirst + r)], mJ = runsH[2 * ((size_t)w.runFirst + r) + 1];
      const int nI = __builtin_popcountll(mI), nJ = __builtin_popcountll(mJ);
      const int nl = rlen[r];
      hI[bin(nI)]++, hJ[bin(nJ)]++, nRun++, runLm += nl;
      const double rows = 3.0 * nl;
      useful += 2.0 * rows * nI * nJ * (diag ? 0.5 : 1.0);
      const int nbI = (nI + 15) / 16, nbJ = (nJ + 15) / 16;
      issued += 2.0 * 4.0 * std::ceil(rows / 4.0) * 256.0 * nbI * nbJ * (diag ? 0.5 : 1.0);
      issued4 += 2.0 * 4.0 * std::ceil(rows / 4.0) * 16.0 * ((nI + 3) / 4) * ((nJ + 3) / 4) * (diag ? 0.5 : 1.0);
    }
    nTask += w.wOff[4];
    for (int t = 0; t < w.wOff[4]; t++) {  // gathered operand bytes: every k-step's NR + NBI 16-wide rows
      const uint32_t code = tasksH[(size_t)w.taskFirst + t];
      const int r = code & 255, nl = (code >> 16) & 63, a0 = (code >> 22) & 3;
      const uint64_t mI = runsH[2 * ((size_t)w.runFirst + r)], mJ = runsH[2 * ((size_t)w.runFirst + r) + 1];
      const int nbI = (__builtin_popcountll(mI) + 15) / 16, nbJ = (__builtin_popcountll(mJ) + 15) / 16;
      const int nr = std::min(kSchurTR, nbJ - a0);
      gathered += 4.0 * ((3 * nl + 3) / 4) * (nr + nbI) * 16 * sizeof(rec_t);
      // k-steps and gather instructions of the dense K mapping (3 rows per landmark, 4 per k-step) against a
      // plane-grouped one (each lane group one landmark's 3 planes over 3 k-steps, the remainder dense)
      int mf = 0;
      for (int i = 0; i < nr; i++)
        for (int b = 0; b < nbI; b++) mf += (!diag || a0 + i <= b) ? 1 : 0;
      const int ksD = (3 * nl + 3) / 4, ksG = 3 * (nl / 4) + (3 * (nl % 4) + 3) / 4;
      nlHist[std::min(nl, 16)] += 1.0, kDense += (double)ksD * mf, kGroup += (double)ksG * mf;
      gDense += (double)ksD * (nr + nbI), gGroup += (double)((nl / 4) * 2 + (3 * (nl % 4) + 3) / 4) * (nr + nbI);
    }
    for (int e = 0; e < w.count; e++) {  // the entries' Y segments once per item
      const TileEnt& a = ents[w.start + e];
      segBytes += 3.0 * (__builtin_popcountll(a.maskI) + (diag ? 0 : __builtin_popcountll(a.maskJ))) * sizeof(rec_t);
    }
  }
  fprintf(stderr,
          "[schur stats] items %zu runs %lld tasks %lld landmarks/run %.2f; nI <=4/8/16/32/64: %lld %lld %lld %lld "
          "%lld; nJ: %lld %lld %lld %lld %lld; GFLOP useful %.2f issued(16x16) %.2f issued(4x4) %.2f; GB gathered %.2f, "
          "entry segments %.2f\n",
          schur.works.size(), (long long)nRun, (long long)nTask, (double)runLm / std::max<int64_t>(1, nRun),
          (long long)hI[0], (long long)hI[1], (long long)hI[2], (long long)hI[3], (long long)hI[4], (long long)hJ[0],
          (long long)hJ[1], (long long)hJ[2], (long long)hJ[3], (long long)hJ[4], useful * 1e-9, issued * 1e-9,
          issued4 * 1e-9, gathered * 1e-9, segBytes * 1e-9);
  fprintf(stderr, "[schur stats] tasks by landmarks:");
  for (int k = 1; k <= 16; k++) fprintf(stderr, " %d:%.0f", k, nlHist[k]);
  fprintf(stderr, "; MFMAs dense K %.3g, plane-grouped K %.3g; gather instructions dense %.3g, plane-grouped %.3g\n",
          kDense, kGroup, gDense, gGroup);
}
}  // namespace

Status schurWork(const Input& in, const Layout& lay, const Observations& obs, const Panels& pan, const Shard& shard,
                 const Pattern& pat, SchurWork& schur) {
  const int64_t nTiles = pat.nTiles;
  std::vector<int64_t> entStart;
  if (Status e = tileEntries(lay, pan, shard, pat, entStart, schur.ents)) return e;
  std::vector<uint8_t> touched(nTiles, 0);  // tiles this shard's partial system writes
  observationGroups(lay, obs, shard, pat, schur, touched);
  // work items: a tile's landmark entries in near-equal chunks of at most kChunkLm; `kind` = 1 when
  // the tile is split over several items (fp64 atomics), else the item owns the tile (plain RMW).
  // Items run in tile-column order (xcd_block hands each XCD a contiguous range of them; by the median
  // landmark of their entries instead: 52.7 against 52.9 it/s, r05).  Longest-first is unnecessary:
  // chunks are bounded; column order keeps the locality of Y / records.
  const int64_t kChunkLm = 256;
  std::vector<TileWork>& works = schur.works;
  works.clear();
  std::vector<int32_t> itemsPerTile(nTiles, 0);
  for (int32_t J = 0; J < lay.nT; J++)
    for (int64_t c = pat.colStart[J]; c < pat.colStart[J + 1]; c++) {
      const int32_t ti = pat.colTiles[c];
      const int64_t e0 = entStart[ti], n = entStart[ti + 1] - e0, nch = (n + kChunkLm - 1) / kChunkLm;
      for (int64_t k = 0; k < nch; k++) {
        TileWork w{};
        const int64_t s0 = n * k / nch, s1 = n * (k + 1) / nch;
        w.tile = ti, w.I = pat.colRows[c], w.J = J, w.count = (int32_t)(s1 - s0);
        w.start = e0 + s0, w.kind = 0;
        works.push_back(w);
        itemsPerTile[ti]++;
        touched[ti] = 1;
      }
    }
  for (TileWork& w : works) w.kind = itemsPerTile[w.tile] > 1 ? 1 : 0;
  // a tile written by exactly one Schur item and by no direct term is stored whole by that item (kind
  // 2: no read of the tile) and left out of the clear in vb_linearize (single handle; shards and
  // partitions clear their tile ranges and add); the clear covers the rest, by tile list
  schur.hasClear = !in.sharded && !in.partSet;
  schur.clearTiles.clear();
  if (schur.hasClear) {
    for (TileWork& w : works)
      if (w.kind == 0 && !pat.tileDirect[w.tile]) w.kind = 2;
    std::vector<uint8_t> stored(nTiles, 0);
    for (const TileWork& w : works)
      if (w.kind == 2) stored[w.tile] = 1;
    for (int64_t t = 0; t < nTiles; t++)
      if (!stored[t]) schur.clearTiles.push_back((int32_t)t);
  }
  runsAndTasks(schur);
  if (in.knobs.stats) printSchurStats(schur);
  // tiles this shard's partial system can touch: the enclosing range (vb_shard_tile_range) and the
  // exact set (vb_shard_tiles: landmark and observation-group targets; the root, which also holds
  // the small factors and the damping, receives rather than sends)
  int64_t lo = INT64_MAX, hi = -1;
  for (int64_t t = 0; t < nTiles; t++)
    if (touched[t]) lo = std::min(lo, t), hi = t;
  if (shard.isRoot) schur.tileFirst = 0, schur.tileCount = nTiles;
  else if (hi < 0) schur.tileFirst = 0, schur.tileCount = 0;
  else schur.tileFirst = lo, schur.tileCount = hi - lo + 1;
  schur.shardTiles.clear();
  if (!shard.isRoot)
    for (int64_t t = 0; t < nTiles; t++)
      if (touched[t]) schur.shardTiles.push_back((int32_t)t);
  return {};
}

// ---------------------------------------------------------------- 11. / 12. the schedules' column selections
Select selectAll(int32_t nT) {
  Select s;
  s.col.assign(nT, 1), s.tgt.assign(nT, 1), s.src.assign(nT, 1), s.pre.assign(nT, 0);
  return s;
}
// a rank's subtree: its columns, fan-in also into the ROOT targets, the ROOT rows known before its
// backward solve
Select selectRank(const std::vector<int8_t>& colOwner, int rank, int world) {
  Select s = selectAll((int32_t)colOwner.size());
  for (size_t J = 0; J < colOwner.size(); J++) {
    const bool own = colOwner[J] == rank, root = colOwner[J] == world;
    s.col[J] = own, s.tgt[J] = own || root, s.src[J] = own, s.pre[J] = root;
  }
  return s;
}
Select selectRoot(const std::vector<int8_t>& colOwner, int world) {
  Select s = selectAll((int32_t)colOwner.size());
  for (size_t J = 0; J < colOwner.size(); J++) s.col[J] = s.tgt[J] = s.src[J] = colOwner[J] == world;
  return s;
}

namespace {
// fan-in contributions by target tile: column K's pair (qi >= qk) of off-diagonal tiles updates the
// target tile (row qi, row qk) with L_{qi,K} L_{qk,K}^T.  Counting sort by target tile over the source
// columns in `sources` order (level order, so every target's list runs from old to new columns);
// skipFirst[K]: leave out K's contributions into its first off-diagonal row's column (pair-internal).
// start: nTiles + 1 offsets into pairs (2 per contribution: tile (qi, K), tile (qk, K)).
Status fanInPairs(const Pattern& pat, int32_t nT, const Select& sel, const std::vector<int32_t>& sources,
                  const std::vector<int8_t>* skipFirst, std::vector<int64_t>& start, std::vector<int32_t>& pairs) {
  start.assign(pat.nTiles + 1, 0);
  pairs.clear();
  for (int pass = 0; pass < 2; pass++) {
    std::vector<int64_t> pos;
    if (pass == 1) {
      for (int64_t t = 0; t < pat.nTiles; t++) start[t + 1] += start[t];
      pos.assign(start.begin(), start.end() - 1);
      pairs.assign(2 * (size_t)start[pat.nTiles], 0);
    }
    for (int32_t K : sources) {
      if (!sel.src[K]) continue;
      const int64_t c0 = pat.colStart[K], n = pat.colStart[K + 1] - c0;
      for (int64_t qi = 1; qi < n; qi++)
        for (int64_t qk = 1; qk <= qi; qk++) {
          if (skipFirst && (*skipFirst)[K] == 1 && qk == 1) continue;
          if (!sel.tgt[pat.colRows[c0 + qk]]) continue;
          const int32_t t = pat.tileIdx[(size_t)pat.colRows[c0 + qi] * nT + pat.colRows[c0 + qk]];
          if (t < 0) return {VB_E_STATE, "internal: symbolic fill incomplete"};
          if (pass == 0) {
            start[t + 1]++;
          } else {
            const int64_t at = pos[t]++;
            pairs[2 * at] = pat.colTiles[c0 + qi], pairs[2 * at + 1] = pat.colTiles[c0 + qk];
          }
        }
    }
  }
  if (start[pat.nTiles] >= INT32_MAX) return {VB_E_STATE, "tile Cholesky too large (contribution count)"};
  return {};
}

// a target tile's contribution list [start[t], start[t + 1]) cut into near-equal chunks of at most
// `chunk`: (tile, first, count, split) appended to fan
void fanChunks(int32_t t, const std::vector<int64_t>& start, int64_t chunk, std::vector<int32_t>& fan) {
  const int64_t b = start[t], m = start[t + 1] - b;
  if (m == 0) return;
  const int64_t nch = (m + chunk - 1) / chunk;
  for (int64_t k = 0; k < nch; k++) {
    const int64_t s0 = b + m * k / nch, s1 = b + m * (k + 1) / nch;
    fan.insert(fan.end(), {t, (int32_t)s0, (int32_t)(s1 - s0), nch > 1 ? 1 : 0});
  }
}

// longest chunks first within each XCD's contiguous range of the launch (kernel_common.hpp xcd_block: the
// dispatcher hands them out in order, LPT): +0.9%
void sortChunksPerXcd(std::vector<int32_t>& fan, size_t first) {
  std::vector<std::array<int32_t, 4>> q((fan.size() / 4) - first);
  for (size_t i = 0; i < q.size(); i++)
    for (int k = 0; k < 4; k++) q[i][k] = fan[4 * (first + i) + k];
  const size_t nq = q.size(), each = nq / 8, extra = nq % 8;
  for (size_t x = 0, b0 = 0; x < 8; x++) {
    const size_t len = each + (x < extra ? 1 : 0);
    std::stable_sort(q.begin() + b0, q.begin() + b0 + len, [](const auto& a, const auto& b) { return a[2] > b[2]; });
    b0 += len;
  }
  for (size_t i = 0; i < q.size(); i++)
    for (int k = 0; k < 4; k++) fan[4 * (first + i) + k] = q[i][k];
}

int64_t contributionsInto(const Pattern& pat, const std::vector<int64_t>& start, int32_t J) {
  int64_t n = 0;
  for (int64_t c = pat.colStart[J]; c < pat.colStart[J + 1]; c++) n += start[pat.colTiles[c] + 1] - start[pat.colTiles[c]];
  return n;
}
}  // namespace

// ---------------------------------------------------------------- 11. column schedule: per level one
// batched fan-in, potrf and trsm launch (or one fused potrf + trsm), and the fan-out solve task lists
Status columnSchedule(const Pattern& pat, int32_t nT, const Select& sel, int64_t ptFuseMax, SchedHost& S) {
  const int32_t nLev = pat.nLevels;
  const int64_t fanWgs = 3072;  // re-tuned for the thin-separator order (2048: -0.5%, 4096-8192: -0.3%)
  std::vector<int32_t> sources;
  for (int32_t L = 0; L < nLev; L++) sources.insert(sources.end(), pat.levelCols[L].begin(), pat.levelCols[L].end());
  std::vector<int64_t> start;
  if (Status e = fanInPairs(pat, nT, sel, sources, nullptr, start, S.fanPairs)) return e;
  // per level: fan-in of the level's target tiles, then potrf of its diagonals, then trsm.  A
  // target's list is cut into near-equal chunks of at most `chunk` contributions, chosen per level so
  // the launch has ~fanWgs workgroups (>= 4 contributions per chunk: one per wave)
  S.lvP.assign(nLev + 1, 0), S.lvT.assign(nLev + 1, 0), S.lvU.assign(nLev + 1, 0), S.lvPF.assign(nLev + 1, 0);
  S.potrfTile.clear(), S.potrfCol.clear(), S.trsmDiag.clear(), S.trsmTarget.clear(), S.trsmCol.clear();
  S.trsmRow.clear(), S.upd.clear(), S.ptf.clear(), S.ptfDiag.clear();
  for (int32_t L = 0; L < nLev; L++) {
    int64_t total = 0;
    for (int32_t J : pat.levelCols[L])
      if (sel.tgt[J]) total += contributionsInto(pat, start, J);
    const int64_t chunk = std::min<int64_t>(32, std::max<int64_t>(4, (total + fanWgs - 1) / fanWgs));
    for (int32_t J : pat.levelCols[L]) {
      const int64_t c0 = pat.colStart[J], n = pat.colStart[J + 1] - c0;
      if (sel.col[J]) {
        S.potrfTile.push_back(pat.colTiles[c0]), S.potrfCol.push_back(J);
        for (int64_t q = 1; q < n; q++)
          S.trsmDiag.push_back(pat.colTiles[c0]), S.trsmTarget.push_back(pat.colTiles[c0 + q]), S.trsmCol.push_back(J),
              S.trsmRow.push_back(pat.colRows[c0 + q]);
      }
      if (!sel.tgt[J]) continue;
      for (int64_t q = 0; q < n; q++) fanChunks(pat.colTiles[c0 + q], start, chunk, S.upd);
    }
    sortChunksPerXcd(S.upd, (size_t)S.lvU[L]);
    S.lvP[L + 1] = (int64_t)S.potrfTile.size(), S.lvT[L + 1] = (int64_t)S.trsmTarget.size(), S.lvU[L + 1] = (int64_t)S.upd.size() / 4;
    if (ptFuseMax > 0 && S.lvP[L + 1] > S.lvP[L] && S.lvT[L + 1] - S.lvT[L] <= ptFuseMax)
      for (int32_t J : pat.levelCols[L]) {
        if (!sel.col[J]) continue;
        const int64_t c0 = pat.colStart[J], n = pat.colStart[J + 1] - c0;
        const int32_t diag = pat.colTiles[c0];
        if (n == 1) S.ptf.insert(S.ptf.end(), {diag, J, -1, -1, 1});
        for (int64_t q = 1; q < n; q++) S.ptf.insert(S.ptf.end(), {diag, J, pat.colTiles[c0 + q], pat.colRows[c0 + q], q == 1 ? 1 : 0});
        S.ptfDiag.insert(S.ptfDiag.end(), {diag, J});
      }
    S.lvPF[L + 1] = (int64_t)S.ptf.size() / 5;
  }
  S.nLevels = nLev, S.nPairs = start[pat.nTiles];
  // fan-out solve task lists, by elimination level: every task of a level only waits on tasks of
  // earlier levels (or the level's own diagonal task listed first), so the waves' in-flight window
  // spans all independent subtrees of the level
  S.tasksF.clear(), S.tasksB.clear(), S.preReady.clear();
  S.expF.assign(nT, 0), S.expB.assign(nT, 0);
  for (int32_t L = 0; L < nLev; L++)
    for (int32_t K : pat.levelCols[L]) {
      if (!sel.col[K]) continue;
      S.tasksF.insert(S.tasksF.end(), {K, -1});
      for (int64_t c = pat.colStart[K] + 1; c < pat.colStart[K + 1]; c++) S.tasksF.insert(S.tasksF.end(), {K, (int32_t)c});
      for (int64_t c = pat.rowStart[K]; c < pat.rowStart[K + 1]; c++) S.expF[K] += sel.src[pat.rowCol[c]] ? 1 : 0;
      S.expB[K] = (int32_t)(pat.colStart[K + 1] - pat.colStart[K] - 1);
    }
  for (int32_t L = nLev - 1; L >= 0; L--)
    for (int32_t J : pat.levelCols[L]) {
      const bool own = sel.col[J], known = sel.pre[J];
      if (own) S.tasksB.insert(S.tasksB.end(), {J, -1});
      if (known) S.preReady.push_back(J);
      if (!own && !known) continue;
      for (int64_t c = pat.rowStart[J]; c < pat.rowStart[J + 1]; c++)
        if (sel.col[pat.rowCol[c]]) S.tasksB.insert(S.tasksB.end(), {J, (int32_t)c});
    }
  S.nF = (int64_t)S.tasksF.size() / 2, S.nB = (int64_t)S.tasksB.size() / 2, S.nPreReady = (int64_t)S.preReady.size();
  S.nPtfDiag = (int64_t)S.ptfDiag.size() / 2;
  S.built = true;
  return {};
}

// diagnostics: the column levels, and the 2-column supernodes (J, J + 1) a single handle could pair
static void printFactorStats(const Pattern& pat, int32_t nT) {
  // pairable: J + 1 is J's first off-diagonal row (its parent) and J's other rows are all rows of J + 1
  std::vector<int8_t> pair(nT, 0);
  int64_t nPair = 0;
  for (int32_t J = 0; J + 1 < nT; J++) {
    if (pair[J] || (J > 0 && pair[J - 1] == 1)) continue;
    const int64_t a = pat.colStart[J], b = pat.colStart[J + 1], a2 = pat.colStart[J + 1], b2 = pat.colStart[J + 2];
    if (b - a < 2 || pat.colRows[a + 1] != J + 1) continue;
    bool sub = true;
    int64_t q = a2 + 1;
    for (int64_t c = a + 2; c < b && sub; c++) {
      while (q < b2 && pat.colRows[q] < pat.colRows[c]) q++;
      sub = q < b2 && pat.colRows[q] == pat.colRows[c];
    }
    if (sub) pair[J] = 1, pair[J + 1] = 2, nPair++;
  }
  std::vector<int32_t> slev(nT, 0);
  int32_t nSl = 0;
  for (int32_t J = 0; J < nT; J++) {
    int32_t lv = 0;
    auto rowsOf = [&](int32_t X) {
      for (int64_t i = pat.rowStart[X]; i < pat.rowStart[X + 1]; i++) {
        const int32_t K = pat.rowCol[i];
        if (pair[X] == 2 && K == X - 1) continue;  // internal to the supernode
        lv = std::max(lv, slev[K] + 1);
      }
    };
    if (pair[J] == 2) continue;
    rowsOf(J);
    if (pair[J] == 1) rowsOf(J + 1);
    slev[J] = lv;
    if (pair[J] == 1) slev[J + 1] = lv;
    nSl = std::max(nSl, lv + 1);
  }
  int64_t contrib = 0, internal = 0;
  for (int32_t K = 0; K < nT; K++) {
    const int64_t n = pat.colStart[K + 1] - pat.colStart[K];
    contrib += (n - 1) * n / 2;
    if (pair[K] == 1) internal += n - 1;  // targets in column K + 1 from K
  }
  fprintf(stderr, "[factor stats] tile columns %d levels %d; pairable 2-column supernodes %lld (%lld columns), "
                  "supernode levels %d; contributions %lld of which internal to pairs %lld\n",
          nT, pat.nLevels, (long long)nPair, (long long)(2 * nPair), nSl, (long long)contrib, (long long)internal);
  for (int32_t L = 0; L < pat.nLevels; L++) {
    int64_t c = 0, np = 0;
    for (int32_t J : pat.levelCols[L]) {
      const int64_t n = pat.rowStart[J + 1] - pat.rowStart[J];
      c += n, np += pair[J] ? 1 : 0;
    }
    fprintf(stderr, "[factor stats] level %d columns %zu (paired %lld) row tiles %lld\n", L, pat.levelCols[L].size(),
            (long long)np, (long long)c);
  }
}

// ---------------------------------------------------------------- 12. two-column supernode schedule
namespace {
// pair J with J + 1: J + 1 is J's first off-diagonal row (its parent) and every other row of J is a
// row of J + 1 (so the pair's rows are J + 1's), both in one nested-dissection part.  role: 0 a single
// column, 1 the first of a pair, 2 the second.
void pairColumns(const Pattern& pat, const std::vector<int8_t>& colOwner, int32_t nT, const Select& sel,
                 std::vector<int8_t>& role) {
  role.assign(nT, 0);
  for (int32_t J = 0; J + 1 < nT; J++) {
    if (role[J]) continue;
    const int64_t a = pat.colStart[J], b = pat.colStart[J + 1], a2 = pat.colStart[J + 1], b2 = pat.colStart[J + 2];
    if (b - a < 2 || pat.colRows[a + 1] != J + 1 || colOwner[J] != colOwner[J + 1] || !sel.col[J] || !sel.col[J + 1])
      continue;
    bool subset = true;
    int64_t q = a2 + 1;
    for (int64_t c = a + 2; c < b && subset; c++) {
      while (q < b2 && pat.colRows[q] < pat.colRows[c]) q++;
      subset = q < b2 && pat.colRows[q] == pat.colRows[c];
    }
    if (subset) role[J] = 1, role[J + 1] = 2;
  }
}

// Streams (nStreams > 1): the supernodes' elimination tree (parent: the supernode of the first row below
// it) cut into independent subtrees on separate streams, so one subtree's diagonal blocks and rows
// (latency-bound, a few workgroups) run beside another's fan-in instead of behind a level barrier of the
// whole chip.  The tree is split from its roots down, heaviest subtree first, until none outweighs
// 1/nStreams of the frontier by more than 15%; the frontier's subtrees go to the streams longest first.
// Their ancestors (the separators above the cut) follow the stream of their heaviest child and wait for
// the others' (segDep), so sibling separators also run side by side.  Weights: the fan-in contributions
// into a supernode's columns.  parent: per first column, the first column of the parent supernode, -1.
void assignStreams(const Pattern& pat, int32_t nT, const std::vector<int8_t>& role, const std::vector<int64_t>& start,
                   int nStreams, bool stats, std::vector<int32_t>& stream, std::vector<int32_t>& parent) {
  std::vector<int32_t> snOf(nT);
  std::vector<double> weight(nT, 0.0);
  std::vector<std::vector<int32_t>> kids(nT);
  for (int32_t J = 0; J < nT; J++) snOf[J] = role[J] == 2 ? J - 1 : J;
  for (int32_t J0 = 0; J0 < nT; J0++) {
    if (role[J0] == 2) continue;
    const int32_t Jl = role[J0] == 1 ? J0 + 1 : J0;
    if (pat.colStart[Jl + 1] - pat.colStart[Jl] > 1) parent[J0] = snOf[pat.colRows[pat.colStart[Jl] + 1]];
    for (int32_t J = J0; J <= Jl; J++) weight[J0] += (double)contributionsInto(pat, start, J);
  }
  std::vector<double> own(weight);
  for (int32_t J0 = 0; J0 < nT; J0++)  // parents come after their children in the elimination order
    if (role[J0] != 2 && parent[J0] >= 0) weight[parent[J0]] += weight[J0], kids[parent[J0]].push_back(J0);
  std::vector<int32_t> front;
  for (int32_t J0 = 0; J0 < nT; J0++)
    if (role[J0] != 2 && parent[J0] < 0) front.push_back(J0);
  std::vector<int8_t> top(nT, 0);
  for (int it = 0; it < 4 * nT && front.size() < 256; it++) {
    double tot = 0.0;
    size_t xi = 0;
    for (size_t i = 0; i < front.size(); i++) {
      tot += weight[front[i]];
      if (weight[front[i]] > weight[front[xi]]) xi = i;
    }
    const int32_t X = front[xi];
    if (weight[X] <= 1.15 * tot / nStreams || kids[X].empty()) break;
    top[X] = 1;
    front.erase(front.begin() + (ptrdiff_t)xi);
    front.insert(front.end(), kids[X].begin(), kids[X].end());
  }
  std::stable_sort(front.begin(), front.end(), [&](int32_t a, int32_t b) { return weight[a] > weight[b]; });
  std::vector<double> load(nStreams, 0.0);
  std::vector<int32_t> rootStream(nT, -1);
  for (int32_t X : front) {
    const int g = (int)(std::min_element(load.begin(), load.end()) - load.begin());
    load[g] += weight[X], rootStream[X] = g;
  }
  for (int32_t J0 = nT - 1; J0 >= 0; J0--)  // the frontier subtrees, parents first
    if (role[J0] != 2 && !top[J0]) stream[J0] = rootStream[J0] >= 0 ? rootStream[J0] : parent[J0] >= 0 ? stream[parent[J0]] : 0;
  for (int32_t J0 = 0; J0 < nT; J0++)  // the separators above the cut, children first
    if (role[J0] != 2 && top[J0]) {
      int32_t best = -1;
      for (int32_t C : kids[J0])
        if (best < 0 || weight[C] > weight[best]) best = C;
      stream[J0] = best >= 0 ? stream[best] : 0;
    }
  for (int32_t J0 = 0; J0 < nT; J0++)
    if (role[J0] == 1) stream[J0 + 1] = stream[J0];
  if (stats) {
    std::vector<double> gw(nStreams, 0.0), gt(nStreams, 0.0);
    std::vector<int> gs(nStreams, 0);
    for (int32_t J0 = 0; J0 < nT; J0++)
      if (role[J0] != 2) gw[stream[J0]] += own[J0], gs[stream[J0]]++, gt[stream[J0]] += top[J0] ? own[J0] : 0.0;
    for (int g = 0; g < nStreams; g++)
      fprintf(stderr, "[factor stats] stream %d: supernodes %d, contributions %.0f (%.0f above the cut)\n", g, gs[g], gw[g],
              gt[g]);
  }
}
}  // namespace

Status supernodeSchedule(const Pattern& pat, const std::vector<int8_t>& colOwner, int32_t nT, const Select& sel,
                         int nStreams, bool stats, SnSchedHost& S) {
  std::vector<int8_t>& role = S.pairRole;
  pairColumns(pat, colOwner, nT, sel, role);
  // supernode levels: one more than the levels of the supernodes of every row tile (pair-internal
  // (J + 1, J) excluded)
  std::vector<int32_t>& lev = S.level;
  lev.assign(nT, 0);
  int32_t nLev = 0;
  for (int32_t J = 0; J < nT; J++) {
    if (role[J] == 2) continue;
    int32_t lv = 0;
    for (int32_t X = J; X <= J + (role[J] == 1 ? 1 : 0); X++)
      for (int64_t i = pat.rowStart[X]; i < pat.rowStart[X + 1]; i++) {
        const int32_t K = pat.rowCol[i];
        if (X == J + 1 && K == J) continue;
        lv = std::max(lv, lev[K] + 1);
      }
    lev[J] = lv;
    if (role[J] == 1) lev[J + 1] = lv;
    nLev = std::max(nLev, lv + 1);
  }
  std::vector<std::vector<int32_t>> sup(nLev);  // first column of every supernode, by level
  for (int32_t J = 0; J < nT; J++)
    if (role[J] != 2) sup[lev[J]].push_back(J);
  // fan-in contributions by target tile, sources in level order, pair-internal ones left out
  std::vector<int32_t> sources;
  for (int32_t L = 0; L < nLev; L++)
    for (int32_t J0 : sup[L])
      for (int32_t K = J0; K <= J0 + (role[J0] == 1 ? 1 : 0); K++) sources.push_back(K);
  std::vector<int64_t> start;
  if (Status e = fanInPairs(pat, nT, sel, sources, &role, start, S.fanPairs)) return e;
  std::vector<int32_t>& stream = S.stream;
  stream.assign(nT, 0);
  std::vector<int32_t> parent(nT, -1);
  const int G = std::max(1, nStreams);
  if (G > 1) assignStreams(pat, nT, role, start, G, stats, stream, parent);
  // a stream's segment shares the chip with the other streams' segments of its level: the fan-in workgroup
  // target and the fused-level threshold are divided by their number
  std::vector<int> nActive(nLev, 0);
  for (int32_t L = 0; L < nLev; L++) {
    uint32_t m = 0;
    for (int32_t J0 : sup[L]) m |= 1u << stream[J0];
    nActive[L] = __builtin_popcount(m);
  }
  // levels with at most this many row items run snpotrf_trsm8_kernel (re-swept at two streams, r05an: 128 /
  // 512 the same, 1024 -1.7%)
  const int64_t fuseMax = 256;
  // fan-in workgroups per level launch, divided among the level's active streams (r05ao: 2048 / 4096 the
  // same, 6144 -0.8%)
  const int64_t fanTarget = 3072;
  S.upd.clear(), S.pot.clear(), S.row.clear(), S.fus.clear(), S.copy.clear();
  S.lvU.assign(1, 0), S.lvS.assign(1, 0), S.lvR.assign(1, 0), S.lvF.assign(1, 0);
  S.segG.clear(), S.segL.clear(), S.segDep.clear();
  S.nTwo = 0;
  auto tile = [&](int32_t I, int32_t J) { return pat.tileIdx[(size_t)I * nT + J]; };
  // segments: (stream, level), level-major; segDep: the other streams whose earlier segments this one
  // needs (streams of its supernodes' children)
  for (int32_t L = 0; L < nLev; L++)
    for (int g = 0; g < G; g++) {
      std::vector<int32_t> supL;
      uint32_t dep = 0;
      for (int32_t J0 : sup[L])
        if (stream[J0] == g) supL.push_back(J0);
      if (supL.empty()) continue;
      if (G > 1)
        for (int32_t J0 = 0; J0 < nT; J0++)
          if (role[J0] != 2 && parent[J0] >= 0 && stream[parent[J0]] == g && lev[parent[J0]] == L && stream[J0] != g)
            dep |= 1u << stream[J0];
      int64_t total = 0;
      for (int32_t J0 : supL)
        for (int32_t J = J0; J <= J0 + (role[J0] == 1 ? 1 : 0); J++) total += contributionsInto(pat, start, J);
      const int share = std::max(1, nActive[L]);
      const int64_t fanWgs = fanTarget / share;
      const int64_t chunk = std::min<int64_t>(32, std::max<int64_t>(4, (total + fanWgs - 1) / fanWgs));
      const size_t firstChunk = S.upd.size() / 4;
      int64_t nRowsL = 0;
      for (int32_t J0 : supL) {
        if (!sel.col[J0]) continue;
        const int32_t Jl = role[J0] == 1 ? J0 + 1 : J0;
        nRowsL += pat.colStart[Jl + 1] - pat.colStart[Jl] - 1;
      }
      const bool fused = nRowsL <= fuseMax / share;
      for (int32_t J0 : supL) {
        const bool two = role[J0] == 1;
        const int32_t J2 = two ? J0 + 1 : -1;
        for (int32_t J = J0; J <= (two ? J2 : J0); J++)
          for (int64_t c = pat.colStart[J]; c < pat.colStart[J + 1]; c++)
            if (sel.tgt[J]) fanChunks(pat.colTiles[c], start, chunk, S.upd);
        if (!sel.col[J0]) continue;
        const int32_t t11 = tile(J0, J0), t21 = two ? tile(J2, J0) : -1, t22 = two ? tile(J2, J2) : -1;
        S.nTwo += two ? 1 : 0;
        // rows below the supernode: those of its last column (a pair's first column has no others)
        const int32_t Jl = two ? J2 : J0;
        const int64_t r0 = pat.colStart[Jl] + 1, r1 = pat.colStart[Jl + 1];
        if (fused) {
          S.copy.insert(S.copy.end(), {t11, J0});
          if (two) S.copy.insert(S.copy.end(), {t22, J2, t21, nT + J0});
          if (r1 == r0) S.fus.insert(S.fus.end(), {t11, J0, t21, t22, -1, -1, -1, 1});
          for (int64_t c = r0; c < r1; c++) {
            const int32_t I = pat.colRows[c];
            S.fus.insert(S.fus.end(), {t11, J0, t21, t22, two ? tile(I, J0) : pat.colTiles[c], two ? pat.colTiles[c] : -1, I,
                                       c == r0 ? 1 : 0});
          }
          continue;
        }
        S.pot.insert(S.pot.end(), {t11, J0, t21, t22});
        for (int64_t c = r0; c < r1; c++) {
          const int32_t I = pat.colRows[c];
          S.row.insert(S.row.end(), {two ? tile(I, J0) : pat.colTiles[c], two ? pat.colTiles[c] : -1, J0, J2, I, t11, t21, t22});
        }
      }
      sortChunksPerXcd(S.upd, firstChunk);
      S.lvU.push_back((int64_t)S.upd.size() / 4), S.lvS.push_back((int64_t)S.pot.size() / 4);
      S.lvR.push_back((int64_t)S.row.size() / 8), S.lvF.push_back((int64_t)S.fus.size() / 8);
      S.segG.push_back(g), S.segL.push_back(L), S.segDep.push_back((int32_t)dep);
    }
  S.nGroups = G;
  S.nLevels = nLev, S.nPairs = start[pat.nTiles];
  S.nSuper = 0;
  for (int32_t J = 0; J < nT; J++) S.nSuper += (role[J] != 2 && sel.col[J]) ? 1 : 0;
  S.nCopy = (int64_t)S.copy.size() / 2;
  // diagonal-tile inverses (factorSeqSn): the columns of in-place (not fused) supernodes before the top
  // separators' chain, and the rest; the same rule for the chain as factorSeqSn's
  S.invEarly.clear(), S.invLate.clear();
  const int nSeg = (int)S.segG.size();
  int chain0 = 0;
  for (int i = 1; i < nSeg; i++)
    if (S.segL[i] == S.segL[i - 1]) chain0 = i + 1;
  std::vector<uint8_t> early(nT, 0);
  for (int i = 0; i < chain0; i++)
    for (int64_t k = S.lvS[i]; k < S.lvS[i + 1]; k++) {
      early[S.pot[4 * k + 1]] = 1;
      if (S.pot[4 * k + 2] >= 0) early[S.pot[4 * k + 1] + 1] = 1;
    }
  for (int32_t J = 0; J < nT; J++)
    if (sel.col[J]) (early[J] ? S.invEarly : S.invLate).push_back(J);
  S.nInvEarly = (int64_t)S.invEarly.size(), S.nInvLate = (int64_t)S.invLate.size();
  S.built = true;
  return {};
}

// ---------------------------------------------------------------- 13. partition tile sets: the tile runs this
// rank writes (its and the ROOT columns; cleared per linearize instead of the store), the ROOT tiles
// and rows, the row blocks this rank solves (vb_share_x)
void partitionSets(const Layout& lay, const Pattern& pat, int rank, int world, PartitionSets& part) {
  part.zeroRuns.clear(), part.rootTiles.clear(), part.rootRows.clear(), part.ownRows.clear();
  for (int32_t J = 0; J < lay.nT; J++) {
    const bool own = lay.colOwner[J] == rank, root = lay.colOwner[J] == world;
    if (own || root) {
      const int64_t a = pat.colStart[J], b = pat.colStart[J + 1];
      if (!part.zeroRuns.empty() && part.zeroRuns.back().second == a) part.zeroRuns.back().second = b;
      else part.zeroRuns.push_back({a, b});
    }
    if (root) {
      part.rootRows.push_back(J);
      for (int64_t c = pat.colStart[J]; c < pat.colStart[J + 1]; c++) part.rootTiles.push_back(pat.colTiles[c]);
    }
    if (own || (rank == 0 && root)) part.ownRows.push_back(J);
  }
}

// ---------------------------------------------------------------- 14. small factors: constants + whitening
// square roots, staging slots
Status smallConstants(const Input& in, SmallConsts& small) {
  small.nSmallStage = 0;
  for (int fk = 1; fk < 14; fk++) {
    const int64_t n = (int64_t)in.fint[fk].size();
    const int extra = (fk >= 1 && fk <= 3) ? 81 : fk == 9 ? 36 : 0;
    const int nc = kNumConsts[fk] + extra;
    small.nc[fk] = nc;
    std::vector<double>& cs = small.consts[fk];
    cs.assign((size_t)n * nc, 0.0);
    for (int64_t f = 0; f < n; f++) {
      const double* src = &in.fconst[fk][f * kNumConsts[fk]];
      double* dst = &cs[f * nc];
      std::copy(src, src + kNumConsts[fk], dst);
      if (fk >= 1 && fk <= 3) {
        if (!precisionChol(src + 11 + 207, 9, dst + 331)) return {VB_E_NUMERIC, "preintegration covariance not SPD"};
      } else if (fk == 9) {
        psdSqrt(src + 7, 6, dst + 43);
      }
    }
    small.stage[fk] = small.nSmallStage;
    small.nSmallStage += n;
  }
  return {};
}

// ---------------------------------------------------------------- 15. --recompute-preint inputs (preint.hip):
// the IMU streams concatenated, per IMU sample variances
Status preintInputs(const Input& in, PreintInputs& preint) {
  preint.present = !in.piSrc.empty();
  if (!preint.present) return {};
  const int nStreams = (int)std::max<size_t>(1, in.piT.size());
  preint.off.assign(nStreams + 1, 0);
  preint.t.clear(), preint.v.clear();
  for (int s = 0; s < nStreams; s++) {
    const std::vector<int64_t>& t = s == 0 ? in.imuT : in.piT[s];
    const std::vector<double>& v = s == 0 ? in.imuV : in.piV[s];
    preint.t.insert(preint.t.end(), t.begin(), t.end());
    preint.v.insert(preint.v.end(), v.begin(), v.end());
    preint.off[s + 1] = (int64_t)preint.t.size();
  }
  for (const PreintSrc& p : in.piSrc)
    if (p.imu < 0 || p.imu >= nStreams || preint.off[p.imu + 1] == preint.off[p.imu])
      return {VB_E_ARG, "preintegration source names an IMU without a measurement stream"};
  preint.noise.assign((size_t)nStreams * 6, 0.0);
  for (int s = 0; s < nStreams; s++)
    for (int k = 0; k < 6; k++)
      preint.noise[s * 6 + k] = 6 * s + k < (int)in.piNoise.size() ? in.piNoise[6 * s + k] : kDefaultImuNoise[k];
  return {};
}

// ---------------------------------------------------------------- 16. visual_cost_kernel's order: the
// observations of each range the kernels run over ([obB, obE), [fB, fE) and the gaps between them), stably
// partitioned into global-shutter then rolling-shutter, so a wave takes one of the two evaluation paths
// instead of both; the kernels' inputs gathered in that order
void costOrder(const Layout& lay, const Observations& obs, const Shard& shard, CostOrder& cost) {
  const int64_t nObs = obs.nObs;
  cost.order.assign(nObs, 0);
  std::vector<int64_t> cuts = {0, shard.obB, shard.obE, shard.fB, shard.fE, nObs};
  std::sort(cuts.begin(), cuts.end());
  for (size_t c = 0; c + 1 < cuts.size(); c++) {
    int64_t w = cuts[c];
    for (int pass = 0; pass < 2; pass++)
      for (int64_t i = cuts[c]; i < cuts[c + 1]; i++)
        if ((obs.obRS[i] >= 0) == (pass == 1)) cost.order[w++] = (int32_t)i;
  }
  auto rsStart = [&](int64_t b, int64_t e) {
    int64_t n = 0;
    for (int64_t i = b; i < e; i++) n += obs.obRS[i] < 0;
    return b + n;
  };
  cost.rsBegin[0] = rsStart(shard.obB, shard.obE), cost.rsBegin[1] = rsStart(shard.fB, shard.fE);
  cost.pack.assign((size_t)nObs * 8, 0);
  cost.cp.assign((size_t)nObs * 6, 0.0);
  for (int64_t i = 0; i < nObs; i++) {
    const int32_t o = cost.order[i];
    int32_t* q = &cost.pack[(size_t)i * 8];
    q[0] = o, q[1] = obs.obPt[o], q[2] = obs.obPose[o], q[3] = obs.obExtr[o], q[4] = obs.obIntr[o], q[5] = obs.obRS[o];
    q[6] = obs.obVel[o];
    q[7] = (obs.obRed[(size_t)o * 4 + kSlotIntr] >= 0 ? 1 : 0) | (obs.obRed[(size_t)o * 4 + kSlotVel] >= 0 ? 2 : 0);
    for (int k = 0; k < 6; k++) cost.cp[(size_t)i * 6 + k] = obs.obC[(size_t)o * 6 + k];
  }
}

// ---------------------------------------------------------------- 17. base-map factors by landmark
Status baseMapOrder(const Input& in, const Registration& reg, BaseMapOrder& bm) {
  bm = BaseMapOrder();
  if (!in.bmPoint || in.bmPoint->empty()) return {};
  const std::vector<int32_t>& pt = *in.bmPoint;
  const int64_t n = (int64_t)pt.size(), nPts = reg.nPts;
  if (n >= INT32_MAX) return {VB_E_ARG, "too many base-map factors (2^31)"};
  bm.n = n;
  bm.start.assign(nPts + 1, 0);
  for (int64_t r = 0; r < n; r++) {
    const int32_t l = reg.lmOfPoint[pt[r]];
    if (l >= 0) bm.start[l + 1]++, bm.nFree++;
  }
  for (int64_t l = 0; l < nPts; l++) {
    if (bm.start[l + 1]) bm.lmWith.push_back((int32_t)l);
    bm.start[l + 1] += bm.start[l];
  }
  bm.rowOfPos.assign(n, 0), bm.posOfRow.assign(n, 0);
  std::vector<int64_t> fill(bm.start.begin(), bm.start.end() - 1);
  int64_t tail = bm.nFree;
  for (int64_t r = 0; r < n; r++) {
    const int32_t l = reg.lmOfPoint[pt[r]];
    const int64_t p = l >= 0 ? fill[l]++ : tail++;
    bm.rowOfPos[p] = (int32_t)r, bm.posOfRow[r] = (int32_t)p;
  }
  return {};
}

// ---------------------------------------------------------------- all stages
Status analyze(const Input& in, Symbolic& S) {
  if (Status e = registerVariables(in, S.reg)) return e;
  timeOrder(in, S.reg, S.time);
  dissect(in, S.reg, S.time, S.nd);
  if (Status e = reducedLayout(S.reg, S.nd, S.lay)) return e;
  S.lmRank.assign(S.reg.nPts, 0);
  if (in.partSet) landmarkOwners(in, S.lay, S.reg, S.lmRank);
  if (Status e = sortObservations(in, S.reg, S.lay, S.obs)) return e;
  if (Status e = landmarkPanels(S.reg, S.lay, S.obs, S.pan)) return e;
  if (Status e = shardRanges(in, S.lay, S.lmRank, S.obs, S.pan, S.shard)) return e;
  tilePattern(in, S.lay, S.obs, S.pan, S.pat);
  if (Status e = schurWork(in, S.lay, S.obs, S.pan, S.shard, S.pat, S.schur)) return e;
  if (in.knobs.stats) printFactorStats(S.pat, S.lay.nT);
  // schedules: [0] the whole factorization, or this rank's subtree plus its partial fan-in into the
  // ROOT targets; [1] the ROOT separators (partitioned, rank 0).  Only the single-handle supernode
  // schedule is cut into streams.
  const int32_t nT = S.lay.nT;
  const bool rootToo = in.partSet && in.partRank == 0;
  const Select sel0 = in.partSet ? selectRank(S.lay.colOwner, in.partRank, in.partWorld) : selectAll(nT);
  const Select sel1 = selectRoot(S.lay.colOwner, in.partWorld);
  if (Status e = columnSchedule(S.pat, nT, sel0, in.knobs.ptFuseMax, S.sch[0])) return e;
  if (rootToo)
    if (Status e = columnSchedule(S.pat, nT, sel1, in.knobs.ptFuseMax, S.sch[1])) return e;
  if (in.partSet) partitionSets(S.lay, S.pat, in.partRank, in.partWorld, S.part);
  if (in.knobs.useSn) {
    const int streams = in.partSet ? 1 : in.knobs.snStreams;
    if (Status e = supernodeSchedule(S.pat, S.lay.colOwner, nT, sel0, streams, in.knobs.stats, S.sn[0])) return e;
    if (rootToo)
      if (Status e = supernodeSchedule(S.pat, S.lay.colOwner, nT, sel1, 1, in.knobs.stats, S.sn[1])) return e;
  }
  if (Status e = smallConstants(in, S.small)) return e;
  if (Status e = preintInputs(in, S.preint)) return e;
  costOrder(S.lay, S.obs, S.shard, S.cost);
  if (in.bmPoint && !in.bmPoint->empty() && (in.partSet || in.sharded))
    return {VB_E_UNSUPPORTED, "base-map factors need the whole problem on one handle (no shard / partition)"};
  if (Status e = baseMapOrder(in, S.reg, S.bm)) return e;
  return {};
}

}  // namespace viba_host
