// vb_finalize's symbolic analysis (symbolic.hip): host-only.  From the variables and factors a handle
// holds before vb_finalize it derives everything the kernels later take on trust -- the reduced order
// and its nested dissection, the tile pattern and fill, the landmark / observation layouts, the Schur
// work lists, both factorization schedules and the solve task lists -- as plain vectors and scalars.
// No HIP API call, no vb_handle_s, no getenv: finalize.hip fills the Input, calls analyze() and uploads
// the Symbolic; tests/cpp/symbolic_check.cpp runs the same code without a device.
#pragma once
#include <algorithm>
#include <array>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "../../include/viba_hip.h"
#include "engine.hpp"

namespace viba_host {
using namespace viba;  // engine.hpp: TileEnt, TileWork, PreintSrc, ImuIdx

constexpr int TS = 64;
constexpr int kVarData[9] = {3, 7, 3, 3, 24, 7, 32, 7, 4};
constexpr int kNumVars[14] = {5, 6, 9, 10, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1};
constexpr int kNumConsts[14] = {6, 331, 331, 331, 4, 23, 17, 6, 6, 43, 55, 41, 13, 13};
// ImuNoiseModelParameters::reset sample variances (imu_types/ImuNoiseModelParameters.h:78-80): accel 3, gyro 3
constexpr double kDefaultImuNoise[6] = {6.6297049e-3, 6.6297049e-3, 6.6297049e-3, 2.7415568e-05, 2.7415568e-05, 2.7415568e-05};
const int kFK[14][10] = {{0, 1, 5, 4, 2}, {6, 1, 2, 1, 2, 8}, {6, 1, 2, 3, 1, 2, 3, 7, 8},
                         {6, 1, 2, 3, 7, 1, 2, 3, 7, 8}, {3, 7}, {6, 6}, {4, 4}, {7, 7}, {5, 5}, {1}, {6}, {4},
                         {5}, {7}};

inline ImuIdx makeJac(int mask) {
  ImuIdx J;
  int i = 0;
  J.gB = (mask & 1) ? (i += 3) - 3 : -1;
  J.aB = (mask & 2) ? (i += 3) - 3 : -1;
  J.gS = (mask & 4) ? (i += 3) - 3 : -1;
  J.aS = (mask & 8) ? (i += 3) - 3 : -1;
  J.gN = (mask & 16) ? (i += 6) - 6 : -1;
  J.aN = (mask & 32) ? (i += 3) - 3 : -1;
  J.rT = (mask & 64) ? (i += 1) - 1 : -1;
  J.gaT = (mask & 128) ? (i += 1) - 1 : -1;
  J.size = i;
  return J;
}

// symmetric square root U (P = U^T U) of a PSD m x m matrix via cyclic Jacobi eigen-decomposition
void psdSqrt(const double* Pm, int m, double* U);
// upper Cholesky U of P = inverse(cov) (cov SPD, col-major m x m): P = U^T U
bool precisionChol(const double* cov, int m, double* U);

// ---------------------------------------------------------------- input
struct Knobs {
  double cutWin = 0.05;      // VIBA_ND_CUTWIN: half width of the cut window around a part's median, 0 .. 0.45
  int64_t leafDims = 1024;   // VIBA_ND_LEAF: parts of at most this many dims are not dissected (>= 64)
  bool kindOrder = true;     // VIBA_ND_KINDS: order every dissection part by variable class (0: plain time order)
  int64_t ptFuseMax = 256;   // column-schedule levels with at most this many off-diagonal tiles are fused
  bool useSn = true;         // VIBA_SUPERNODE: also build the two-column supernode schedules
  int snStreams = 2;         // VIBA_SN_STREAMS: streams of the single-handle supernode schedule, 1 .. 4
  bool stats = false;        // VIBA_STATS: print the [schur stats] / [factor stats] lines to stderr
};

struct Input {
  const std::vector<double> (&data)[9];
  const std::vector<uint8_t> (&cst)[9];
  const std::vector<int32_t> (&fvars)[14];
  const std::vector<int32_t> (&fint)[14];
  const std::vector<double> (&fconst)[14];
  int imuCalibOptions;  // vb_config::imu_calib_options: the IMU calibration's tangent size
  int32_t nRS;          // rolling-shutter tables a visual factor may name
  // landmark shard request (vb_set_landmark_shard): lmEnd < 0 is "all"
  bool sharded;
  int64_t lmBegin, lmEnd;
  bool isRoot;
  // partition request (vb_set_partition)
  bool partSet;
  int partRank, partWorld;
  // --recompute-preint: stream 0 is (imuT, imuV), streams 1.. (piT[s], piV[s])
  const std::vector<PreintSrc>& piSrc;
  const std::vector<int64_t>& imuT;
  const std::vector<double>& imuV;
  const std::vector<std::vector<int64_t>>& piT;
  const std::vector<std::vector<double>>& piV;
  const std::vector<double>& piNoise;
  Knobs knobs;
  // base-map visual factors (vb_add_basemap_factors): the point handle of every row; nullptr: none
  const std::vector<int32_t>* bmPoint = nullptr;
};

// error of a stage: code 0 is success; the caller hands (code, msg) to fail()
struct Status {
  int code = 0;
  const char* msg = "";
  explicit operator bool() const { return code != 0; }
};

// ---------------------------------------------------------------- what the stages produce
// 1. registration: the free non-point variables in first-use order, the free observed points numbered
struct Registration {
  int64_t nvar[9] = {};
  std::vector<std::pair<int, int>> reg;  // registered (kind, handle), in registration order
  std::vector<int32_t> regOf[9];         // variable handle -> registration index, -1
  std::vector<int> tdims;                // tangent size per registration index
  // point handle -> landmark, -1; by first observing rig, ties by handle (stage 5 renumbers it by rank)
  std::vector<int32_t> lmOfPoint;
  int64_t nPts = 0;
  int jacSize = 0;
};
// 2. time order of the registered variables and the span of time positions each is coupled to
struct TimeOrder {
  std::vector<int> order;     // time position -> registration index
  std::vector<int> pos;       // registration index -> time position
  std::vector<int> hiP, loP;  // per registration index: highest / lowest coupled time position
};
// 3. nested dissection: the final order cut into tile-aligned parts and who owns each
struct Dissection {
  std::vector<int> order;          // reduced id -> registration index
  std::vector<size_t> partBegin;   // first reduced id of every part
  std::vector<int> partOwner;      // rank of the part's subtree, partWorld: ROOT (0 when not partitioned)
};
// 4. reduced layout
struct Layout {
  int32_t nRV = 0, nT = 0;
  int64_t nRed = 0, nRedReal = 0;
  std::vector<int32_t> rvKind, rvHandle, rvDim;
  std::vector<int64_t> rvOff;      // nRV + 1
  std::vector<int32_t> redOf[9];   // variable handle -> reduced id, -1
  std::vector<int64_t> padRows;    // rows no block covers
  std::vector<int8_t> colOwner;    // per tile column
};
// 6. observations sorted by landmark (constant-point observations last), their index arrays
struct Observations {
  int64_t nObs = 0, nObsPad = 0;
  std::vector<int64_t> perm;  // sorted position -> visual factor row
  std::vector<int32_t> obPose, obExtr, obIntr, obVel, obRS, obPt;
  std::vector<int32_t> obRed;  // 4 per observation
  std::vector<double> obC;     // 6 per observation
  std::vector<int64_t> lmObs;  // nPts + 1
};
// 7. landmark panels and blocks, incidence lists
struct Panels {
  std::vector<int64_t> lmBlk, lmY;
  std::vector<int32_t> blkRed, blkCol, obCol, pcRow, pcBlk, bxEnt;
  std::vector<int64_t> bxStart;
  std::vector<int64_t> oxStart, lxStart, lxChunk;
  std::vector<int32_t> oxObs, oxSlot, lxLm, lxCol;
  int64_t nYcol = 0;
};
// 8. this handle's shard: landmarks [lmBegin, lmEnd), their observations [obB, obE), constant-point
// observations [fB, fE)
struct Shard {
  int64_t lmBegin = 0, lmEnd = 0;
  bool isRoot = true;
  int64_t obB = 0, obE = 0, obFree = 0, fB = 0, fE = 0;
  std::vector<int32_t> lmList;  // narrow panels (<= kLmSmallCols columns) first, then the wide ones
  int64_t nLmSmall = 0, nLmBig = 0;
  int32_t lmBigCols = 0;
  // landmarks without a visual observation (free points that only base-map factors name): an empty
  // observation range and panel, kept out of lmList so no record-staging kernel meets one
  std::vector<int32_t> loneList;
};
// 9. tile pattern with fill, by column and by row
struct Pattern {
  int64_t nTiles = 0;
  std::vector<int64_t> rowEnd;       // per reduced variable: end of its last coupled block
  std::vector<int32_t> tileIdx;      // nT * nT, -1
  std::vector<uint8_t> tileFill;     // per tile: 1 = no coupling produced it
  std::vector<uint8_t> tileDirect;   // per tile: a direct term (not only landmark products) writes it
  std::vector<int64_t> colStart, rowStart;
  std::vector<int32_t> colTiles, colRows, rowTiles, rowCol;
  // elimination levels of the tile columns (the column schedule's)
  int32_t nLevels = 0;
  std::vector<int32_t> level;
  std::vector<std::vector<int32_t>> levelCols;
};
// 10. Schur work
struct SchurWork {
  std::vector<TileEnt> ents;
  std::vector<TileWork> works;
  std::vector<uint64_t> runs;
  std::vector<uint32_t> tasks;
  std::vector<int64_t> grpStart;
  std::vector<int32_t> grpObs, grpRed;
  bool hasClear = false;             // single handle: clearTiles is the linearization's clear list
  std::vector<int32_t> clearTiles;
  int64_t tileFirst = 0, tileCount = 0;
  std::vector<int32_t> shardTiles;   // non-root: exact tiles of the partial system
};
// 11. / 12. columns a schedule factors, takes fan-in targets in, takes contributions from, and rows whose
// x is known before the backward solve
struct Select {
  std::vector<uint8_t> col, tgt, src, pre;
};
// the host side of Sched (host.hpp): Sched adds the device pointers and graphs
struct SchedShape {
  std::vector<int64_t> lvP, lvT, lvU;
  // levels factored by one potrf + trsm launch (potrf_trsm_kernel): per level the range of its items
  // (diagonal tile, column, target, row, writer) in ptf; the diagonal tiles to copy back from Lscr
  std::vector<int64_t> lvPF;
  int64_t nPtfDiag = 0;
  int32_t nLevels = 0;
  int64_t nPairs = 0;
  int64_t nF = 0, nB = 0, nPreReady = 0;  // preReady: rows whose x is known before the backward solve
  bool built = false;
};
struct SchedHost : SchedShape {
  std::vector<int32_t> potrfTile, potrfCol, trsmDiag, trsmTarget, trsmCol, trsmRow, upd, fanPairs;
  std::vector<int32_t> tasksF, tasksB, expF, expB, preReady, ptf, ptfDiag;
};
// the host side of SnSched (host.hpp)
struct SnSchedShape {
  int32_t nLevels = 0;
  int64_t nPairs = 0;                  // fan-in contributions (external to the supernodes)
  int64_t nSuper = 0, nTwo = 0;        // supernodes, of which two-column
  std::vector<int64_t> lvU, lvS, lvR;  // per segment: fan-in chunk, supernode and row-item ranges
  // segments: one level of one stream (nGroups > 1: independent subtrees and the separators above them),
  // level-major; segL its level, segDep the bit mask of other streams it waits for
  std::vector<int32_t> segG, segL, segDep;
  int nGroups = 1;
  std::vector<int64_t> lvF;            // per segment: fused items
  int64_t nCopy = 0;
  int64_t nInvEarly = 0, nInvLate = 0;
  bool built = false;
};
struct SnSchedHost : SnSchedShape {
  std::vector<int32_t> upd, fanPairs, pot, row, fus, copy, invEarly, invLate;
  // for the checks: first column's role (0 single, 1 first of a pair, 2 second), level and stream
  std::vector<int8_t> pairRole;
  std::vector<int32_t> level, stream;
};
// 13. partition tile sets
struct PartitionSets {
  std::vector<std::pair<int64_t, int64_t>> zeroRuns;
  std::vector<int32_t> rootTiles, rootRows, ownRows;
};
// 14. small-factor constants with the whitening roots appended
struct SmallConsts {
  int nc[14] = {};
  int64_t stage[14] = {};
  std::vector<double> consts[14];
  int64_t nSmallStage = 0;
};
// 15. --recompute-preint inputs
struct PreintInputs {
  bool present = false;
  std::vector<int64_t> off, t;
  std::vector<double> v, noise;
};
// 16. cost order and the packed observation arrays
struct CostOrder {
  std::vector<int32_t> order, pack;
  std::vector<double> cp;
  int64_t rsBegin[2] = {0, 0};
};

// 17. base-map factors sorted by landmark, constant-point factors after them (rows keep their order
// inside a landmark)
struct BaseMapOrder {
  int64_t n = 0, nFree = 0;
  std::vector<int64_t> start;      // nPts + 1: landmark l's factors are positions [start[l], start[l + 1])
  std::vector<int32_t> rowOfPos;   // position -> vb_add_basemap_factors row
  std::vector<int32_t> posOfRow;   // and back (the report's order)
  std::vector<int32_t> lmWith;     // landmarks that have factors, ascending
};

struct Symbolic {
  Registration reg;
  TimeOrder time;
  Dissection nd;
  Layout lay;
  std::vector<int> lmRank;  // 5. partitioned: owning rank per landmark (ascending)
  Observations obs;
  Panels pan;
  Shard shard;
  Pattern pat;
  SchurWork schur;
  SchedHost sch[2];      // [0] everything, or this rank's subtree + its ROOT targets; [1] ROOT (rank 0)
  SnSchedHost sn[2];
  PartitionSets part;
  SmallConsts small;
  PreintInputs preint;
  CostOrder cost;
  BaseMapOrder bm;
};

// ---------------------------------------------------------------- the stages
Status registerVariables(const Input& in, Registration& reg);
void timeOrder(const Input& in, const Registration& reg, TimeOrder& time);
void dissect(const Input& in, const Registration& reg, const TimeOrder& time, Dissection& nd);
Status reducedLayout(const Registration& reg, const Dissection& nd, Layout& lay);
void landmarkOwners(const Input& in, const Layout& lay, Registration& reg, std::vector<int>& lmRank);
Status sortObservations(const Input& in, const Registration& reg, const Layout& lay, Observations& obs);
Status landmarkPanels(const Registration& reg, const Layout& lay, const Observations& obs, Panels& pan);
Status shardRanges(const Input& in, const Layout& lay, const std::vector<int>& lmRank, const Observations& obs,
                   const Panels& pan, Shard& shard);
void tilePattern(const Input& in, const Layout& lay, const Observations& obs, const Panels& pan, Pattern& pat);
Status schurWork(const Input& in, const Layout& lay, const Observations& obs, const Panels& pan, const Shard& shard,
                 const Pattern& pat, SchurWork& schur);
Select selectAll(int32_t nT);
Select selectRank(const std::vector<int8_t>& colOwner, int rank, int world);
Select selectRoot(const std::vector<int8_t>& colOwner, int world);
Status columnSchedule(const Pattern& pat, int32_t nT, const Select& sel, int64_t ptFuseMax, SchedHost& S);
Status supernodeSchedule(const Pattern& pat, const std::vector<int8_t>& colOwner, int32_t nT, const Select& sel,
                         int nStreams, bool stats, SnSchedHost& S);
void partitionSets(const Layout& lay, const Pattern& pat, int rank, int world, PartitionSets& part);
Status smallConstants(const Input& in, SmallConsts& small);
Status preintInputs(const Input& in, PreintInputs& preint);
void costOrder(const Layout& lay, const Observations& obs, const Shard& shard, CostOrder& cost);
Status baseMapOrder(const Input& in, const Registration& reg, BaseMapOrder& bm);

// all of them in order
Status analyze(const Input& in, Symbolic& S);

}  // namespace viba_host
