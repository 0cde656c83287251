// Host side of the HIP LM engine, shared by its translation units: the kernel launchers (visual.hip / small.hip /
// chol.hip / ...), host helpers, the schedules and the handle.  vb_handle_s is a few groups, one per lifetime:
// a group's owner (devmem.hpp), the device pointers into its memory and its host-side data are one object, and
// dropping the object is the only way to undo the group.  Finalized and the lazy groups are built beside the
// handle and installed once whole, so a failure leaves the handle as it was.  api.hip: the C-ABI and the queued
// phases; factor_host.hip, pcg_host.hip: the drivers; symbolic.hip + finalize.hip: vb_finalize; multi.hip.
#pragma once
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <climits>
#include <numeric>
#include <string>
#include <unordered_map>
#include <map>
#include <memory>
#include <vector>

#include "../../include/viba_hip.h"
#include "devmem.hpp"
#include "engine.hpp"
#include "symbolic.hpp"

namespace viba {
// kernel launchers, each group under the file that defines it
// visual factors (visual.hip)
void launch_visual_lin(const Dev& d, int updateCache, int dontRetry, int64_t lo, int64_t hi, hipStream_t st);
void launch_visual_cost(const Dev& d, int comparable, int64_t lo, int64_t hi, hipStream_t st);
// base-map visual factors (basemap.hip): linearization + the per-landmark sums, cost pass; nothing without factors
void launch_basemap_lin(const Dev& d, int updateCache, int dontRetry, hipStream_t st);
void launch_basemap_cost(const Dev& d, int comparable, hipStream_t st);
// LM bookkeeping (lm_kernels.hip)
void launch_fold_red(const Dev& d, hipStream_t st);
void launch_copy_vars(const Dev& d, bool backup, const int64_t* len, hipStream_t st);
void launch_spec_commit(const Dev& d, hipStream_t st);
// small factors (small.hip)
void launch_small(const Dev& d, int mode, double* gOut, hipStream_t st);
void launch_small_eval(const Dev& d, int mode, double* gOut, hipStream_t st);
void launch_small_assemble(const Dev& d, int mode, double* gOut, hipStream_t st, int part = 3);
// rolling shutter (rs.hip), triangulation (triangulate.hip), preintegration (preint.hip), point refinement (refine.hip)
void launch_rs_build(const Dev& d, hipStream_t st);
void launch_rs_row_poses(const Dev& d, int64_t n, const int32_t* obsRig, const int32_t* obsCam, const double* obsRow,
                         const double* rigPose, const double* rigVel, const int32_t* rigRS, const double* cams,
                         double* out, hipStream_t st);
void launch_triangulate(int64_t nTracks, int64_t nObs, const int64_t* start, const int32_t* seed, const double* Tcw,
                        const int32_t* obsCam, const double* cams, const double* uv, const double* sqrtH, double* rays,
                        double* point, uint8_t* ok, uint8_t* inlier, hipStream_t st);
void launch_preint(const Dev& d, const PreintArgs& pa, hipStream_t st);
void launch_refine_points(const Dev& d, const int64_t* gStart, const int32_t* gObs, const int32_t* gPt, int64_t nG,
                          double* backups, double* acc, hipStream_t st);
// landmark elimination (landmark.hip)
void launch_landmark(const Dev& d, double lambda, int mode, hipStream_t st);
// observation-group Gram blocks (obs_group.hip)
void launch_groups(const Dev& d, double lambda, hipStream_t st, int mode = 0);
// reduced diagonal damping, Schur products, new reduced RHS (schur.hip)
void launch_schur(const Dev& d, double lambda, int addIdentity, hipStream_t st);
void launch_damp(const Dev& d, double lambda, int addIdentity, hipStream_t st);
void launch_schur_products(const Dev& d, double lambda, hipStream_t st);
void launch_reduced_grad(const Dev& d, int mode, hipStream_t st);
// tile Cholesky: diagonal blocks and rows of both schedules, diagonal inverses, padding (chol.hip)
void launch_potrf(const Dev& d, const int32_t* tiles, const int32_t* cols, int n, double* dinv, hipStream_t st,
                  const double* fwdB = nullptr, double* fwdY = nullptr);
void launch_trsm(const Dev& d, const int32_t* diag, const int32_t* target, const int32_t* cols, int n, const double* dinv,
                 hipStream_t st, const int32_t* rows = nullptr, const double* fwdY = nullptr, double* fwdB = nullptr);
void launch_potrf_trsm(const Dev& d, const int32_t* items, int n, double* Lscr, double* dinv, hipStream_t st,
                       double* fwdB, double* fwdY);
void launch_copy_diag(const Dev& d, const int32_t* pairs, int n, const double* Lscr, hipStream_t st);
void launch_snpotrf(const Dev& d, const int32_t* items, int n, double* dinv, hipStream_t st, const double* fwdB,
                    double* fwdY);
void launch_snpotrf_trsm(const Dev& d, const int32_t* items, int n, double* Lscr, double* dinv, hipStream_t st,
                         double* fwdB, double* fwdY);
void launch_sntrsm(const Dev& d, const int32_t* items, int n, const double* dinv, hipStream_t st, const double* fwdY,
                   double* fwdB);
void launch_diag_inverse(const Dev& d, const int32_t* cols, int64_t n, double* linv, hipStream_t st);
void launch_pad_diag(const Dev& d, const int64_t* rows, int64_t n, hipStream_t st);
// tile Cholesky: fan-in (fanin.hip)
void launch_fanin(const Dev& d, const int32_t* work, const int32_t* pairs, int n, hipStream_t st);
// persistent triangular solves (trisolve.hip)
void launch_solve_fanout(const Dev& d, const int32_t* tasksF, int64_t nF, const int32_t* tasksB, int64_t nB,
                         const int32_t* expF, const int32_t* expB, const int32_t* colTiles, const int32_t* colRows,
                         const int32_t* rowTiles, const int32_t* rowCol, const double* linv, double* b, double* y,
                         double* x, unsigned* flags, int G, hipStream_t st, int phases, const int32_t* pre,
                         int64_t nPre);
// back-substitution, vector utilities, applyStep (step.hip)
void launch_backsub(const Dev& d, int mode, int64_t lo, int64_t hi, const double* xr, double* xp, hipStream_t st);
void launch_dot(const double* a, const double* b, int64_t n, double* out, hipStream_t st);
void launch_axpby(double* y, const double* x, double a, double b, int64_t n, hipStream_t st);
void launch_boxplus(const Dev& d, const double* stepRed, const double* stepPt, hipStream_t st);
// iterative reduced solve (pcg.hip)
void launch_tile_symv(const double* tiles, const int32_t* tileList, const int32_t* tileRC, int64_t n, const double* x,
                      double* y, const double* stop, hipStream_t st);
void launch_jacobi_init(const Dev& d, double* jac, hipStream_t st);
void launch_jacobi_apply(const Dev& d, const double* jac, const double* r, double* z, hipStream_t st);
void launch_pcg_xr(double* x, double* r, const double* p, const double* Ap, const double* red, int zr, int pAp,
                   int64_t n, double* rn2, hipStream_t st);
void launch_pcg_p(double* p, double* Ap, const double* z, const double* red, int zrNew, int zr, int64_t n,
                  hipStream_t st);
void launch_pcg_check(double* red, double r0, double tol, int k, int maxIt, int zrNew, hipStream_t st);
// shard / partition exchange (multi.hip)
void launch_tile_gather(const Dev& d, const int32_t* tiles, int64_t n, double* out, hipStream_t st);
void launch_tile_scatter_add(const Dev& d, const int32_t* tiles, int64_t n, const double* in, hipStream_t st);
void launch_chunk_copy(double* base, const int32_t* idx, int64_t n, int chunk, double* buf, int mode, hipStream_t st);
// selected inversion (selinv.hip), point covariances (pointcov.hip)
void launch_selinv_level(double* tiles, const int32_t* tileIdx, int32_t nT, const int64_t* colStart,
                         const int32_t* colRows, const int32_t* colTiles, const double* linv, double* U,
                         const int32_t* uItems, int nU, const int32_t* zItems, int nZ, const int32_t* dItems, int nD,
                         hipStream_t st);
void launch_gather(const double* src, const int64_t* idx, int64_t n, double* out, hipStream_t st);
void launch_zero_tiles(double* tiles, const int32_t* list, int64_t n, hipStream_t st);
void launch_pointcov(const Dev& d, const int32_t* items, int64_t nSmall, int64_t nBig, const int32_t* reqLm,
                     const int64_t* xStart, const int32_t* xPc, const int64_t* outOff, double* out, hipStream_t st);
// fp32 preconditioner factor (lowprec.hip)
void launch_lp_cast(const double* in, float* out, int64_t n, hipStream_t st);
void launch_lp_uncast(const float* in, double* out, int64_t n, hipStream_t st);
void launch_lp_damp(float* t32, const int32_t* tileIdx, int32_t nT, const int64_t* rvOff, const int32_t* rvDim,
                    int64_t nRV, float eps, hipStream_t st);
void launch_lp_factor_level(float* t32, const int32_t* work, int nWork, const int32_t* pairs, const int32_t* diag,
                            const int32_t* cols, int nDiag, const int32_t* targets, const int32_t* tcols, int nTrsm,
                            float* linv, hipStream_t st);
void launch_lp_nonfinite(const float* x, int64_t n, int32_t* flag, float* sum, hipStream_t st);
void launch_lp_fwd_level(const float* t32, const int32_t* cols, int nCols, const int32_t* targets, const int32_t* tcols,
                         const int32_t* trows, int nTrsm, const float* linv, float* t, hipStream_t st);
void launch_lp_bwd_level(const float* t32, const int64_t* colStart, const int32_t* colTiles, const int32_t* colRows,
                         const int32_t* cols, int nCols, const float* linv, float* t, hipStream_t st);
}  // namespace viba

using namespace viba;

namespace viba_host {

inline thread_local std::string g_err = "";
constexpr int kMaxTan[9] = {3, 6, 3, 3, 17, 6, 23, 6, 2};

inline int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}
#define HIPCHK(x)                                                                       \
  do {                                                                                  \
    hipError_t e_ = (x);                                                                \
    if (e_ != hipSuccess) return fail(VB_E_HIP, std::string(#x) + ": " + hipGetErrorString(e_)); \
  } while (0)

inline LossParams makeLoss(double a, double k) {
  LossParams L;
  L.a = a, L.b = a * a, L.k2 = k * k, L.h = 2.0 * a * k - a * a;
  return L;
}

// a failed DevOwner request as the C-ABI's error
template <class Owner>
int devFail(const Owner& m, const std::string& what) {
  return fail(VB_E_HIP, what + ": " + hipGetErrorString((hipError_t)m.lastError()));
}
// queue the read-back of dev[0, n) on st (nothing for a null host pointer)
template <typename T>
int download(T* host, const T* dev, size_t n, hipStream_t st) {
  if (host && n) HIPCHK(hipMemcpyAsync(host, dev, n * sizeof(T), hipMemcpyDeviceToHost, st));
  return 0;
}

}  // namespace viba_host
using namespace viba_host;

// One tile-Cholesky schedule (factorSeq): per elimination level the potrf / trsm / fan-in work
// lists (offsets lvP / lvT / lvU), the fan-in contribution pairs it indexes, and the fan-out solve
// task lists over the same columns (trisolve.hip fwd/bwd_fanout_kernel).
struct Sched : SchedShape {
  int32_t *ptfD = nullptr, *ptfDiagD = nullptr;
  int32_t *potrfTileD = nullptr, *potrfColD = nullptr, *trsmDiagD = nullptr, *trsmTargetD = nullptr,
          *trsmColD = nullptr, *updD = nullptr, *fanPairsD = nullptr, *trsmRowD = nullptr;
  int32_t *tasksFD = nullptr, *tasksBD = nullptr, *expFD = nullptr, *expBD = nullptr, *preReadyD = nullptr;
  hipGraphExec_t graph[2] = {nullptr, nullptr};  // per tile store (Finalized::tileSet)
};

// Two-column supernodes (VIBA_SUPERNODE, single handle): where column J + 1 is J's parent in the
// elimination tree and J's other rows are rows of J + 1, the pair is factored as one 128-wide diagonal
// block (snpotrf8_kernel: L11, L21 = A21 L11^-T, A22 -= L21 L21^T, L22) and its rows by one kernel
// (sntrsm_kernel: L_I1 = A_I1 L11^-T, A_I2 -= L_I1 L21^T, L_I2 = A_I2 L22^-T), so the pair is ONE level
// of the schedule: about half the levels (launches, dependency gaps, potrf latency chains) of the
// column schedule.  The fan-in lists leave out the pair-internal contributions (J -> J + 1).
struct SnSched : SnSchedShape {
  int32_t *updD = nullptr, *fanPairsD = nullptr;
  int32_t *potD = nullptr;  // per supernode: tile (J, J), J, tile (J + 1, J) or -1, tile (J + 1, J + 1) or -1
  int32_t *rowD = nullptr;  // per row item: tile (I, J) or -1, tile (I, J + 1) or -1, J, J + 1 or -1, I,
                            //   tile (J, J), tile (J + 1, J), tile (J + 1, J + 1)
  // levels with few rows: diagonal block + one row per block in one launch (snpotrf_trsm8_kernel); items
  // (tile (J, J), J, tile (J + 1, J) or -1, tile (J + 1, J + 1) or -1, tile (I, J) or -1, tile (I, J + 1) or
  // -1, I or -1, writer); their factored diagonal-block tiles come back from the scratch at the end
  int32_t *fusD = nullptr, *copyD = nullptr;
  // the solves' diagonal-tile inverses: of the columns factored in place before the top separators' chain
  // (invEarlyD, queued on a free stream when the chain starts) and of the rest (invLateD, after the join)
  int32_t *invEarlyD = nullptr, *invLateD = nullptr;

  hipGraphExec_t graph[2] = {nullptr, nullptr};
};

// ---------------------------------------------------------------- the handle's groups
// what the caller sets before vb_finalize (vb_finalize only reads it)
struct Problem {
  std::vector<double> data[9];
  std::vector<uint8_t> cst[9];
  std::vector<int32_t> fvars[14], fint[14];
  std::vector<double> fconst[14];
  int32_t nRS = 0;
  std::vector<int64_t> rsOff;  // of the given tables (vb_set_rs_tables); Finalized::rsOff: the device tables'
  std::vector<double> rsS, rsI, rsG;
  // device rebuild of the tables (vb_set_imu_measurements / vb_set_rs_rigs)
  std::vector<int64_t> imuT, rsMid, rsHalf;
  std::vector<double> imuV;
  std::vector<int32_t> rsCalib;
  int32_t rsGravVar = -1;
  bool rsDevice = false;
  // --recompute-preint (vb_set_imu_stream / vb_set_imu_noise / vb_set_preint_sources): IMU streams
  // 1.. (stream 0 is imuT / imuV), per IMU sample variances, per inertial row its IMU and interval
  std::vector<std::vector<int64_t>> piT;
  std::vector<std::vector<double>> piV;
  std::vector<double> piNoise;  // 6 per IMU: accel var 3, gyro var 3, as given (Finalized::piNoise: every IMU's)
  std::vector<PreintSrc> piSrc;
  bool recomputePreint = false;
  // the landmark shard and the partition as requested (Finalized::shard: the shard as resolved)
  int64_t lmBegin = 0, lmEnd = -1;
  bool sharded = false, isRoot = true, partSet = false;
  int partRank = 0, partWorld = 1;  // world 1 with partSet: one rank factors its subtree and the ROOT
  // the base map (vb_set_basemap): key rig poses (7 each), per camera its key rig, extrinsics (7) and record
  // (24); its factors (vb_add_basemap_factors): point handle, camera, 6 constants
  bool bmSet = false;
  std::vector<double> bmRig, bmCamT, bmCam, bmConst;
  std::vector<int32_t> bmCamRig, bmPoint, bmCamera;
};

// vb_create's streams and events, destroyed last
struct Streams {
  DevOwner mem;
  // st2: the small (non-visual) factor kernels -- few waves, latency-bound -- beside the visual kernels, forked
  // after the buffer resets and joined before their first consumer.  stZ: vb_linearize's clear of the reduced
  // system, so the small factors' evaluation (st2) does not queue behind the 2.2 GB memset (evZero).  The
  // supernode schedule's streams (VIBA_SN_STREAMS, 1..4) are st, st2, stZ, stF, forked and launched eagerly:
  // captured into a graph the forked schedule ran 12% slower per iteration (r05k)
  hipStream_t st = nullptr, st2 = nullptr, stZ = nullptr, stF = nullptr;
  hipEvent_t ev[12];
  hipEvent_t evFork = nullptr, evJoin = nullptr;
  hipEvent_t evZero = nullptr, evSmallE = nullptr, evZJoin = nullptr;
  hipEvent_t evSnFork = nullptr, evSnLvl[4] = {}, evClr = nullptr, evClrDone = nullptr, evInvAt[4] = {}, evInvDone = nullptr;
  hipEvent_t evStep = nullptr, evRs = nullptr;  // vb_optimize: box-plus done; the speculative rebuild on stF done
};

// what vb_create reads from the environment or the device, and what vb_set_solver sets
struct Tuning {
  bool useGraphs = true;  // the tile factorization's launches as one HIP graph per schedule and tile store
  bool specEarly = true;  // specEarly beside the cost pass (VIBA_SPEC_EARLY=0: inside the speculative linearization)
  bool costFuse = true;  // the global-shutter cost pass inside the speculative linearization (VIBA_COST_FUSE=0)
  // vb_optimize: the clear of the spare tile store for the next iteration's speculative linearization
  // queued on stZ from inside the factorization, at the top separators' chain (one stream, a few
  // latency-bound launches per level, HBM idle) instead of beside the cost pass (VIBA_CLEAR_IN_FACTOR=0)
  bool clearInFactor = true;
  bool specFailDebug = false;  // VIBA_DEBUG_SPEC_FAIL=1: specPrepare fails after its first allocations (test)
  bool useSn = true;           // VIBA_SUPERNODE=0 at creation: the column schedule
  int snStreams = 2, numCUs = 256;
  int64_t ptFuseMax = 256;  // levels with at most this many off-diagonal tiles run potrf + trsm in one launch
  // vb_set_solver: direct, or S x = rhsWork by PCG over the unfactored tiles (pcg_host.hip)
  int solverType = VB_SOLVER_DIRECT, pcgMaxIt = 40;  // Optimizer.h:43-45 defaults
  double pcgTol = 1e-10;
};

// what changes from call to call
struct RunState {
  bool linearized = false, factored = false;
  vb_phase_times times{};
  // vb_set_deferred: the phase functions of the multi-process controllers queue their work and return
  // without a host wait or scalar read; their scalars stay in red[0, 17) / err for one vb_read_scalars
  bool deferred = false;
  bool scalarsMarked = false;  // vb_mark_scalars recorded evCost since the last read
  int specSet = 0;             // vb_spec_linearize's event set
  int specCommitted = -1;      // the event set of the speculative linearization last committed
  bool specPending = false;    // a vb_spec_linearize awaits vb_spec_commit
  int32_t lastWords[2] = {0, 0};  // error words of the last check (vb_error_words)
  bool rsTimed = false;
  // clearWanted: factorSeqSn queues the spare store's clear (Tuning::clearInFactor; then sets clearQueued)
  bool clearWanted = false, clearQueued = false, clearOnF = false;
  bool factorOnly = false;  // no solve follows (vb_compute_covariances): no fused forward solve, eager
  double pointCovMs[3] = {0.0, 0.0, 0.0};  // host ms of the last point covariances: prologue, inversion, rest
  double calibEvalMs = 0.0;  // device time of the last vb_calib_projection_offsets' kernels (calib_eval.hip)
  int32_t pcgIters = 0;
  double pcgRelRes = 0.0;
  int faultNegModelRedIt = -1, faultFailIt = -1;  // vb_debug_negate_model_reduction / _fail_iteration (tests)
  // a step / sub-step is on the device (vb_damp_factor_solve / vb_solve_with_new_gradient have run):
  // vb_factor_expected_delta and vb_inspect_nonlinearities need one
  bool haveStep = false, haveSub = false;
  int inspectIt = 0, inspectK = 5;  // vb_set_inspect_iteration (1-based iteration of vb_optimize, 0: off)
};

// everything vb_finalize makes (doFinalize, finalize.hip); the handle is finalized when it has one
struct Finalized {
  DevOwner mem;
  Dev d;
  PreintArgs pi;
  // tile-Cholesky schedules: sch[0] the whole factorization (or, partitioned, this rank's subtree
  // plus its partial fan-in into the ROOT targets), sch[1] the ROOT separators (partitioned, rank 0);
  // sn[]: their two-column supernode schedules (direct factorization)
  Sched sch[2];
  SnSched sn[2];
  int tileSet = 0;  // which of the two tile stores d.tiles is (selects the factorization graph)
  int64_t* padRowsD = nullptr;  // reduced rows that belong to no variable (tile alignment of parts)
  // tiles the linearization clears (single handle): every tile but those one Schur item stores whole
  int32_t *clearTilesD = nullptr, *shardTilesD = nullptr;
  double* shardPack = nullptr;  // packed copy of shardTiles (vb_pack_shard_tiles)
  double *dinv = nullptr, *yvec = nullptr, *rhsWork = nullptr, *linv = nullptr;
  double* lscr = nullptr;    // L_JJ of the fused levels' columns (nT tiles), copied back after the factorization
  double* lscrSn = nullptr;  // the supernode schedule's: L11 / L22 at [J] / [J + 1], L21 at [nT + J]
  int32_t *colTilesD = nullptr, *colRowsD = nullptr, *rowTilesD = nullptr, *rowColD = nullptr;
  int64_t *colStartD = nullptr, *rowStartD = nullptr;
  unsigned* solveFlags = nullptr;
  // partitioned: tiles of ROOT columns, ROOT tile rows, the row blocks this rank solves (vb_share_x)
  int32_t *rootTilesD = nullptr, *rootRowsD = nullptr, *ownRowsD = nullptr;
  double *rootPack = nullptr, *rowPack = nullptr, *ownPack = nullptr;
  // host-side results of the analysis (symbolic.hpp), moved out of it
  Layout lay;
  Shard shard;  // the shard as resolved: lmBegin, lmEnd, isRoot
  PartitionSets part;
  std::vector<int32_t> lmOfPoint;
  std::vector<int64_t> colStart, rowStart;  // per tile column into colTilesH / colRowsH, per tile row into rowColH
  std::vector<int32_t> colTilesH, colRowsH, rowColH;
  std::vector<uint8_t> tileFill;     // per tile: 1 = created by the symbolic factorization (zero in S)
  std::vector<int32_t> shardTiles;   // exact tiles of this (non-root) shard's partial system
  std::vector<int32_t> visRowOfPos;  // the visual factor row (vb_add_factors order) at every position of obCostOrder
  std::vector<int64_t> rsOff;        // offsets of the device rolling-shutter tables (capacities when rebuilt there)
  std::vector<double> piNoise;       // 6 per IMU, every IMU of the preintegration sources (device copy: pi.noise)
  std::vector<int32_t> bmRowOfPos;   // the base-map factor row (vb_add_basemap_factors order) at every sorted position
  std::vector<int32_t> loneLm;       // landmarks without a visual observation, ascending (Shard::loneList)
  int64_t nParams = 0, order = 0, nClear = 0, nTileEnt = 0, tileFirst = 0, tileCount = 0, nPairs = 0;
  int32_t nLevels = 0;
  int64_t costRsB[2] = {0, 0};  // obCostOrder: where the rolling-shutter observations of [obB, obE), [fB, fE) start
  ~Finalized() {
    for (hipGraphExec_t g : {sn[0].graph[0], sn[0].graph[1], sn[1].graph[0], sn[1].graph[1], sch[0].graph[0],
                             sch[0].graph[1], sch[1].graph[0], sch[1].graph[1]})
      if (g) hipGraphExecDestroy(g);
  }
};

// vb_optimize's speculative linearization (specEnqueue): the next iteration's rolling-shutter rebuild
// and linearization are queued behind this iteration's cost pass, before the host reads its scalars,
// into a second tile store, ResultCache, gradient and rolling-shutter table set (and reduction /
// error slots red[48, 64), err[4, 6)); they are swapped in when the step is accepted at full size
// (specCommit), and left unused otherwise (the host then takes the step-rescaling path, which needs
// this iteration's factor, cache and tables as they are).  Dropped only when its own preparation fails, or with
// the handle -- never after a specCommit: the pointers it swaps with Finalized::d need both owners to the end.
struct SpecState {
  DevOwner mem;
  double *tilesAlt = nullptr, *cacheAlt = nullptr, *gRedAlt = nullptr;
  double *rsSAlt = nullptr, *rsIAlt = nullptr, *rsGAlt = nullptr;
  int32_t* rsNAlt = nullptr;
  hipStream_t stR = nullptr;  // the scalar readback, beside the speculative work
  hipEvent_t evCost = nullptr, evS[2][4] = {};
  double* hostRed = nullptr;  // pinned readback buffer: red[0, 17), then err[0, 2) as int32
};

// the PCG path's buffers (pcgPrepare): made at its first use, grown at a preconditioner type's first use
struct PcgState {
  DevOwner mem;
  int32_t *symvTilesD = nullptr, *symvRCD = nullptr;  // the tiles of S (no fill) and their (row, column)
  int64_t nSymv = 0;
  double *pcgR = nullptr, *pcgZ = nullptr, *pcgP = nullptr, *pcgAp = nullptr, *pcgB = nullptr;
  double *jacL = nullptr, *tilesGS = nullptr;  // Jacobi block factors / Gauss-Seidel pseudo-factor
  // LowerPrecSolvePrecond (lowprec.hip): fp32 factor tiles, fp32 diagonal-tile inverses, fp32 vector
  float *lpTiles = nullptr, *lpLinv = nullptr, *lpT = nullptr;
};

// point refinement groups (built at the first vb_refine_points): observations by point
struct RefineState {
  DevOwner mem;
  int64_t nRefG = 0;
  int64_t* refStartD = nullptr;
  int32_t *refObsD = nullptr, *refPtD = nullptr;
  double *refBackD = nullptr, *refAccD = nullptr;
};

// the residual report's device state (report.hip), made at its first call
struct ReportState {
  DevOwner mem;
  int32_t* posOfRow = nullptr;  // visual factor row -> position of obCostOrder
  int32_t* err = nullptr;       // bit 1: a rolling-shutter lookup out of range
  hipEvent_t ev[2] = {nullptr, nullptr};
  double histMs = 0.0;  // device time of the last vb_error_histogram's kernels
};

// the non-linearity inspection (inspect.hip): its device state, made at its first call, and the last result
struct InspectState {
  DevOwner mem;
  int32_t *rowOfPos = nullptr, *posIdent = nullptr;  // position of obCostOrder -> visual row; the identity map
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};  // x0 [0, 1], x1 [2, 3], selection [3, 4]
  double ms[3] = {0.0, 0.0, 0.0};  // x0 pass, x1 pass, selection of the last vb_inspect_nonlinearities
  int32_t nFound = 0;
  int64_t nCompared = 0;
  int32_t kinds[VB_INSPECT_MAX_K];
  int64_t rows[VB_INSPECT_MAX_K];
  double score[VB_INSPECT_MAX_K], v0[VB_INSPECT_MAX_K], delta[VB_INSPECT_MAX_K], v1[VB_INSPECT_MAX_K], gnorm[VB_INSPECT_MAX_K];
};

// per-kernel-family device timing (vb_profile_kernel): event pairs around every launch
struct ProfState {
  DevOwner mem;
  int family = -1;
  std::vector<hipEvent_t> ev;
  size_t used = 0;
  size_t done = 0;    // leading ev entries known complete, harvested after the next enqueue
  size_t atCost = 0;  // profiled event pairs recorded before evCost
  int64_t launches = 0;
  double ms = 0.0, busyMs = 0.0;  // summed launch durations; the union of the launches' intervals
};

// destroyed in reverse order: the lazy groups, then `fin`, the streams last
struct vb_handle_s {
  vb_config cfg;
  Streams str;
  Problem prob;
  Tuning tune;
  RunState run;
  std::unique_ptr<Finalized> fin;
  std::unique_ptr<SpecState> spec;
  std::unique_ptr<PcgState> pcg;
  std::unique_ptr<RefineState> refine;
  std::unique_ptr<ReportState> rep;
  std::unique_ptr<InspectState> ins;
  ProfState prof;
};

// ---------------------------------------------------------------- shared host functions
#include "host_decl.hpp"
