// Declarations of the host functions the engine's translation units share (host.hpp), each group under the
// file that defines it.
#pragma once

namespace viba_host {
// kernel families for vb_profile_kernel
enum { KF_VISUAL_LIN = 0, KF_LANDMARK, KF_SCHUR, KF_POTRF, KF_GEMM, KF_FWD, KF_BWD, KF_BACKSUB, KF_VISUAL_COST,
       KF_SMALL, KF_TRSM, KF_SYMV, KF_COUNT };

inline void profBegin(vb_handle h, int fam) {
  if (h->prof.family != fam) return;
  if (h->prof.used + 2 > h->prof.ev.size()) {
    for (int i = 0; i < 256; i++) {
      hipEvent_t e;
      (void)h->prof.mem.event(&e);
      h->prof.ev.push_back(e);
    }
  }
  g_prof.start = h->prof.ev[h->prof.used], g_prof.stop = h->prof.ev[h->prof.used + 1], g_prof.consumed = false;
}
inline void profEnd(vb_handle h, int fam) {
  if (h->prof.family != fam) return;
  if (g_prof.consumed) h->prof.used += 2;  // the wrapper launched the family's kernel with the events
  g_prof = ProfSlot();
}
// kernel-family event timing and error words (api.hip)
float profPairMs(hipEvent_t a, hipEvent_t b);
double elapsed(hipEvent_t a, hipEvent_t b);
void profHarvest(vb_handle h);
void profHarvestPrefix(vb_handle h, size_t n);
int checkErr(vb_handle h);
int errFromWords(vb_handle h, const int32_t* ee);
int readRed(vb_handle h, double* out, int i0, int n);
int readRedErr(vb_handle h, double* out, int n);
// numeric phases (api.hip)
bool smallHere(vb_handle h, int mode);
// the factorization and solve drivers (factor_host.hip)
bool fwdFused(vb_handle h);
int factorReduced(vb_handle h, int which = 0);
int solveReduced(vb_handle h, int which = 0, int phases = 3);
void backSubstitute(vb_handle h, int which);
// the iterative reduced solve (pcg_host.hip)
bool pcgMode(vb_handle h);
int precondInit(vb_handle h);
int pcgSolve(vb_handle h);
// the residual report's entry checks and device state, its error word (report.hip)
int reportCommon(vb_handle h, const char* what);
int checkReportErr(vb_handle h);
// vb_inspect_nonlinearities into the handle's InspectState (inspect.hip); kInspectStop: the private return of
// vb_optimize's iteration primitive that ends the run after the inspected iteration
constexpr int kInspectStop = 1;
int inspectRun(vb_handle h, int which, uint32_t kindMask, int32_t k);
// vb_finalize (finalize.hip)
int doFinalize(vb_handle h);
// is the whole problem on this handle (no landmark shard, no partition)?  vb_refine_points alone accepts a
// vb_set_landmark_shard call that names every landmark on the root (shardCall = false)
inline bool wholeProblem(vb_handle h, bool shardCall = true) {
  const Dev& d = h->fin->d;
  return !(h->prob.partSet || (shardCall && h->prob.sharded) || d.lmB != 0 || d.lmE != d.nPts || !h->fin->shard.isRoot);
}
// capacity of a rolling-shutter table that is rebuilt on the device: the IMU samples (stamps t[0, n) [ns]) of
// [mid - half, mid + half] [us] widened by 20 ms on both sides (the reference-time offsets of the calibration
// move the gyro boundaries by far less), + 4
inline int64_t rsTableCapacity(const int64_t* t, int64_t n, int64_t midUs, int64_t halfUs) {
  const int64_t kWidenNs = 20000000;
  const int64_t a = (midUs - halfUs) * 1000 - kWidenNs, b = (midUs + halfUs) * 1000 + kWidenNs;
  return (std::upper_bound(t, t + n, b) - std::lower_bound(t, t + n, a)) + 4;
}
}  // namespace viba_host

extern "C" {
// queued phases (api.hip; C linkage, defined in its C-ABI block)
int clearReduced(vb_handle h, const Dev& d, hipStream_t zs);
int rsUpdateAsync(vb_handle h, bool tables = true, bool preint = false);
int linearizeBody(vb_handle h, const Dev& d, int update_cache, int dont_retry_failed, hipEvent_t evA, hipEvent_t evB,
                  bool early = false);
int linearizeEnqueue(vb_handle h, int update_cache, int dont_retry_failed);
int assembleEnqueue(vb_handle h, double lambda);
int dampFactorSolveEnqueue(vb_handle h, double lambda, bool clearErr);
int applyStepEnqueue(vb_handle h, int which, int e0, int e1);
int costEnqueue(vb_handle h, int comparable, bool clearErr);
int costFusedEnqueue(vb_handle h);
void costStats(vb_handle h, const double* r, double* cost, vb_cost_stats* stats);
// vb_optimize's speculation (optimize.hip)
Dev specDev(vb_handle h);
bool specPrepare(vb_handle h);
int specEnqueue(vb_handle h, int dontRetry, int p, bool early, bool rsDone = false, bool fuseCost = false);
int specEarly(vb_handle h, bool cleared = false, bool storeCleared = false);
void specCommit(vb_handle h);
int readIterScalars(vb_handle h, double* out, int n);
}
