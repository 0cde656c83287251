// Host side of the HIP LM engine: the C-ABI (include/viba_hip.h) and the queued numeric phases.  All numeric
// work runs in HIP kernels on the handle's streams; the host only orders launches and reads back scalars.  The
// factorization and solve drivers are factor_host.hip, the PCG driver pcg_host.hip, the Levenberg-Marquardt loop
// optimize.hip over lm_controller.hpp, vb_finalize finalize.hip, the multi-process entries multi.hip.
#include "host.hpp"

namespace viba {
ProfSlot g_prof;
}

namespace viba_host {

// duration of one profiled launch.  The stop event of a hipExtLaunchKernelGGL launch can still report
// hipErrorNotReady after a wait on a later event of the same stream (about a quarter of the pairs read
// right after vb_optimize's scalar read did, and counted 0 ms: the event-timed fan-in average came out
// 26% low against rocprofv3); such a pair is read again after hipEventSynchronize.
float profPairMs(hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  if (hipEventElapsedTime(&ms, a, b) == hipErrorNotReady) {
    (void)hipEventSynchronize(b);
    (void)hipEventSynchronize(a);
    ms = 0;
    (void)hipEventElapsedTime(&ms, a, b);
  }
  return ms;
}
// the first n recorded pairs into the totals: the summed launch durations, and the family's busy time, the
// union of the launches' intervals (launches on several streams overlap: the factorization's streams)
void profAccumulate(vb_handle h, size_t n) {
  std::vector<std::pair<double, double>> iv;
  for (size_t i = 0; i < n; i += 2) {
    const float ms = profPairMs(h->prof.ev[i], h->prof.ev[i + 1]);
    h->prof.ms += ms;
    h->prof.launches++;
    // the launch's start against the first one's, with the same not-ready retry as its duration (a
    // not-ready pair read as 0 would place the launch at the origin and shrink the busy union)
    const float t0 = i > 0 ? profPairMs(h->prof.ev[0], h->prof.ev[i]) : 0.0f;
    iv.push_back({(double)t0, (double)t0 + ms});
  }
  std::sort(iv.begin(), iv.end());
  double end = -1e300;
  for (const auto& x : iv) {
    if (x.first > end) h->prof.busyMs += x.second - x.first, end = x.second;
    else if (x.second > end) h->prof.busyMs += x.second - end, end = x.second;
  }
}
// harvest recorded pairs (call after a stream synchronisation)
void profHarvest(vb_handle h) {
  if (h->prof.family < 0 || h->prof.used == 0) return;
  (void)hipStreamSynchronize(h->str.st);
  profAccumulate(h, h->prof.used);
  h->prof.used = 0, h->prof.done = 0;
}
// harvest the first n entries (complete at the last stream sync) after the next iteration's work is
// queued, so the host reads the event times while the device runs instead of between two iterations;
// the entries still pending move to the front
void profHarvestPrefix(vb_handle h, size_t n) {
  if (h->prof.family < 0 || n == 0 || n > h->prof.used) return;
  profAccumulate(h, n);
  std::rotate(h->prof.ev.begin(), h->prof.ev.begin() + n, h->prof.ev.begin() + h->prof.used);
  h->prof.used -= n, h->prof.done = 0;
}

int checkRsErr(vb_handle h, int32_t e);
int checkErr(vb_handle h) {
  int32_t ee[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(ee, h->fin->d.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  return errFromWords(h, ee);
}
int errFromWords(vb_handle h, const int32_t* ee) {
  h->run.lastWords[0] = ee[0], h->run.lastWords[1] = ee[1];
  const int32_t e = ee[0];
  if (int rc = checkRsErr(h, ee[1])) return rc;
  // in causal order within an iteration: the linearization, the elimination and factorization, then the
  // cost pass at the stepped variables (whose lookups a broken step can push out of range)
  if (e & 1) return fail(VB_E_RANGE, "RollingShutterData::getEstimate: out of range");
  if (e & 2) return fail(VB_E_NUMERIC, "landmark 3x3 Cholesky breakdown");
  if (e & 8) return fail(VB_E_NUMERIC, "reduced system Cholesky breakdown (not positive definite)");
  if (e & 4) return fail(VB_E_STATE, "internal: Schur contribution outside the symbolic structure");
  if (e & 16) return fail(VB_E_HIP, "internal: triangular-solve hand-off timed out");
  if (e & 32) return fail(VB_E_RANGE, "RollingShutterData::getEstimate: out of range (cost pass)");
  return 0;
}

// errors of the last device rolling-shutter rebuild (rs.hip): the reference throws there
int checkRsErr(vb_handle h, int32_t e) {
  if (e & 1) return fail(VB_E_RANGE, "enumIntegrationSteps: IMU measurements do not cover the rolling-shutter interval");
  if (e & 2) return fail(VB_E_NUMERIC, "RollingShutterData::compute: non-increasing sample times");
  if (e & 4) return fail(VB_E_STATE, "internal: rolling-shutter table capacity exceeded");
  if (e & 8) return fail(VB_E_RANGE, "enumIntegrationSteps: IMU measurements do not cover a preintegration interval");
  if (e & 16) return fail(VB_E_NUMERIC, "computePreIntegration: covariance not positive definite");
  return 0;
}

int readRed(vb_handle h, double* out, int i0, int n) {
  HIPCHK(hipMemcpyAsync(out, h->fin->d.red + i0, n * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  profHarvest(h);
  return 0;
}
// vb_optimize's one read per iteration: the scalars red[0, n) and the error words in one stream sync;
// the profiled events stay for profHarvestPrefix after the next enqueue
int readRedErr(vb_handle h, double* out, int n) {
  int32_t ee[2] = {0, 0};
  HIPCHK(hipMemcpyAsync(out, h->fin->d.red, n * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipMemcpyAsync(ee, h->fin->d.err, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  h->prof.done = h->prof.used;
  return errFromWords(h, ee);
}

// ------------------------------------------------------------------ numeric phases
// small factors (root only) on the side stream; joinSmall makes the main stream wait for them
bool smallHere(vb_handle h, int mode) { return h->fin->shard.isRoot || (h->prob.partSet && mode != 2); }
void forkSmall(vb_handle h, int mode, double* gOut) {
  if (!smallHere(h, mode)) return;
  (void)hipEventRecord(h->str.evFork, h->str.st);
  (void)hipStreamWaitEvent(h->str.st2, h->str.evFork, 0);
  launch_small(h->fin->d, mode, gOut, h->str.st2);
  (void)hipEventRecord(h->str.evJoin, h->str.st2);
}
void joinSmall(vb_handle h) {
  if (h->fin->shard.isRoot || h->prob.partSet) (void)hipStreamWaitEvent(h->str.st, h->str.evJoin, 0);
}

// visual kernels over this shard's observations (+ the root's constant-point observations)
void visualLinShard(vb_handle h, const Dev& d, int updateCache, int dontRetry) {
  profBegin(h, KF_VISUAL_LIN);
  launch_visual_lin(d, updateCache, dontRetry, d.obB, d.obE, h->str.st);
  launch_visual_lin(d, updateCache, dontRetry, d.fB, d.fE, h->str.st);
  profEnd(h, KF_VISUAL_LIN);
  launch_basemap_lin(d, updateCache, dontRetry, h->str.st);
  launch_fold_red(d, h->str.st);
}
void visualCostShard(vb_handle h, int comparable) {
  const Dev& d = h->fin->d;
  profBegin(h, KF_VISUAL_COST);
  launch_visual_cost(d, comparable, d.obB, d.obE, h->str.st);
  launch_visual_cost(d, comparable, d.fB, d.fE, h->str.st);
  profEnd(h, KF_VISUAL_COST);
  launch_basemap_cost(d, comparable, h->str.st);
  launch_fold_red(d, h->str.st);
}

double elapsed(hipEvent_t a, hipEvent_t b) { return profPairMs(a, b); }

}  // namespace viba_host

// ====================================================================== C ABI
extern "C" {

const char* vb_last_error(void) { return g_err.c_str(); }
int vb_factor_num_vars(int k) { return (k >= 0 && k < 14) ? kNumVars[k] : -1; }
int vb_factor_num_consts(int k) { return (k >= 0 && k < 14) ? kNumConsts[k] : -1; }

void vb_default_config(vb_config* c) {
  c->reproj_loss_radius = 1.0, c->reproj_loss_cutoff = 3.0;
  c->imu_loss_radius = INFINITY, c->imu_loss_cutoff = INFINITY;
  c->imu_calib_options = VB_IMU_OPT_ALL, c->device = 0, c->tile = 0, c->reserved = 0;
}
void vb_default_settings(vb_settings* s) {
  s->max_num_iterations = 50, s->stop_if_no_improvement_for = 3, s->distance_from_troubled_iteration = 3;
  s->max_step_factor_attempts = 2, s->try_sub_step = 1, s->verbose = 0;
  s->absolute_cost_tolerance = 1e-8, s->relative_cost_tolerance = 1e-10, s->variables_tolerance = 1e-5;
  s->damping = 1e-5, s->damping_adjust_on_fail = 2.5, s->damping_adjust_on_good_step = 0.7;
  s->damping_adjust_on_average_step = 1.5, s->damping_max = 1e8, s->damping_min = 1e-9;
  s->min_relative_cost_reduction = 0.3, s->step_factor_decrease = 0.3, s->min_step_factor_for_good = 0.7;
}

int vb_create(const vb_config* cfg, vb_handle* out) {
  if (!out) return fail(VB_E_ARG, "null output handle");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(VB_E_HIP, "no HIP device available");
  vb_config c;
  if (cfg) c = *cfg;
  else vb_default_config(&c);
  if (c.tile != 0 && c.tile != TS) return fail(VB_E_UNSUPPORTED, "only tile size 64 is built");
  if (c.device < 0 || c.device >= ndev) return fail(VB_E_ARG, "bad device ordinal");
  HIPCHK(hipSetDevice(c.device));
  std::unique_ptr<vb_handle_s> hp(new vb_handle_s());  // (a failure below gives back what was made so far)
  vb_handle h = hp.get();
  h->cfg = c;
  if (const char* e = getenv("VIBA_SPEC_EARLY")) h->tune.specEarly = e[0] != '0';
  if (const char* e = getenv("VIBA_COST_FUSE")) h->tune.costFuse = e[0] != '0';
  if (const char* e = getenv("VIBA_CLEAR_IN_FACTOR")) h->tune.clearInFactor = e[0] != '0';
  if (const char* e = getenv("VIBA_DEBUG_SPEC_FAIL")) h->tune.specFailDebug = e[0] == '1';
  if (const char* e = getenv("VIBA_SUPERNODE")) h->tune.useSn = e[0] == '1';
  if (const char* e = getenv("VIBA_SN_STREAMS")) h->tune.snStreams = std::max(1, std::min(4, atoi(e)));
  {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, c.device) == hipSuccess && prop.multiProcessorCount > 0)
      h->tune.numCUs = prop.multiProcessorCount;
  }
  Streams& s = h->str;
  DevOwner& m = s.mem;
  bool bad = false;
  for (hipStream_t* q : {&s.st, &s.st2, &s.stZ, &s.stF}) bad = bad || m.stream(q);
  for (auto& e : s.ev) bad = bad || m.event(&e);
  for (hipEvent_t* e : {&s.evFork, &s.evJoin, &s.evZero, &s.evSmallE, &s.evZJoin, &s.evSnFork, &s.evClr, &s.evClrDone,
                        &s.evInvDone, &s.evStep, &s.evRs, &s.evInvAt[0], &s.evInvAt[1], &s.evInvAt[2], &s.evInvAt[3],
                        &s.evSnLvl[0], &s.evSnLvl[1], &s.evSnLvl[2], &s.evSnLvl[3]})
    bad = bad || m.event(e, hipEventDisableTiming);
  if (bad) return devFail(m, "vb_create: stream / event");
  *out = hp.release();
  return 0;
}

int vb_destroy(vb_handle h) {
  if (!h) return 0;
  hipSetDevice(h->cfg.device);
  hipStreamSynchronize(h->str.st);
  delete h;  // its groups (vb_handle_s) give back every graph, buffer, event and stream
  return 0;
}

int vb_set_vars(vb_handle h, int kind, int64_t n, const double* data, const uint8_t* constant) {
  if (!h || kind < 0 || kind >= 9 || n < 0 || (n > 0 && !data)) return fail(VB_E_ARG, "bad vb_set_vars arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_set_vars after vb_finalize");
  h->prob.data[kind].assign(data, data + n * kVarData[kind]);
  h->prob.cst[kind].assign(n, 0);
  if (constant) std::copy(constant, constant + n, h->prob.cst[kind].begin());
  return 0;
}

int vb_add_factors(vb_handle h, int kind, int64_t n, const int32_t* var_idx, const int32_t* ivals,
                   const double* consts) {
  if (!h || kind < 0 || kind >= 14 || n < 0 || (n > 0 && (!var_idx || !consts)))
    return fail(VB_E_ARG, "bad vb_add_factors arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_add_factors after vb_finalize");
  h->prob.fvars[kind].insert(h->prob.fvars[kind].end(), var_idx, var_idx + n * kNumVars[kind]);
  for (int64_t i = 0; i < n; i++) h->prob.fint[kind].push_back(ivals ? ivals[i] : -1);
  h->prob.fconst[kind].insert(h->prob.fconst[kind].end(), consts, consts + n * kNumConsts[kind]);
  return 0;
}

// ---- base-map visual factors (BaseMapVisualFactor.{h,cpp}; MultiSessionProblemImpl.h:19-40)
int vb_set_basemap(vb_handle h, int64_t n_keyrigs, const double* T_bodyImu_world7, int64_t n_cameras,
                   const int32_t* keyrig_of_camera, const double* T_cam_bodyImu7, const double* cam_data) {
  if (!h || n_keyrigs < 0 || n_cameras < 0 || (n_keyrigs > 0 && !T_bodyImu_world7) ||
      (n_cameras > 0 && (!keyrig_of_camera || !T_cam_bodyImu7 || !cam_data)))
    return fail(VB_E_ARG, "bad vb_set_basemap arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_set_basemap after vb_finalize");
  if (n_keyrigs > INT32_MAX || n_cameras > INT32_MAX) return fail(VB_E_ARG, "vb_set_basemap: too many key rigs / cameras");
  for (int64_t c = 0; c < n_cameras; c++)
    if (keyrig_of_camera[c] < 0 || keyrig_of_camera[c] >= n_keyrigs) return fail(VB_E_ARG, "vb_set_basemap: camera names an unknown key rig");
  for (const int32_t c : h->prob.bmCamera)
    if (c >= n_cameras) return fail(VB_E_ARG, "vb_set_basemap: a base-map factor names a camera outside the new base map");
  Problem& P = h->prob;
  P.bmRig.assign(T_bodyImu_world7, T_bodyImu_world7 + n_keyrigs * 7);
  P.bmCamRig.assign(keyrig_of_camera, keyrig_of_camera + n_cameras);
  P.bmCamT.assign(T_cam_bodyImu7, T_cam_bodyImu7 + n_cameras * 7);
  P.bmCam.assign(cam_data, cam_data + n_cameras * VB_CAM_DATA);
  P.bmSet = true;
  return 0;
}

int vb_add_basemap_factors(vb_handle h, int64_t n, const int32_t* point, const int32_t* camera, const double* consts6) {
  if (!h || n < 0 || (n > 0 && (!point || !camera || !consts6))) return fail(VB_E_ARG, "bad vb_add_basemap_factors arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_add_basemap_factors after vb_finalize");
  if (n == 0) return 0;
  if (!h->prob.bmSet) return fail(VB_E_ARG, "vb_add_basemap_factors before vb_set_basemap");
  if (h->prob.sharded || h->prob.partSet)
    return fail(VB_E_UNSUPPORTED, "base-map factors need the whole problem on one handle (no shard / partition)");
  const int64_t nCam = (int64_t)h->prob.bmCamRig.size();
  for (int64_t i = 0; i < n; i++) {
    if (camera[i] < 0 || camera[i] >= nCam) return fail(VB_E_ARG, "vb_add_basemap_factors: camera index out of range");
    if (point[i] < 0) return fail(VB_E_ARG, "vb_add_basemap_factors: point index out of range");
  }
  // (the points are checked against the point variables at vb_finalize, as vb_add_factors' handles are)
  h->prob.bmPoint.insert(h->prob.bmPoint.end(), point, point + n);
  h->prob.bmCamera.insert(h->prob.bmCamera.end(), camera, camera + n);
  h->prob.bmConst.insert(h->prob.bmConst.end(), consts6, consts6 + n * 6);
  return 0;
}

int vb_num_basemap_factors(vb_handle h, int64_t* n) {
  if (!h || !n) return fail(VB_E_ARG, "vb_num_basemap_factors: null argument");
  *n = (int64_t)h->prob.bmPoint.size();
  return 0;
}

int vb_set_rs_tables(vb_handle h, int32_t nt, const int64_t* offsets, const double* samples, const double* interp,
                     const double* gravity) {
  if (!h || nt < 0) return fail(VB_E_ARG, "bad vb_set_rs_tables arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_set_rs_tables after vb_finalize");
  if (h->prob.rsDevice) return fail(VB_E_STATE, "vb_set_rs_tables after vb_set_rs_rigs (tables are rebuilt on the device)");
  h->prob.nRS = nt;
  h->prob.rsOff.assign(offsets, offsets + nt + 1);
  const int64_t ns = offsets[nt];
  h->prob.rsS.assign(samples, samples + ns * 11);
  h->prob.rsI.assign(interp, interp + (ns - nt) * 9);
  h->prob.rsG.assign(gravity, gravity + nt * 3);
  for (int t = 0; t < nt; t++)
    if (offsets[t + 1] - offsets[t] < 2) return fail(VB_E_ARG, "RS table needs >= 2 samples");
  return 0;
}

int vb_set_imu_measurements(vb_handle h, int64_t n, const int64_t* timestamp_ns, const double* gyro,
                             const double* accel) {
  if (!h || n < 0 || (n && (!timestamp_ns || !gyro || !accel))) return fail(VB_E_ARG, "bad vb_set_imu_measurements arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_set_imu_measurements after vb_finalize");
  h->prob.imuT.assign(timestamp_ns, timestamp_ns + n);
  h->prob.imuV.resize((size_t)n * 6);
  for (int64_t i = 0; i < n; i++) {
    if (i && timestamp_ns[i] <= timestamp_ns[i - 1]) return fail(VB_E_ARG, "IMU timestamps must increase");
    for (int k = 0; k < 3; k++) h->prob.imuV[6 * i + k] = gyro[3 * i + k], h->prob.imuV[6 * i + 3 + k] = accel[3 * i + k];
  }
  return 0;
}

int vb_set_rs_rigs(vb_handle h, int32_t nt, const int64_t* mid_us, const int64_t* half_us, const int32_t* imu_calib,
                   int32_t gravity_var) {
  if (!h || nt < 0 || (nt && (!mid_us || !half_us || !imu_calib))) return fail(VB_E_ARG, "bad vb_set_rs_rigs arguments");
  if (h->fin) return fail(VB_E_STATE, "vb_set_rs_rigs after vb_finalize");
  if (h->prob.imuT.empty() && nt) return fail(VB_E_STATE, "vb_set_rs_rigs needs vb_set_imu_measurements first");
  const int64_t nCalib = (int64_t)h->prob.data[6].size() / 32, nGrav = (int64_t)h->prob.data[8].size() / 4;
  if (gravity_var < 0 || gravity_var >= nGrav) return fail(VB_E_ARG, "vb_set_rs_rigs: unknown gravity variable");
  for (int32_t t = 0; t < nt; t++) {
    if (imu_calib[t] < 0 || imu_calib[t] >= nCalib) return fail(VB_E_ARG, "vb_set_rs_rigs: unknown IMU calibration");
    if (half_us[t] <= 0) return fail(VB_E_ARG, "vb_set_rs_rigs: half length must be positive");
  }
  h->prob.nRS = nt;
  h->prob.rsMid.assign(mid_us, mid_us + nt);
  h->prob.rsHalf.assign(half_us, half_us + nt);
  h->prob.rsCalib.assign(imu_calib, imu_calib + nt);
  h->prob.rsGravVar = gravity_var;
  h->prob.rsDevice = true;
  h->prob.rsS.clear(), h->prob.rsI.clear(), h->prob.rsG.clear(), h->prob.rsOff.clear();
  return 0;
}

// enqueue the rebuild; its errors surface at the next synchronising check (checkErr reads err[1])
int rsUpdateAsync(vb_handle h, bool tables, bool preint) {
  HIPCHK(hipMemsetAsync(h->fin->d.err + 1, 0, sizeof(int32_t), h->str.st));
  HIPCHK(hipEventRecord(h->str.ev[8], h->str.st));
  if (tables) launch_rs_build(h->fin->d, h->str.st);
  if (preint) launch_preint(h->fin->d, h->fin->pi, h->str.st);
  HIPCHK(hipEventRecord(h->str.ev[9], h->str.st));
  h->run.rsTimed = true;
  return 0;
}

int vb_update_rs_tables(vb_handle h) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_update_rs_tables before vb_finalize");
  if (!h->prob.rsDevice) return fail(VB_E_STATE, "vb_update_rs_tables without vb_set_rs_rigs");
  if (int rc = rsUpdateAsync(h)) return rc;
  if (h->run.deferred) return 0;
  int32_t e = 0;
  HIPCHK(hipMemcpyAsync(&e, h->fin->d.err + 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  return checkRsErr(h, e);
}

int vb_set_imu_stream(vb_handle h, int imu, int64_t n, const int64_t* timestamp_ns, const double* gyro,
                      const double* accel) {
  if (!h || imu < 0 || n < 0 || (n && (!timestamp_ns || !gyro || !accel))) return fail(VB_E_ARG, "bad vb_set_imu_stream arguments");
  if (imu == 0) return vb_set_imu_measurements(h, n, timestamp_ns, gyro, accel);
  if (h->fin) return fail(VB_E_STATE, "vb_set_imu_stream after vb_finalize");
  if ((int)h->prob.piT.size() <= imu) h->prob.piT.resize(imu + 1), h->prob.piV.resize(imu + 1);
  std::vector<int64_t>& t = h->prob.piT[imu];
  std::vector<double>& v = h->prob.piV[imu];
  t.assign(timestamp_ns, timestamp_ns + n);
  v.resize((size_t)n * 6);
  for (int64_t i = 0; i < n; i++) {
    if (i && timestamp_ns[i] <= timestamp_ns[i - 1]) return fail(VB_E_ARG, "IMU timestamps must increase");
    for (int k = 0; k < 3; k++) v[6 * i + k] = gyro[3 * i + k], v[6 * i + 3 + k] = accel[3 * i + k];
  }
  return 0;
}

int vb_set_imu_noise(vb_handle h, int imu, const double* accel_var, const double* gyro_var) {
  if (!h || imu < 0 || !accel_var || !gyro_var) return fail(VB_E_ARG, "bad vb_set_imu_noise arguments");
  std::vector<double>& noise = h->fin ? h->fin->piNoise : h->prob.piNoise;
  if (h->fin && (h->fin->pi.n == 0 || 6 * imu + 6 > (int)noise.size()))
    return fail(VB_E_STATE, "vb_set_imu_noise after vb_finalize for an IMU without preintegration sources");
  if ((int)noise.size() < 6 * imu + 6) {
    const size_t was = noise.size();
    noise.resize(6 * imu + 6);
    for (size_t k = was; k < noise.size(); k++) noise[k] = kDefaultImuNoise[k % 6];
  }
  for (int k = 0; k < 3; k++) noise[6 * imu + k] = accel_var[k], noise[6 * imu + 3 + k] = gyro_var[k];
  if (h->fin) {
    HIPCHK(hipMemcpyAsync(const_cast<double*>(h->fin->pi.noise) + 6 * imu, &noise[6 * imu], 6 * sizeof(double),
                          hipMemcpyHostToDevice, h->str.st));
    HIPCHK(hipStreamSynchronize(h->str.st));
  }
  return 0;
}

int vb_set_preint_sources(vb_handle h, int kind, int64_t n, const int32_t* imu, const int64_t* t0_us,
                          const int64_t* t1_us) {
  if (!h || kind < VB_F_IMU || kind > VB_F_IMU_SEC_SPLIT || n < 0 || (n && (!imu || !t0_us || !t1_us)))
    return fail(VB_E_ARG, "bad vb_set_preint_sources arguments (inertial kinds only)");
  if (h->fin) return fail(VB_E_STATE, "vb_set_preint_sources after vb_finalize");
  if (n != (int64_t)h->prob.fint[kind].size()) return fail(VB_E_ARG, "vb_set_preint_sources: one source per factor row of the kind");
  std::vector<PreintSrc> keep;
  for (const PreintSrc& p : h->prob.piSrc)
    if (p.kind != kind) keep.push_back(p);
  for (int64_t r = 0; r < n; r++) {
    if (imu[r] < 0) return fail(VB_E_ARG, "vb_set_preint_sources: bad IMU index");
    if (t1_us[r] <= t0_us[r]) return fail(VB_E_ARG, "vb_set_preint_sources: empty interval");
    keep.push_back(PreintSrc{kind, imu[r], r, t0_us[r], t1_us[r]});
  }
  h->prob.piSrc.swap(keep);
  return 0;
}

int vb_set_recompute_preint(vb_handle h, int on) {
  if (!h) return fail(VB_E_ARG, "null handle");
  h->prob.recomputePreint = on != 0;
  return 0;
}

int vb_update_preintegrations(vb_handle h) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_update_preintegrations before vb_finalize");
  if (h->fin->pi.n == 0) return 0;
  if (int rc = rsUpdateAsync(h, false, true)) return rc;
  int32_t e = 0;
  HIPCHK(hipMemcpyAsync(&e, h->fin->d.err + 1, sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  return checkRsErr(h, e);
}

int vb_get_factor_consts(vb_handle h, int kind, int64_t row, double* out) {
  if (!h || kind < 0 || kind >= 14 || !out || row < 0 || row >= (int64_t)h->prob.fint[kind].size())
    return fail(VB_E_ARG, "bad vb_get_factor_consts arguments");
  if (!h->fin || kind == VB_F_VISUAL) {
    std::copy(&h->prob.fconst[kind][row * kNumConsts[kind]], &h->prob.fconst[kind][(row + 1) * kNumConsts[kind]], out);
    return 0;
  }
  const SmallFactors& sf = h->fin->d.sf[kind];
  HIPCHK(hipMemcpyAsync(out, sf.consts + row * sf.nc, kNumConsts[kind] * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  return 0;
}

int vb_refine_points(vb_handle h, double* costs, int64_t* stats) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_refine_points before vb_finalize");
  Dev& d = h->fin->d;
  if (!wholeProblem(h, false))
    return fail(VB_E_UNSUPPORTED, "vb_refine_points needs the whole problem on this handle (no shard / partition)");
  if (!h->refine) {
    // observations grouped by point variable (refinePoints' perPointTracks, PointRefinement.cpp:20-45),
    // in device observation order
    std::vector<int32_t> obPt(d.nObs);
    if (d.nObs) HIPCHK(hipMemcpy(obPt.data(), d.obPt, d.nObs * sizeof(int32_t), hipMemcpyDeviceToHost));
    const int64_t nP = d.nvar[0];
    // (a point's base-map factors follow its visual ones, as entries -(position + 1): refine_eval)
    const std::vector<int32_t>& bmRow = h->fin->bmRowOfPos;
    const int64_t nBm = d.bm.n, nEnt = d.nObs + nBm;
    std::vector<int64_t> cnt(nP + 1, 0);
    for (int32_t p : obPt) cnt[p + 1]++;
    for (int64_t i = 0; i < nBm; i++) cnt[h->prob.bmPoint[bmRow[i]] + 1]++;
    for (int64_t p = 0; p < nP; p++) cnt[p + 1] += cnt[p];
    std::vector<int32_t> obs(nEnt);
    std::vector<int64_t> pos(cnt.begin(), cnt.end() - 1);
    for (int64_t o = 0; o < d.nObs; o++) obs[pos[obPt[o]]++] = (int32_t)o;
    for (int64_t i = 0; i < nBm; i++) obs[pos[h->prob.bmPoint[bmRow[i]]]++] = (int32_t)(-(i + 1));
    std::vector<int64_t> gs(1, 0);
    std::vector<int32_t> gp;
    for (int64_t p = 0; p < nP; p++)
      if (cnt[p + 1] > cnt[p]) gp.push_back((int32_t)p), gs.push_back(cnt[p + 1]);
    auto g = std::make_unique<RefineState>();
    g->nRefG = (int64_t)gp.size();
    DevOwner& m = g->mem;
    if (m.put(&g->refStartD, gs) || m.put(&g->refObsD, obs) || m.put(&g->refPtD, gp) ||
        m.zeroed(&g->refBackD, (size_t)nEnt) || m.zeroed(&g->refAccD, 8))
      return devFail(m, "vb_refine_points: device allocation");  // (g goes: the next call starts over)
    h->refine = std::move(g);
  }
  const RefineState& r = *h->refine;
  HIPCHK(hipMemsetAsync(r.refAccD, 0, 8 * sizeof(double), h->str.st));
  HIPCHK(hipMemsetAsync(d.err, 0, 2 * sizeof(int32_t), h->str.st));
  launch_refine_points(d, r.refStartD, r.refObsD, r.refPtD, r.nRefG, r.refBackD, r.refAccD, h->str.st);
  double acc[8];
  HIPCHK(hipMemcpyAsync(acc, r.refAccD, sizeof(acc), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  if (int rc = checkErr(h)) return rc;
  if (costs) costs[0] = acc[0], costs[1] = acc[1];
  if (stats) stats[0] = (int64_t)acc[2], stats[1] = (int64_t)acc[3], stats[2] = (int64_t)acc[4];
  h->run.linearized = false, h->run.factored = false;
  return 0;
}

int vb_get_rs_table(vb_handle h, int32_t t, int32_t* n_samples, double* samples, double* interp) {
  if (!h || !h->fin || !n_samples) return fail(VB_E_STATE, "vb_get_rs_table before vb_finalize");
  if (t < 0 || t >= h->prob.nRS) return fail(VB_E_ARG, "vb_get_rs_table: bad table index");
  int32_t n = 0;
  HIPCHK(hipMemcpyAsync(&n, h->fin->d.rsN + t, sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  *n_samples = n;
  const int64_t s0 = h->fin->rsOff[t];
  if (samples && n) HIPCHK(hipMemcpy(samples, h->fin->d.rsS + s0 * 11, (size_t)n * 11 * sizeof(double), hipMemcpyDeviceToHost));
  if (interp && n > 1)
    HIPCHK(hipMemcpy(interp, h->fin->d.rsI + (s0 - t) * 9, (size_t)(n - 1) * 9 * sizeof(double), hipMemcpyDeviceToHost));
  return 0;
}

int vb_finalize(vb_handle h) {
  if (!h) return fail(VB_E_ARG, "null handle");
  if (h->fin) return fail(VB_E_STATE, "already finalized");
  HIPCHK(hipSetDevice(h->cfg.device));
  return doFinalize(h);
}

int64_t vb_reduced_order(vb_handle h) { return !h ? -1 : h->fin ? h->fin->lay.nRedReal : 0; }
int64_t vb_total_order(vb_handle h) { return !h ? -1 : h->fin ? h->fin->order : 0; }

int vb_set_landmark_shard(vb_handle h, int64_t lm_begin, int64_t lm_end, int is_root) {
  if (!h) return fail(VB_E_ARG, "null handle");
  if (h->fin) return fail(VB_E_STATE, "vb_set_landmark_shard must precede vb_finalize");
  if (lm_begin < 0 || lm_begin > lm_end) return fail(VB_E_ARG, "bad landmark range");
  if (!h->prob.bmPoint.empty()) return fail(VB_E_UNSUPPORTED, "vb_set_landmark_shard on a handle with base-map factors");
  h->prob.lmBegin = lm_begin, h->prob.lmEnd = lm_end, h->prob.isRoot = is_root != 0, h->prob.sharded = true;
  return 0;
}

// the reduced system's clear on stream zs: the tiles no Schur item stores whole, the gradient, the
// padded diagonal
int clearReduced(vb_handle h, const Dev& d, hipStream_t zs) {
  if (h->fin->clearTilesD) {
    launch_zero_tiles(d.tiles, h->fin->clearTilesD, h->fin->nClear, zs);
  } else if (h->fin->part.zeroRuns.empty()) {
    HIPCHK(hipMemsetAsync(d.tiles, 0, (size_t)d.nTiles * TS * TS * sizeof(double), zs));
  } else {  // partitioned: colStart runs are tile-store index ranges (tiles stored column by column)
    for (const auto& r : h->fin->part.zeroRuns)
      HIPCHK(hipMemsetAsync(d.tiles + r.first * TS * TS, 0, (size_t)(r.second - r.first) * TS * TS * sizeof(double), zs));
  }
  HIPCHK(hipMemsetAsync(d.gRed, 0, (size_t)d.nT * TS * sizeof(double), zs));
  if (h->fin->shard.isRoot || h->prob.partSet) launch_pad_diag(d, h->fin->padRowsD, (int64_t)h->fin->lay.padRows.size(), zs);
  return 0;
}

// vb_linearize's device work over the buffers of `d` (Finalized::d, or the speculative copy of vb_optimize:
// another tile store, cache write buffer, reduction and error slots), no host read, no reset of the
// reduction / error slots (the caller's); events evA / evB bracket it.  early: the small factors'
// evaluation and the clear were queued on stZ already (specEarly)
int linearizeBody(vb_handle h, const Dev& d, int update_cache, int dont_retry_failed, hipEvent_t evA, hipEvent_t evB,
                  bool early) {
  const bool fuseCost = d.costS != nullptr;
  HIPCHK(hipEventRecord(evA, h->str.st));
  // the reduced system is cleared and the small factors assembled on the side stream while the visual
  // factors linearize on the main stream (they write only their records and the cost)
  const bool side = smallHere(h, 0);
  hipStream_t zs = side ? h->str.stZ : h->str.st;
  if (side && !early) {
    HIPCHK(hipEventRecord(h->str.evFork, h->str.st));
    HIPCHK(hipStreamWaitEvent(h->str.st2, h->str.evFork, 0));
    HIPCHK(hipStreamWaitEvent(h->str.stZ, h->str.evFork, 0));
    launch_small_eval(d, 0, d.gRed, h->str.st2);
  }
  if (!early)
    if (int rc = clearReduced(h, d, zs)) return rc;
  if (side && early) {
    // evaluation and clear done in order on stZ: the IMU kinds' assembly on st2 waits for both
    HIPCHK(hipEventRecord(h->str.evZero, h->str.stZ));
    HIPCHK(hipStreamWaitEvent(h->str.st2, h->str.evZero, 0));
    launch_small_assemble(d, 0, d.gRed, h->str.st2, 1);
    launch_small_assemble(d, 0, d.gRed, h->str.stZ, 2);
    HIPCHK(hipEventRecord(h->str.evJoin, h->str.st2));
    HIPCHK(hipEventRecord(h->str.evZJoin, h->str.stZ));
  } else if (side) {
    // the IMU kinds' assembly on st2, the other kinds' on stZ after the clear: both wait for the clear
    // and the evaluation
    HIPCHK(hipEventRecord(h->str.evZero, h->str.stZ));
    HIPCHK(hipEventRecord(h->str.evSmallE, h->str.st2));
    HIPCHK(hipStreamWaitEvent(h->str.st2, h->str.evZero, 0));
    HIPCHK(hipStreamWaitEvent(h->str.stZ, h->str.evSmallE, 0));
    launch_small_assemble(d, 0, d.gRed, h->str.st2, 1);
    launch_small_assemble(d, 0, d.gRed, h->str.stZ, 2);
    HIPCHK(hipEventRecord(h->str.evJoin, h->str.st2));
    HIPCHK(hipEventRecord(h->str.evZJoin, h->str.stZ));
  }
  visualLinShard(h, d, update_cache, dont_retry_failed);
  if (fuseCost) {  // the rest of vb_optimize's cost pass (costFusedEnqueue): its sums into red[1..4]
    launch_fold_red(h->fin->d, h->str.st);
    HIPCHK(hipEventRecord(h->str.ev[7], h->str.st));
    HIPCHK(hipEventRecord(h->spec->evCost, h->str.st));
    h->prof.atCost = h->prof.used;
  }
  joinSmall(h);
  if (side) HIPCHK(hipStreamWaitEvent(h->str.st, h->str.evZJoin, 0));
  HIPCHK(hipEventRecord(evB, h->str.st));
  return 0;
}
// cost in red[0], errors in err
int linearizeEnqueue(vb_handle h, int update_cache, int dont_retry_failed) {
  Dev& d = h->fin->d;
  HIPCHK(hipMemsetAsync(d.red, 0, 64 * sizeof(double), h->str.st));
  HIPCHK(hipMemsetAsync(d.err, 0, sizeof(int32_t), h->str.st));
  return linearizeBody(h, d, update_cache, dont_retry_failed, h->str.ev[0], h->str.ev[1]);
}

int vb_linearize(vb_handle h, int update_cache, int dont_retry_failed, double* cost) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_linearize before vb_finalize");
  if (int rc = linearizeEnqueue(h, update_cache, dont_retry_failed)) return rc;
  h->run.scalarsMarked = false;
  if (h->run.deferred) {  // cost in red[0]
    if (cost) *cost = std::nan("");
    h->run.linearized = true, h->run.factored = false;
    return 0;
  }
  double c = 0;
  if (int rc = readRed(h, &c, 0, 1)) return rc;
  if (int rc = checkErr(h)) return rc;
  h->run.times.linearize_ms = elapsed(h->str.ev[0], h->str.ev[1]);
  if (h->run.rsTimed) h->run.times.rs_update_ms = elapsed(h->str.ev[8], h->str.ev[9]), h->run.rsTimed = false;
  if (cost) *cost = c;
  h->run.linearized = true, h->run.factored = false;
  return 0;
}

// damp + eliminate the landmarks (of this shard) into the reduced system and its RHS: the observation-
// group Gram blocks on the side stream beside the landmark elimination (both stream records from HBM;
// neither reads what the other writes), joined before the tile products
int assembleEnqueue(vb_handle h, double lambda) {
  Dev& d = h->fin->d;
  const int addId = (h->fin->shard.isRoot || h->prob.partSet) ? 1 : 0;
  launch_damp(d, lambda, addId, h->str.st);
  HIPCHK(hipEventRecord(h->str.evFork, h->str.st));
  HIPCHK(hipStreamWaitEvent(h->str.st2, h->str.evFork, 0));
  launch_groups(d, lambda, h->str.st2);
  HIPCHK(hipEventRecord(h->str.evJoin, h->str.st2));
  profBegin(h, KF_LANDMARK);
  launch_landmark(d, lambda, 0, h->str.st);
  profEnd(h, KF_LANDMARK);
  HIPCHK(hipMemsetAsync(d.rhs, 0, (size_t)d.nT * TS * sizeof(double), h->str.st));
  HIPCHK(hipStreamWaitEvent(h->str.st, h->str.evJoin, 0));
  profBegin(h, KF_SCHUR);
  launch_schur_products(d, lambda, h->str.st);
  profEnd(h, KF_SCHUR);
  return 0;
}

// vb_damp_factor_solve's device work (model dot in red[16]); clearErr = false keeps the linearization's
// error bits for one check at the end of the iteration (vb_optimize)
int dampFactorSolveEnqueue(vb_handle h, double lambda, bool clearErr) {
  Dev& d = h->fin->d;
  if (clearErr) HIPCHK(hipMemsetAsync(d.err, 0, sizeof(int32_t), h->str.st));
  HIPCHK(hipEventRecord(h->str.ev[2], h->str.st));
  if (int rc = assembleEnqueue(h, lambda)) return rc;
  HIPCHK(hipEventRecord(h->str.ev[3], h->str.st));
  const bool fused = !pcgMode(h) && fwdFused(h);
  if (fused)  // the factorization runs the forward solve of rhsWork (into yvec)
    HIPCHK(hipMemcpyAsync(h->fin->rhsWork, d.rhs, (size_t)d.nT * TS * sizeof(double), hipMemcpyDeviceToDevice, h->str.st));
  if (pcgMode(h)) {
    if (int rc = precondInit(h)) return rc;
  } else if (int rc = factorReduced(h)) {
    return rc;
  }
  HIPCHK(hipEventRecord(h->str.ev[4], h->str.st));
  if (!fused)
    HIPCHK(hipMemcpyAsync(h->fin->rhsWork, d.rhs, (size_t)d.nT * TS * sizeof(double), hipMemcpyDeviceToDevice, h->str.st));
  if (pcgMode(h)) {
    if (int rc = pcgSolve(h)) return rc;
  } else if (int rc = solveReduced(h, 0, fused ? 2 : 3)) {
    return rc;
  }
  backSubstitute(h, 0);
  HIPCHK(hipEventRecord(h->str.ev[5], h->str.st));
  return 0;
}

int vb_damp_factor_solve(vb_handle h, double lambda, double* model_cost_reduction) {
  if (!h || !h->run.linearized) return fail(VB_E_STATE, "vb_damp_factor_solve needs a fresh vb_linearize");
  if (int rc = dampFactorSolveEnqueue(h, lambda, true)) return rc;
  double dotv = 0;
  if (int rc = readRed(h, &dotv, 16, 1)) return rc;
  if (int rc = checkErr(h)) return rc;
  h->run.times.schur_ms = elapsed(h->str.ev[2], h->str.ev[3]);
  h->run.times.factor_ms = elapsed(h->str.ev[3], h->str.ev[4]);
  h->run.times.solve_ms = elapsed(h->str.ev[4], h->str.ev[5]);
  if (model_cost_reduction) *model_cost_reduction = 0.5 * dotv;
  h->run.linearized = false, h->run.factored = true, h->run.haveStep = true;
  return 0;
}

int vb_gradient_dot_step(vb_handle h, int dont_retry_failed, double* back_red) {
  if (!h || !h->run.factored) return fail(VB_E_STATE, "vb_gradient_dot_step needs a factorization");
  Dev& d = h->fin->d;
  HIPCHK(hipMemsetAsync(d.err, 0, sizeof(int32_t), h->str.st));
  HIPCHK(hipMemsetAsync(d.gRedNew, 0, (size_t)d.nT * TS * sizeof(double), h->str.st));
  HIPCHK(hipMemsetAsync(d.red, 0, 1 * sizeof(double), h->str.st));
  forkSmall(h, 1, d.gRedNew);
  visualLinShard(h, h->fin->d, 0, dont_retry_failed);
  joinSmall(h);
  launch_landmark(d, 0.0, 1, h->str.st);
  launch_reduced_grad(d, 0, h->str.st);
  HIPCHK(hipMemsetAsync(d.red + 16, 0, 8 * sizeof(double), h->str.st));
  launch_dot(d.gRedNew, d.stepRed, d.nRed, d.red + 16, h->str.st);
  launch_dot(d.gpNew + d.lmB * 3, d.stepPt + d.lmB * 3, (d.lmE - d.lmB) * 3, d.red + 16, h->str.st);
  double dotv = 0;
  if (int rc = readRed(h, &dotv, 16, 1)) return rc;
  if (int rc = checkErr(h)) return rc;
  if (back_red) *back_red = -0.5 * dotv;
  return 0;
}

int vb_solve_with_new_gradient(vb_handle h) {
  if (!h || !h->run.factored) return fail(VB_E_STATE, "vb_solve_with_new_gradient needs a factorization");
  Dev& d = h->fin->d;
  launch_landmark(d, 0.0, 2, h->str.st);
  launch_reduced_grad(d, 1, h->str.st);
  HIPCHK(hipMemcpyAsync(h->fin->rhsWork, d.rhs, (size_t)d.nT * TS * sizeof(double), hipMemcpyDeviceToDevice, h->str.st));
  if (pcgMode(h)) {
    if (int rc = pcgSolve(h)) return rc;
  } else if (int rc = solveReduced(h)) {
    return rc;
  }
  backSubstitute(h, 1);
  HIPCHK(hipStreamSynchronize(h->str.st));
  if (int rc = checkErr(h)) return rc;
  h->run.haveSub = true;
  return 0;
}

int vb_set_solver(vb_handle h, int solver_type, int pcg_max_iterations, double pcg_desired_residual) {
  if (!h) return fail(VB_E_ARG, "null handle");
  if (solver_type < VB_SOLVER_DIRECT || solver_type > VB_SOLVER_PCG_LOWER_PREC) return fail(VB_E_ARG, "unknown solver type");
  if (solver_type != VB_SOLVER_DIRECT && (h->prob.partSet || h->prob.sharded))
    return fail(VB_E_UNSUPPORTED, "the PCG solvers run on a single handle (no landmark shards, no partition)");
  if (pcg_max_iterations < 1) return fail(VB_E_ARG, "pcg_max_iterations must be >= 1");
  h->tune.solverType = solver_type, h->tune.pcgMaxIt = pcg_max_iterations, h->tune.pcgTol = pcg_desired_residual;
  return 0;
}
int vb_reduced_layout(vb_handle h, int32_t* kinds, int32_t* handles, int64_t* offsets, int64_t* n, int64_t* padded_order) {
  if (!h || !h->fin) return fail(VB_E_STATE, "vb_reduced_layout before vb_finalize");
  const int64_t nRV = (int64_t)h->fin->lay.rvKind.size();
  if (n) *n = nRV;
  if (padded_order) *padded_order = (int64_t)h->fin->d.nT * TS;
  for (int64_t i = 0; i < nRV; i++) {
    if (kinds) kinds[i] = h->fin->lay.rvKind[i];
    if (handles) handles[i] = h->fin->lay.rvHandle[i];
    if (offsets) offsets[i] = h->fin->lay.rvOff[i];
  }
  return 0;
}
int vb_debug_negate_model_reduction(vb_handle h, int iteration) {
  if (!h) return fail(VB_E_ARG, "null handle");
  h->run.faultNegModelRedIt = iteration;
  return 0;
}
int vb_debug_fail_iteration(vb_handle h, int iteration) {
  if (!h) return fail(VB_E_ARG, "null handle");
  h->run.faultFailIt = iteration;
  return 0;
}
// slot of tile (I, J) of the reduced tile store (vb_reduced_buffers), -1 when it is not stored
int vb_debug_live_resources(int64_t out[3]) {
  if (!out) return fail(VB_E_ARG, "vb_debug_live_resources: null argument");
  for (int i = 0; i < 3; i++) out[i] = g_live[i].load();
  return 0;
}
int vb_debug_tile_slot(vb_handle h, int32_t I, int32_t J, int64_t* slot) {
  if (!h || !h->fin || !slot) return fail(VB_E_STATE, "vb_debug_tile_slot before vb_finalize");
  *slot = -1;
  if (I < J || J < 0 || I >= h->fin->d.nT) return 0;
  for (int64_t c = h->fin->colStart[J]; c < h->fin->colStart[J + 1]; c++)
    if (h->fin->colRowsH[c] == I) *slot = h->fin->colTilesH[c];
  return 0;
}
int vb_pcg_stats(vb_handle h, int32_t* iterations, double* relative_residual) {
  if (!h) return fail(VB_E_ARG, "null handle");
  if (iterations) *iterations = h->run.pcgIters;
  if (relative_residual) *relative_residual = h->run.pcgRelRes;
  return 0;
}

int vb_scale_step(vb_handle h, double f) {
  if (!h || !h->fin) return fail(VB_E_STATE, "not finalized");
  launch_axpby(h->fin->d.stepRed, h->fin->d.stepRed, 0.0, f, h->fin->d.nRed, h->str.st);
  launch_axpby(h->fin->d.stepPt, h->fin->d.stepPt, 0.0, f, h->fin->d.nPts * 3, h->str.st);
  return 0;
}

// box-plus of the step (red[8..10]: the raw step ratios), bracketed by events e0 / e1
int applyStepEnqueue(vb_handle h, int which, int e0, int e1) {
  Dev& d = h->fin->d;
  HIPCHK(hipEventRecord(h->str.ev[e0], h->str.st));
  HIPCHK(hipMemsetAsync(d.red + 8, 0, 3 * sizeof(double), h->str.st));
  launch_boxplus(d, which ? d.subRed : d.stepRed, which ? d.subPt : d.stepPt, h->str.st);
  HIPCHK(hipEventRecord(h->str.ev[e1], h->str.st));
  return 0;
}
int vb_apply_step_raw(vb_handle h, int which, double raw[3]) {
  if (!h || !h->fin) return fail(VB_E_STATE, "not finalized");
  if (int rc = applyStepEnqueue(h, which, 10, 11)) return rc;
  if (h->run.deferred) {  // raw ratios in red[8..10]
    if (raw) raw[0] = raw[1] = raw[2] = std::nan("");
    return 0;
  }
  double r[3];
  if (int rc = readRed(h, r, 8, 3)) return rc;
  h->run.times.step_ms = elapsed(h->str.ev[10], h->str.ev[11]);
  if (raw) raw[0] = r[0], raw[1] = r[1], raw[2] = r[2];
  return 0;
}
int vb_apply_step(vb_handle h, int which, double ratios[3]) {
  double r[3];
  if (int rc = vb_apply_step_raw(h, which, r)) return rc;
  const double n = (double)std::max<int64_t>(1, h->fin->nParams);
  if (ratios) ratios[0] = r[0], ratios[1] = std::sqrt(r[1] / n), ratios[2] = r[2] / n;
  return 0;
}
int64_t vb_num_params(vb_handle h) { return !h ? -1 : h->fin ? h->fin->nParams : 0; }

// the cost pass (red[1..4]: cost and CostStats), bracketed by ev[6] / ev[7]
int costEnqueue(vb_handle h, int comparable, bool clearErr) {
  Dev& d = h->fin->d;
  HIPCHK(hipEventRecord(h->str.ev[6], h->str.st));
  HIPCHK(hipMemsetAsync(d.red + 1, 0, 4 * sizeof(double), h->str.st));
  if (clearErr) HIPCHK(hipMemsetAsync(d.err, 0, sizeof(int32_t), h->str.st));
  forkSmall(h, 2, nullptr);
  visualCostShard(h, comparable);
  joinSmall(h);
  HIPCHK(hipEventRecord(h->str.ev[7], h->str.st));
  return 0;
}
// vb_optimize's cost pass with the global-shutter observations folded into the speculative
// linearization queued next (specEnqueue with fuseCost: visual_lin_kernel<true>, then the fold and
// ev[7] / evCost): here only the small factors and the rolling-shutter observations, evaluated with the
// iteration's tables while the rebuild for the next one runs on stF
int costFusedEnqueue(vb_handle h) {
  Dev& d = h->fin->d;
  HIPCHK(hipEventRecord(h->str.ev[6], h->str.st));
  HIPCHK(hipMemsetAsync(d.red + 1, 0, 4 * sizeof(double), h->str.st));
  forkSmall(h, 2, nullptr);
  profBegin(h, KF_VISUAL_COST);
  launch_visual_cost(d, 1, h->fin->costRsB[0], d.obE, h->str.st);
  launch_visual_cost(d, 1, h->fin->costRsB[1], d.fE, h->str.st);
  profEnd(h, KF_VISUAL_COST);
  joinSmall(h);
  return 0;
}
void costStats(vb_handle h, const double* r, double* cost, vb_cost_stats* stats) {
  int64_t nSmall = 0;
  if (h->fin->shard.isRoot)
    for (int k = 1; k < 14; k++) nSmall += h->fin->d.sf[k].n;
  if (cost) *cost = r[0];
  if (stats) stats->num_total = (int64_t)std::llround(r[1]) + nSmall, stats->num_invalid = std::llround(r[2]),
             stats->num_prev_invalid = std::llround(r[3]);
}
int vb_cost(vb_handle h, int comparable, double* cost, vb_cost_stats* stats) {
  if (!h || !h->fin) return fail(VB_E_STATE, "not finalized");
  if (int rc = costEnqueue(h, comparable, !h->run.deferred)) return rc;
  if (h->run.deferred) {  // cost and CostStats in red[1..4] (vb_small_factor_count: the root's addition)
    if (cost) *cost = std::nan("");
    return 0;
  }
  double r[4];
  if (int rc = readRed(h, r, 1, 4)) return rc;
  if (int rc = checkErr(h)) return rc;
  h->run.times.cost_ms = elapsed(h->str.ev[6], h->str.ev[7]);
  costStats(h, r, cost, stats);
  return 0;
}

static int copyVars(vb_handle h, bool backup) {
  if (!h || !h->fin) return fail(VB_E_STATE, "not finalized");
  int64_t len[9];
  for (int k = 0; k < 9; k++) len[k] = (int64_t)h->prob.data[k].size();
  launch_copy_vars(h->fin->d, backup, len, h->str.st);
  return 0;
}
int vb_backup(vb_handle h) { return copyVars(h, true); }
int vb_restore(vb_handle h) { return copyVars(h, false); }

int vb_get_vars(vb_handle h, int kind, double* out) {
  if (!h || kind < 0 || kind >= 9 || !out) return fail(VB_E_ARG, "bad vb_get_vars arguments");
  if (!h->fin) {
    std::copy(h->prob.data[kind].begin(), h->prob.data[kind].end(), out);
    return 0;
  }
  HIPCHK(hipMemcpyAsync(out, h->fin->d.var[kind], h->prob.data[kind].size() * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  return 0;
}

static int getPerKind(vb_handle h, const double* red, const double* pt, int kind, double* out) {
  Dev& d = h->fin->d;
  const int64_t n = d.nvar[kind];
  const int md = kMaxTan[kind];
  std::fill(out, out + n * md, 0.0);
  if (kind == 0) {
    std::vector<double> v(d.nPts * 3);
    if (!v.empty()) HIPCHK(hipMemcpyAsync(v.data(), pt, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
    HIPCHK(hipStreamSynchronize(h->str.st));
    for (int64_t p = 0; p < n; p++) {
      const int l = h->fin->lmOfPoint[p];
      if (l >= 0) std::copy(&v[l * 3], &v[l * 3] + 3, out + p * 3);
    }
    return 0;
  }
  std::vector<double> v(d.nRed);
  if (!v.empty()) HIPCHK(hipMemcpyAsync(v.data(), red, v.size() * sizeof(double), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  const Layout& L = h->fin->lay;
  for (int i = 0; i < d.nRV; i++)
    if (L.rvKind[i] == kind) std::copy(&v[L.rvOff[i]], &v[L.rvOff[i]] + L.rvDim[i], out + (int64_t)L.rvHandle[i] * md);
  return 0;
}

int vb_get_step(vb_handle h, int which, int kind, double* out) {
  if (!h || !h->fin || kind < 0 || kind >= 9 || !out) return fail(VB_E_ARG, "bad vb_get_step arguments");
  return getPerKind(h, which ? h->fin->d.subRed : h->fin->d.stepRed, which ? h->fin->d.subPt : h->fin->d.stepPt, kind, out);
}
// The visual part of the gradient is assembled inside the Schur pass (vb_damp_factor_solve); before
// that, assemble it on demand into the gradient-only buffers (same kernels as gradient_dot_step).
int vb_get_gradient(vb_handle h, int kind, double* out) {
  if (!h || !h->fin || kind < 0 || kind >= 9 || !out) return fail(VB_E_ARG, "bad vb_get_gradient arguments");
  if (h->run.linearized) {
    Dev& d = h->fin->d;
    HIPCHK(hipMemsetAsync(d.gRedNew, 0, (size_t)d.nT * TS * sizeof(double), h->str.st));
    if (smallHere(h, 1)) launch_small(d, 1, d.gRedNew, h->str.st);
    launch_landmark(d, 0.0, 1, h->str.st);
    launch_reduced_grad(d, 0, h->str.st);
    return getPerKind(h, d.gRedNew, d.gpNew, kind, out);
  }
  return getPerKind(h, h->fin->d.gRed, h->fin->d.gp, kind, out);
}

int vb_last_phase_times(vb_handle h, vb_phase_times* out) {
  if (!h || !out) return fail(VB_E_ARG, "null argument");
  *out = h->run.times;
  return 0;
}

void* vb_stream(vb_handle h) { return h ? (void*)h->str.st : nullptr; }

int vb_profile_kernel(vb_handle h, int family) {
  if (!h || family < -1 || family >= KF_COUNT) return fail(VB_E_ARG, "bad kernel family");
  profHarvest(h);
  h->prof.family = family, h->prof.launches = 0, h->prof.ms = 0.0, h->prof.busyMs = 0.0, h->prof.used = 0, h->prof.done = 0;
  return 0;
}
int vb_kernel_time(vb_handle h, int64_t* launches, double* total_ms) {
  if (!h) return fail(VB_E_ARG, "null handle");
  profHarvest(h);
  if (launches) *launches = h->prof.launches;
  if (total_ms) *total_ms = h->prof.ms;
  return 0;
}
int vb_kernel_busy_time(vb_handle h, double* busy_ms) {
  if (!h || !busy_ms) return fail(VB_E_ARG, "null argument");
  profHarvest(h);
  *busy_ms = h->prof.busyMs;
  return 0;
}
int vb_problem_stats(vb_handle h, int64_t* out) {  // 12 entries
  if (!h || !h->fin || !out) return fail(VB_E_STATE, "not finalized");
  const Dev& d = h->fin->d;
  out[0] = d.nObs, out[1] = d.nPts, out[2] = d.nRV, out[3] = d.nRed, out[4] = d.nT, out[5] = d.nTiles;
  out[6] = h->fin->nPairs;
  int64_t sm = 0;
  for (int k = 1; k < 14; k++) sm += d.sf[k].n;
  out[7] = sm;
  // Schur work-list sizes: landmark-pair entries, observation-pair entries
  out[8] = h->fin->nTileEnt, out[9] = d.nGroups;
  // levels of the tile Cholesky (fan-in launches per factorization); tiles of S itself (the stored
  // tiles less the symbolic fill: what the PCG product reads)
  int64_t nS = 0;
  for (uint8_t f : h->fin->tileFill) nS += f ? 0 : 1;
  out[10] = h->fin->nLevels, out[11] = nS;
  return 0;
}

// the factorization's schedule as it runs: [levels, fan-in contributions per factorization, supernodes,
// two-column supernodes] (the column schedule: supernodes = columns, no two-column ones)
int vb_factor_schedule_stats(vb_handle h, int64_t* out4) {
  if (!h || !h->fin || !out4) return fail(VB_E_STATE, "not finalized");
  if (h->fin->sn[0].built) {
    const SnSched& N = h->fin->sn[0];
    out4[0] = N.nLevels, out4[1] = N.nPairs, out4[2] = N.nSuper, out4[3] = N.nTwo;
  } else {
    out4[0] = h->fin->nLevels, out4[1] = h->fin->nPairs, out4[2] = h->fin->d.nT, out4[3] = 0;
  }
  return 0;
}

int vb_reduced_buffers(vb_handle h, double** matrix, int64_t* matrix_len, double** rhs, int64_t* rhs_len) {
  if (!h || !h->fin) return fail(VB_E_STATE, "not finalized");
  if (matrix) *matrix = h->fin->d.tiles;
  if (matrix_len) *matrix_len = h->fin->d.nTiles * TS * TS;
  if (rhs) *rhs = h->fin->d.rhs;
  if (rhs_len) *rhs_len = (int64_t)h->fin->d.nT * TS;
  return 0;
}

}  // extern "C"

