// Residual report on the device (gfx950): vb_factor_errors / vb_error_histogram, the numbers behind
// Histograms::show (viba/problem/Histograms.cpp) and the rawError / unweightedError logs of the add*
// methods, from the factors the handle holds.  Per factor i of a store (lib/small_thing/Factor.h:172-232):
//   rawError(i)               the functor's return, nothing when the factor fails (visual kinds only)
//   unweightedSquaredError    0.5 |e|^2
//   covWeightedSquaredError   0.5 e^T P e (P: inverse rvpCov of the inertial kinds, H of the pose prior;
//                             every other functor whitens its own return: equal to the unweighted one)
//   singleCost                computeSingleCost(i, false) = 0.5 rho(e^T P e); stored cache untouched
// The factor evaluations are those of the LM loop (factor_eval.hpp: vis_obs_eval as the cost pass calls it; small.hip:
// small_eval's evaluate-only instantiation); here the generic binning kernel of the small kinds and the
// C-ABI.  The report reads the variables and rolling-shutter tables and writes only buffers of its own:
// the cost cache, the red[] / error-word slots, the step and the speculative buffers stay as they are.
#include "host.hpp"
#include "report.hpp"

namespace viba {
namespace {

// values of n evaluated factors (small kinds: a few thousand) binned as H asks: which 0 / 1 from the
// squared norms, 2..4 the rotation [deg] / velocity [cm/s] / position [cm] part of an inertial raw row
// (Histograms.cpp:373-384)
__global__ void __launch_bounds__(256) bin_values_kernel(int64_t n, int m, const double* raw, const double* squ,
                                                         const double* sqw, const double* cost, RepHist H) {
  __shared__ RepTable tab;
  rep_clear(tab, H);
  for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < n; t += (int64_t)gridDim.x * 256) {
    double value;
    if (H.which == VB_ERR_UNWEIGHTED) {
      value = sqrt(2.0 * squ[t]);
    } else if (H.which == VB_ERR_WEIGHTED) {
      value = sqrt(2.0 * sqw[t]);
    } else {
      const double* r = raw + t * m + 3 * (H.which - VB_ERR_ROT_DEG);
      const double nrm = sqrt(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
      value = H.which == VB_ERR_ROT_DEG ? nrm * (180.0 / 3.14159265358979323846) : nrm * 100.0;
    }
    rep_add(tab, H, H.grp ? H.grp[t] : 0, true, value, cost[t]);
  }
  rep_flush(tab, H);
}

}  // namespace
}  // namespace viba

namespace viba_host {
namespace {

constexpr int kErrSize[14] = {2, 9, 9, 9, 3, 23, 17, 6, 6, 6, 23, 17, 6, 6};
static_assert(VB_REPORT_MAX_GROUPS == kRepMaxGroups && VB_REPORT_MAX_EDGES == kRepMaxEdges, "caps of the LDS bin table");

}  // namespace

// (shared with the non-linearity inspection, inspect.hip)
int reportCommon(vb_handle h, const char* what) {
  if (!h) return fail(VB_E_ARG, std::string(what) + ": null handle");
  if (!h->fin) return fail(VB_E_STATE, std::string(what) + " before vb_finalize");
  if (!wholeProblem(h))
    return fail(VB_E_UNSUPPORTED, std::string(what) + " needs the whole problem on this handle (no shard / partition)");
  HIPCHK(hipSetDevice(h->cfg.device));
  if (!h->rep) {
    std::vector<int32_t> pos(h->fin->visRowOfPos.size());
    for (size_t i = 0; i < pos.size(); i++) pos[h->fin->visRowOfPos[i]] = (int32_t)i;
    auto r = std::make_unique<ReportState>();
    if (r->mem.put(&r->posOfRow, pos) || r->mem.zeroed(&r->err, 2) || r->mem.event(&r->ev[0]) || r->mem.event(&r->ev[1]))
      return fail(VB_E_HIP, std::string(what) + ": could not allocate the report's device state");  // (r goes)
    h->rep = std::move(r);
  }
  return 0;
}

int checkReportErr(vb_handle h) {
  int32_t e = 0;
  HIPCHK(hipMemcpyAsync(&e, h->rep->err, sizeof(int32_t), hipMemcpyDeviceToHost, h->str.st));
  HIPCHK(hipStreamSynchronize(h->str.st));
  if (e & 1) return fail(VB_E_RANGE, "RollingShutterData::getEstimate: out of range (residual report)");
  return 0;
}

}  // namespace viba_host

extern "C" {

int vb_factor_error_size(int kind) { return kind >= 0 && kind < 14 ? kErrSize[kind] : VB_E_ARG; }

int vb_factor_errors(vb_handle h, int kind, int64_t first, int64_t n, double* raw, double* sq_unweighted,
                     double* sq_weighted, double* cost, uint8_t* valid) {
  if (int rc = reportCommon(h, "vb_factor_errors")) return rc;
  if (kind < 0 || kind >= 14) return fail(VB_E_ARG, "vb_factor_errors: bad factor kind");
  const int64_t N = (int64_t)h->prob.fint[kind].size();
  if (first < 0 || n < 0 || first > N || n > N - first) return fail(VB_E_ARG, "vb_factor_errors: rows out of range");
  if (n == 0) return 0;
  const int m = kErrSize[kind];
  DevOwner S;  // frees its buffers when the call returns, on every path
  RepRows R;
  R.first = first, R.n = n;
  if ((raw && S.get(&R.raw, (size_t)n * m)) || (sq_unweighted && S.get(&R.squ, n)) ||
      (sq_weighted && S.get(&R.sqw, n)) || (cost && S.get(&R.cost, n)) ||
      (valid && kind == VB_F_VISUAL && S.get(&R.valid, n)))
    return devFail(S, "vb_factor_errors: device allocation");
  HIPCHK(hipMemsetAsync(h->rep->err, 0, sizeof(int32_t), h->str.st));
  if (kind == VB_F_VISUAL) launch_visual_rows(h->fin->d, h->rep->posOfRow, R, h->rep->err, h->str.st);
  else launch_small_rows(h->fin->d, kind, R, h->str.st);
  HIPCHK(hipGetLastError());
  if (download(raw, R.raw, (size_t)n * m, h->str.st) || download(sq_unweighted, R.squ, n, h->str.st) ||
      download(sq_weighted, R.sqw, n, h->str.st) || download(cost, R.cost, n, h->str.st))
    return VB_E_HIP;
  if (valid && kind == VB_F_VISUAL && download(valid, R.valid, n, h->str.st)) return VB_E_HIP;
  if (valid && kind != VB_F_VISUAL) std::fill(valid, valid + n, (uint8_t)1);  // only visual factors can fail
  return checkReportErr(h);
}

int vb_error_histogram(vb_handle h, int kind, int which, int32_t n_groups, const int32_t* group_of_factor,
                       int32_t n_edges, const double* edges, int64_t* counts, double* cost, int64_t* n_factors,
                       int64_t* n_failing) {
  if (int rc = reportCommon(h, "vb_error_histogram")) return rc;
  if (kind < 0 || kind >= 14) return fail(VB_E_ARG, "vb_error_histogram: bad factor kind");
  if (which < VB_ERR_UNWEIGHTED || which > VB_ERR_POS_CM) return fail(VB_E_ARG, "vb_error_histogram: bad error selector");
  if (which >= VB_ERR_ROT_DEG && !(kind >= VB_F_IMU && kind <= VB_F_IMU_SEC_SPLIT))
    return fail(VB_E_ARG, "vb_error_histogram: rotation / velocity / position errors exist for the inertial kinds only");
  if (n_groups < 1 || n_groups > VB_REPORT_MAX_GROUPS || n_edges < 1 || n_edges > VB_REPORT_MAX_EDGES || !edges)
    return fail(VB_E_ARG, "vb_error_histogram: n_groups must be in [1, 64] and n_edges in [1, 32]");
  for (int32_t e = 0; e < n_edges; e++)
    if (!std::isfinite(edges[e]) || (e > 0 && !(edges[e] > edges[e - 1])))
      return fail(VB_E_ARG, "vb_error_histogram: edges must be finite and strictly increasing");
  const Dev& d = h->fin->d;
  const int64_t N = (int64_t)h->prob.fint[kind].size();
  const bool visual = kind == VB_F_VISUAL;
  // the group of every item in the kernel's item order: obCostOrder positions (visual), rows (the rest)
  std::vector<uint8_t> grp;
  if (group_of_factor) {
    grp.resize(N);
    for (int64_t i = 0; i < N; i++) {
      const int32_t g = group_of_factor[visual ? h->fin->visRowOfPos[i] : i];
      if (g < 0 || g >= n_groups) return fail(VB_E_ARG, "vb_error_histogram: group id outside [0, n_groups)");
      grp[i] = (uint8_t)g;
    }
  }
  const size_t nb = (size_t)n_groups * (n_edges + 1);
  DevOwner S;  // frees its buffers when the call returns, on every path
  RepHist H;
  H.which = which, H.nGroups = n_groups, H.nEdges = n_edges;
  uint8_t* grpD = nullptr;
  double* edgesD = nullptr;
  if (S.get(&edgesD, n_edges) || S.get(&H.counts, nb) || S.get(&H.cost, n_groups) || S.get(&H.nFactors, n_groups) ||
      S.get(&H.nFailing, n_groups) || (group_of_factor && S.get(&grpD, N)))
    return devFail(S, "vb_error_histogram: device allocation");
  H.edges = edgesD, H.grp = grpD;
  hipStream_t st = h->str.st;
  HIPCHK(hipMemcpyAsync(edgesD, edges, n_edges * sizeof(double), hipMemcpyHostToDevice, st));
  if (grpD && N) HIPCHK(hipMemcpyAsync(grpD, grp.data(), N, hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(H.counts, 0, nb * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(H.cost, 0, n_groups * sizeof(double), st));
  HIPCHK(hipMemsetAsync(H.nFactors, 0, n_groups * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(H.nFailing, 0, n_groups * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(h->rep->err, 0, sizeof(int32_t), st));
  HIPCHK(hipEventRecord(h->rep->ev[0], st));
  if (visual) {
    // a few workgroups per CU walk the positions: the table's flush is paid once per workgroup
    launch_visual_hist(d, H, h->rep->err, h->tune.numCUs * 8, st);
  } else if (N > 0) {
    const int m = kErrSize[kind];
    RepRows R;
    R.first = 0, R.n = N;
    if (S.get(&R.raw, (size_t)N * m) || S.get(&R.squ, N) || S.get(&R.sqw, N) || S.get(&R.cost, N))
      return devFail(S, "vb_error_histogram: device allocation");
    launch_small_rows(d, kind, R, st);
    hipLaunchKernelGGL(bin_values_kernel, dim3((unsigned)std::min<int64_t>((N + 255) / 256, 64)), dim3(256), 0, st, N, m,
                       R.raw, R.squ, R.sqw, R.cost, H);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(h->rep->ev[1], st));
  std::vector<unsigned long long> cnt(nb), nf(n_groups), nx(n_groups);
  if (download(cnt.data(), H.counts, nb, st) || download(nf.data(), H.nFactors, n_groups, st) ||
      download(nx.data(), H.nFailing, n_groups, st) || download(cost, H.cost, n_groups, st))
    return VB_E_HIP;
  if (int rc = checkReportErr(h)) return rc;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, h->rep->ev[0], h->rep->ev[1]));
  h->rep->histMs = ms;
  if (counts) std::copy(cnt.begin(), cnt.end(), counts);
  if (n_factors) std::copy(nf.begin(), nf.end(), n_factors);
  if (n_failing) std::copy(nx.begin(), nx.end(), n_failing);
  return 0;
}

// the base-map factors' report (Histograms.cpp:72, 257-306), under vb_factor_errors' rules
int vb_basemap_errors(vb_handle h, int64_t first, int64_t n, double* raw, double* sq_unweighted, double* cost,
                      uint8_t* valid) {
  if (int rc = reportCommon(h, "vb_basemap_errors")) return rc;
  const int64_t N = h->fin->d.bm.n;
  if (first < 0 || n < 0 || first > N || n > N - first) return fail(VB_E_ARG, "vb_basemap_errors: rows out of range");
  if (n == 0) return 0;
  DevOwner S;  // frees its buffers when the call returns, on every path
  RepRows R;
  R.first = first, R.n = n;
  if ((raw && S.get(&R.raw, (size_t)n * 2)) || (sq_unweighted && S.get(&R.squ, n)) || (cost && S.get(&R.cost, n)) ||
      (valid && S.get(&R.valid, n)))
    return devFail(S, "vb_basemap_errors: device allocation");
  launch_basemap_rows(h->fin->d, R, h->str.st);
  HIPCHK(hipGetLastError());
  if (download(raw, R.raw, (size_t)n * 2, h->str.st) || download(sq_unweighted, R.squ, n, h->str.st) ||
      download(cost, R.cost, n, h->str.st) || download(valid, R.valid, n, h->str.st))
    return VB_E_HIP;
  HIPCHK(hipStreamSynchronize(h->str.st));
  return 0;
}

int vb_basemap_histogram(vb_handle h, int which, int32_t n_edges, const double* edges, int64_t* counts, double* cost,
                         int64_t* n_factors, int64_t* n_failing) {
  if (int rc = reportCommon(h, "vb_basemap_histogram")) return rc;
  if (which != VB_ERR_UNWEIGHTED && which != VB_ERR_WEIGHTED) return fail(VB_E_ARG, "vb_basemap_histogram: bad error selector");
  if (n_edges < 1 || n_edges > VB_REPORT_MAX_EDGES || !edges) return fail(VB_E_ARG, "vb_basemap_histogram: n_edges must be in [1, 32]");
  for (int32_t e = 0; e < n_edges; e++)
    if (!std::isfinite(edges[e]) || (e > 0 && !(edges[e] > edges[e - 1])))
      return fail(VB_E_ARG, "vb_basemap_histogram: edges must be finite and strictly increasing");
  const size_t nb = (size_t)n_edges + 1;
  DevOwner S;
  RepHist H;
  H.which = which, H.nGroups = 1, H.nEdges = n_edges;
  double* edgesD = nullptr;
  if (S.get(&edgesD, n_edges) || S.get(&H.counts, nb) || S.get(&H.cost, 1) || S.get(&H.nFactors, 1) || S.get(&H.nFailing, 1))
    return devFail(S, "vb_basemap_histogram: device allocation");
  H.edges = edgesD;
  hipStream_t st = h->str.st;
  HIPCHK(hipMemcpyAsync(edgesD, edges, n_edges * sizeof(double), hipMemcpyHostToDevice, st));
  HIPCHK(hipMemsetAsync(H.counts, 0, nb * sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(H.cost, 0, sizeof(double), st));
  HIPCHK(hipMemsetAsync(H.nFactors, 0, sizeof(unsigned long long), st));
  HIPCHK(hipMemsetAsync(H.nFailing, 0, sizeof(unsigned long long), st));
  launch_basemap_hist(h->fin->d, H, h->tune.numCUs * 8, st);
  HIPCHK(hipGetLastError());
  std::vector<unsigned long long> cnt(nb);
  unsigned long long nf = 0, nx = 0;
  if (download(cnt.data(), H.counts, nb, st) || download(&nf, H.nFactors, 1, st) || download(&nx, H.nFailing, 1, st) ||
      download(cost, H.cost, 1, st))
    return VB_E_HIP;
  HIPCHK(hipStreamSynchronize(st));
  if (counts) std::copy(cnt.begin(), cnt.end(), counts);
  if (n_factors) *n_factors = (int64_t)nf;
  if (n_failing) *n_failing = (int64_t)nx;
  return 0;
}

int vb_report_device_ms(vb_handle h, double* ms) {
  if (!h || !ms) return fail(VB_E_ARG, "vb_report_device_ms: null argument");
  *ms = h->rep ? h->rep->histMs : 0.0;
  return 0;
}

}  // extern "C"
