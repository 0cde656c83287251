// Non-linearity inspection on the device (gfx950): vb_factor_expected_delta / vb_inspect_nonlinearities /
// vb_set_inspect_iteration, the numbers behind Settings::triggerDebuggingOfNonlinearities (Optimizer.cpp:861-883,
// compareExpectedValues :727-766) from the factors the handle holds.  Per factor (Factor.h:470-540):
//   singleExpectedDelta(i, step)  {v0 = 0.5 rho, delta = step . J^T rho' P e, |J^T rho' P e|}; {-1, 0, 0} when
//                                 the factor fails (visual kinds only)
//   singleCost(i)                 at the stepped variables: the residual report's cost (report.hip)
//   score                         |v0 + delta - v1| / (min(|grad|, 1000) + 1)
// The expected-delta kernels are in visual.hip / small.hip beside the evaluators (inspect.hpp); the stepped costs come
// from the residual report's kernels (so v1 is vb_factor_errors' cost bit for bit); here the score / key
// kernel, the exact top-k selection and the C-ABI.
// Items of one inspection: the visual factors by position of obCostOrder (global shutter first, so a wave
// runs one evaluation path), then the small kinds 1..13 by row; base[kind] is a kind's first item.
#include "host.hpp"
#include "inspect.hpp"
#include "report.hpp"

namespace viba {
namespace {

constexpr unsigned long long kNoKey = ~0ull;  // a factor that does not take part (above every score's bits)
constexpr unsigned long long kInfKey = 0x7ff0000000000000ull;

struct InsItems {
  int64_t base[15];  // base[14]: the number of items
  const int32_t* rowOfPos;
};
__device__ __forceinline__ int ins_kind_of(const InsItems& I, int64_t t) {
  int k = 0;
  while (k < 13 && t >= I.base[k + 1]) k++;
  return k;
}

// score and key of every item: the key is the score's bit pattern (the score is non-negative or NaN, NaN
// counted as +inf, so the keys order as unsigned integers); kNoKey for a factor that fails at either point or
// whose kind is masked out
__global__ void __launch_bounds__(256) inspect_key_kernel(InsItems I, uint32_t mask, const double* v0, const double* delta,
                                                          const double* gnorm, const double* v1, const uint8_t* validVis,
                                                          unsigned long long* key) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= I.base[14]) return;
  const int kind = ins_kind_of(I, t);
  const double a = v0[t];
  const bool ok = a >= 0.0 && (kind != 0 || validVis[t]) && ((mask >> kind) & 1u);
  const double s = fabs((a + delta[t]) - v1[t]) / (fmin(gnorm[t], 1000.0) + 1.0);
  unsigned long long kb = s != s ? kInfKey : (unsigned long long)__double_as_longlong(s);
  key[t] = ok ? kb : kNoKey;
}

// the k best (key descending, tie ascending) a workgroup has seen, in LDS, sorted; tie = kind << 56 | row
struct TopK {
  unsigned long long key[VB_INSPECT_MAX_K], tie[VB_INSPECT_MAX_K];
  long long idx[VB_INSPECT_MAX_K];
  unsigned long long ckey[256], ctie[256];
  long long cidx[256];
  int n, nc;
};
__device__ __forceinline__ bool ins_better(unsigned long long ka, unsigned long long ta, unsigned long long kb,
                                           unsigned long long tb) {
  return ka > kb || (ka == kb && ta < tb);
}
// One round of a 256-thread workgroup: every thread offers at most one candidate.  Those that beat the
// table's last entry (or find it not full) are collected (LDS counter: their order varies, the table they
// leave does not, the order is total) and inserted by thread 0; after the first rounds few pass the threshold.
__device__ void topk_round(TopK& T, int k, bool has, unsigned long long key, unsigned long long tie, long long idx) {
  if (threadIdx.x == 0) T.nc = 0;
  __syncthreads();
  if (has && (T.n < k || ins_better(key, tie, T.key[k - 1], T.tie[k - 1]))) {
    const int c = atomicAdd(&T.nc, 1);
    T.ckey[c] = key, T.ctie[c] = tie, T.cidx[c] = idx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int c = 0; c < T.nc; c++) {
      const unsigned long long ck = T.ckey[c], ct = T.ctie[c];
      int p = T.n < k ? T.n : k - 1;  // the slot that opens: a new one, or the last entry's
      if (T.n == k && !ins_better(ck, ct, T.key[k - 1], T.tie[k - 1])) continue;
      while (p > 0 && ins_better(ck, ct, T.key[p - 1], T.tie[p - 1])) {
        T.key[p] = T.key[p - 1], T.tie[p] = T.tie[p - 1], T.idx[p] = T.idx[p - 1];
        p--;
      }
      T.key[p] = ck, T.tie[p] = ct, T.idx[p] = T.cidx[c];
      if (T.n < k) T.n++;
    }
  }
  __syncthreads();
}

// every workgroup walks its share of the items and leaves its k best at part[blockIdx.x * k ..) (key, tie,
// idx; kNoKey-padded); the factors that take part are counted with integer atomics
__global__ void __launch_bounds__(256) inspect_select_kernel(InsItems I, const unsigned long long* key, int k,
                                                             unsigned long long* partKey, unsigned long long* partTie,
                                                             long long* partIdx, unsigned long long* nCompared) {
  __shared__ TopK T;
  __shared__ unsigned int cnt;
  if (threadIdx.x == 0) T.n = 0, cnt = 0;
  __syncthreads();
  const int64_t N = I.base[14];
  unsigned int mine = 0;
  for (int64_t t0 = (int64_t)blockIdx.x * 256; t0 < N; t0 += (int64_t)gridDim.x * 256) {  // (block-uniform trip count)
    const int64_t t = t0 + threadIdx.x;
    unsigned long long kb = kNoKey, tie = 0;
    if (t < N) kb = key[t];
    const bool has = kb != kNoKey;
    if (has) {
      mine++;
      const int kind = ins_kind_of(I, t);
      const int64_t row = kind == 0 ? I.rowOfPos[t] : t - I.base[kind];
      tie = (unsigned long long)kind << 56 | (unsigned long long)row;
    }
    topk_round(T, k, has, kb, tie, t);
  }
  if (mine) atomicAdd(&cnt, mine);
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(nCompared, (unsigned long long)cnt);
  for (int i = threadIdx.x; i < k; i += 256) {
    const bool in = i < T.n;
    partKey[(int64_t)blockIdx.x * k + i] = in ? T.key[i] : kNoKey;
    partTie[(int64_t)blockIdx.x * k + i] = in ? T.tie[i] : 0;
    partIdx[(int64_t)blockIdx.x * k + i] = in ? T.idx[i] : -1;
  }
}

// one workgroup merges the nPart * k partial entries by (key descending, kind, row) and gathers the found
// factors' values: out[0..7) x VB_INSPECT_MAX_K 8-byte words (kind, row as integers; score, v0, delta, v1,
// gnorm), then [n_found, -]
__global__ void __launch_bounds__(256) inspect_merge_kernel(const unsigned long long* partKey, const unsigned long long* partTie,
                                                            const long long* partIdx, int64_t nEnt, int k, const double* v0,
                                                            const double* delta, const double* gnorm, const double* v1,
                                                            long long* out) {
  __shared__ TopK T;
  if (threadIdx.x == 0) T.n = 0;
  __syncthreads();
  for (int64_t t0 = 0; t0 < nEnt; t0 += 256) {
    const int64_t t = t0 + threadIdx.x;
    unsigned long long kb = kNoKey, tie = 0;
    long long idx = -1;
    if (t < nEnt) kb = partKey[t], tie = partTie[t], idx = partIdx[t];
    topk_round(T, k, kb != kNoKey, kb, tie, idx);
  }
  const int i = threadIdx.x;
  if (i < T.n) {
    const long long t = T.idx[i];
    out[0 * VB_INSPECT_MAX_K + i] = (long long)(T.tie[i] >> 56);
    out[1 * VB_INSPECT_MAX_K + i] = (long long)(T.tie[i] & ((1ull << 56) - 1));
    out[2 * VB_INSPECT_MAX_K + i] = (long long)T.key[i];
    out[3 * VB_INSPECT_MAX_K + i] = __double_as_longlong(v0[t]);
    out[4 * VB_INSPECT_MAX_K + i] = __double_as_longlong(delta[t]);
    out[5 * VB_INSPECT_MAX_K + i] = __double_as_longlong(v1[t]);
    out[6 * VB_INSPECT_MAX_K + i] = __double_as_longlong(gnorm[t]);
  }
  if (i == 0) out[7 * VB_INSPECT_MAX_K] = T.n;
}

}  // namespace
}  // namespace viba

namespace viba_host {
namespace {

constexpr int64_t kStageCap = 16384;  // small factors evaluated per launch pair: at most 16384 x 15.1 KB of staging

int inspectCommon(vb_handle h, const char* what, int which) {
  if (int rc = reportCommon(h, what)) return rc;
  if (which != 0 && which != 1) return fail(VB_E_ARG, std::string(what) + ": which must be 0 (step) or 1 (sub-step)");
  if (!h->run.haveStep) return fail(VB_E_STATE, std::string(what) + " needs a step on the device (vb_damp_factor_solve)");
  if (which == 1 && !h->run.haveSub)
    return fail(VB_E_STATE, std::string(what) + ": which = 1 needs a sub-step on the device (vb_solve_with_new_gradient)");
  if (!h->ins) {
    const std::vector<int32_t>& rop = h->fin->visRowOfPos;
    std::vector<int32_t> ident(rop.size());
    std::iota(ident.begin(), ident.end(), 0);
    auto s = std::make_unique<InspectState>();
    bool bad = s->mem.put(&s->rowOfPos, rop) || s->mem.put(&s->posIdent, ident);
    for (hipEvent_t& e : s->ev) bad = bad || s->mem.event(&e);
    if (bad) return fail(VB_E_HIP, std::string(what) + ": could not allocate the inspection's device state");
    h->ins = std::move(s);
  }
  return 0;
}

int allocStage(DevOwner& S, InsStage* st, int64_t cap) {
  st->cap = cap;
  return S.get(&st->sJ, (size_t)cap * kSmallJ) || S.get(&st->sE, (size_t)cap * kSmallE) || S.get(&st->sMeta, (size_t)cap * kSmallMeta);
}

// rows [first, first + n) of small kind fk in launches of at most the staging's capacity
void smallExpected(const Dev& d, int fk, InsRows R, const InsStage& st, hipStream_t s) {
  for (int64_t o = 0; o < R.n; o += st.cap) {
    InsRows C = R;
    C.first = R.first + o, C.n = std::min(st.cap, R.n - o);
    C.v0 = R.v0 + o, C.delta = R.delta + o, C.gnorm = R.gnorm + o;
    launch_small_expected(d, fk, C, st, s);
  }
}

template <typename T>
void copyOut(T* dst, const T* src, int n) {
  if (dst) std::copy(src, src + n, dst);
}
int resultOut(vb_handle h, int32_t* kinds, int64_t* rows, double* score, double* v0, double* delta, double* v1,
              double* grad_norm, int32_t* n_found, int64_t* n_compared) {
  if (n_found) *n_found = 0;
  if (n_compared) *n_compared = 0;
  if (!h->ins) return 0;  // (no inspection yet)
  const InspectState& r = *h->ins;
  const int n = r.nFound;
  copyOut(kinds, r.kinds, n), copyOut(rows, r.rows, n), copyOut(score, r.score, n), copyOut(v0, r.v0, n);
  copyOut(delta, r.delta, n), copyOut(v1, r.v1, n), copyOut(grad_norm, r.gnorm, n);
  if (n_found) *n_found = n;
  if (n_compared) *n_compared = r.nCompared;
  return 0;
}

}  // namespace

int inspectRun(vb_handle h, int which, uint32_t kindMask, int32_t k) {
  const char* what = "vb_inspect_nonlinearities";
  if (int rc = inspectCommon(h, what, which)) return rc;
  if (k < 1 || k > VB_INSPECT_MAX_K) return fail(VB_E_ARG, "vb_inspect_nonlinearities: k must be in [1, VB_INSPECT_MAX_K]");
  if (kindMask == 0 || (kindMask >> 14) != 0) return fail(VB_E_ARG, "vb_inspect_nonlinearities: kind_mask must name kinds 0..13");
  const Dev& d = h->fin->d;
  InspectState& I = *h->ins;
  I.nFound = 0, I.nCompared = 0;
  InsItems it{};
  it.rowOfPos = I.rowOfPos;
  it.base[0] = 0;
  int64_t maxSmall = 0;
  for (int kind = 0; kind < 14; kind++) {
    const int64_t n = (int64_t)h->prob.fint[kind].size();
    it.base[kind + 1] = it.base[kind] + n;
    if (kind > 0) maxSmall = std::max(maxSmall, n);
  }
  const int64_t N = it.base[14], nVis = it.base[1];
  const int nPart = (int)std::max<int64_t>(1, std::min<int64_t>((N + 255) / 256, (int64_t)h->tune.numCUs * 4));
  DevOwner S;  // frees its buffers when the call returns, on every path
  double *v0 = nullptr, *delta = nullptr, *gnorm = nullptr, *v1 = nullptr;
  unsigned long long *key = nullptr, *partKey = nullptr, *partTie = nullptr, *nCmp = nullptr;
  long long *partIdx = nullptr, *out = nullptr;
  uint8_t* valid = nullptr;
  InsStage st;
  const size_t nA = (size_t)std::max<int64_t>(N, 1), nP = (size_t)nPart * k;
  constexpr int kOut = 7 * VB_INSPECT_MAX_K + 2;
  if (S.get(&v0, nA) || S.get(&delta, nA) || S.get(&gnorm, nA) || S.get(&v1, nA) || S.get(&key, nA) ||
      S.get(&valid, (size_t)std::max<int64_t>(nVis, 1)) || S.get(&partKey, nP) || S.get(&partTie, nP) || S.get(&partIdx, nP) ||
      S.get(&nCmp, 1) || S.get(&out, kOut) || allocStage(S, &st, std::max<int64_t>(1, std::min(kStageCap, maxSmall))))
    return devFail(S, "vb_inspect_nonlinearities: device allocation");
  hipStream_t s = h->str.st;
  HIPCHK(hipMemsetAsync(h->rep->err, 0, sizeof(int32_t), s));
  HIPCHK(hipMemsetAsync(nCmp, 0, sizeof(unsigned long long), s));
  HIPCHK(hipMemsetAsync(out, 0, kOut * sizeof(long long), s));
  // x0: the expected values at the current variables
  HIPCHK(hipEventRecord(I.ev[0], s));
  InsRows R;
  R.stepRed = which ? d.subRed : d.stepRed, R.stepPt = which ? d.subPt : d.stepPt;
  R.first = 0, R.n = nVis, R.v0 = v0, R.delta = delta, R.gnorm = gnorm;
  // the small kinds (a chain of few-wave launches, latency-bound) on the side stream beside the visual pass
  hipStream_t s2 = h->str.st2;
  HIPCHK(hipEventRecord(h->str.evFork, s));
  HIPCHK(hipStreamWaitEvent(s2, h->str.evFork, 0));
  launch_visual_expected(d, nullptr, R, h->rep->err, s);
  for (int kind = 1; kind < 14; kind++) {
    R.first = 0, R.n = it.base[kind + 1] - it.base[kind];
    R.v0 = v0 + it.base[kind], R.delta = delta + it.base[kind], R.gnorm = gnorm + it.base[kind];
    smallExpected(d, kind, R, st, s2);
  }
  HIPCHK(hipEventRecord(h->str.evJoin, s2));
  HIPCHK(hipStreamWaitEvent(s, h->str.evJoin, 0));
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(I.ev[1], s));
  if (int rc = checkReportErr(h)) return rc;  // (out of range at the linearization point: no step taken)
  // backupVariables, applyStep(which)
  if (int rc = vb_backup(h)) return rc;
  if (int rc = applyStepEnqueue(h, which, 10, 11)) return rc;
  // x1: singleCost at the stepped variables (the residual report's kernels), score and key
  HIPCHK(hipEventRecord(I.ev[2], s));
  RepRows C;
  C.first = 0, C.n = nVis, C.cost = v1, C.valid = valid;
  HIPCHK(hipEventRecord(h->str.evFork, s));
  HIPCHK(hipStreamWaitEvent(s2, h->str.evFork, 0));
  launch_visual_rows(d, I.posIdent, C, h->rep->err, s);  // (the identity map: items in position order)
  for (int kind = 1; kind < 14; kind++) {
    RepRows Q;
    Q.first = 0, Q.n = it.base[kind + 1] - it.base[kind], Q.cost = v1 + it.base[kind];
    launch_small_rows(d, kind, Q, s2);
  }
  HIPCHK(hipEventRecord(h->str.evJoin, s2));
  HIPCHK(hipStreamWaitEvent(s, h->str.evJoin, 0));
  if (N > 0)
    hipLaunchKernelGGL(inspect_key_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, it, kindMask, v0, delta, gnorm,
                       v1, valid, key);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(I.ev[3], s));
  // the k worst
  hipLaunchKernelGGL(inspect_select_kernel, dim3((unsigned)nPart), dim3(256), 0, s, it, key, (int)k, partKey, partTie, partIdx,
                     nCmp);
  hipLaunchKernelGGL(inspect_merge_kernel, dim3(1), dim3(256), 0, s, partKey, partTie, partIdx, (int64_t)nP, (int)k, v0, delta,
                     gnorm, v1, out);
  HIPCHK(hipGetLastError());
  HIPCHK(hipEventRecord(I.ev[4], s));
  long long res[kOut];
  unsigned long long nc = 0;
  if (download(res, out, (size_t)kOut, s) || download(&nc, nCmp, (size_t)1, s)) return VB_E_HIP;
  if (int rc = checkReportErr(h)) return rc;
  float ms[3] = {0.f, 0.f, 0.f};
  HIPCHK(hipEventElapsedTime(&ms[0], I.ev[0], I.ev[1]));
  HIPCHK(hipEventElapsedTime(&ms[1], I.ev[2], I.ev[3]));
  HIPCHK(hipEventElapsedTime(&ms[2], I.ev[3], I.ev[4]));
  for (int i = 0; i < 3; i++) I.ms[i] = ms[i];
  const int n = (int)res[7 * VB_INSPECT_MAX_K];
  auto asDouble = [](long long b) {
    double x;
    std::memcpy(&x, &b, sizeof(x));
    return x;
  };
  for (int i = 0; i < n; i++) {
    I.kinds[i] = (int32_t)res[i], I.rows[i] = res[VB_INSPECT_MAX_K + i];
    I.score[i] = asDouble(res[2 * VB_INSPECT_MAX_K + i]), I.v0[i] = asDouble(res[3 * VB_INSPECT_MAX_K + i]);
    I.delta[i] = asDouble(res[4 * VB_INSPECT_MAX_K + i]), I.v1[i] = asDouble(res[5 * VB_INSPECT_MAX_K + i]);
    I.gnorm[i] = asDouble(res[6 * VB_INSPECT_MAX_K + i]);
  }
  I.nFound = n, I.nCompared = (int64_t)nc;
  return 0;
}

}  // namespace viba_host

extern "C" {

int vb_factor_expected_delta(vb_handle h, int kind, int64_t first, int64_t n, int which, double* v0, double* delta,
                             double* grad_norm) {
  const char* what = "vb_factor_expected_delta";
  if (int rc = inspectCommon(h, what, which)) return rc;
  if (kind < 0 || kind >= 14) return fail(VB_E_ARG, "vb_factor_expected_delta: bad factor kind");
  const int64_t N = (int64_t)h->prob.fint[kind].size();
  if (first < 0 || n < 0 || first > N || n > N - first) return fail(VB_E_ARG, "vb_factor_expected_delta: rows out of range");
  if (n == 0) return 0;
  const Dev& d = h->fin->d;
  DevOwner S;  // frees its buffers when the call returns, on every path
  InsRows R;
  R.first = first, R.n = n;
  R.stepRed = which ? d.subRed : d.stepRed, R.stepPt = which ? d.subPt : d.stepPt;
  InsStage st;
  if (S.get(&R.v0, n) || S.get(&R.delta, n) || S.get(&R.gnorm, n) ||
      (kind != VB_F_VISUAL && allocStage(S, &st, std::min(kStageCap, n))))
    return devFail(S, "vb_factor_expected_delta: device allocation");
  hipStream_t s = h->str.st;
  HIPCHK(hipMemsetAsync(h->rep->err, 0, sizeof(int32_t), s));
  if (kind == VB_F_VISUAL) launch_visual_expected(d, h->rep->posOfRow, R, h->rep->err, s);
  else smallExpected(d, kind, R, st, s);
  HIPCHK(hipGetLastError());
  if (download(v0, (const double*)R.v0, n, s) || download(delta, (const double*)R.delta, n, s) ||
      download(grad_norm, (const double*)R.gnorm, n, s))
    return VB_E_HIP;
  return checkReportErr(h);
}

int vb_inspect_nonlinearities(vb_handle h, int which, uint32_t kind_mask, int32_t k, int32_t* kinds, int64_t* rows,
                              double* score, double* v0, double* delta, double* v1, double* grad_norm, int32_t* n_found,
                              int64_t* n_compared) {
  if (int rc = inspectRun(h, which, kind_mask, k)) return rc;
  return resultOut(h, kinds, rows, score, v0, delta, v1, grad_norm, n_found, n_compared);
}

int vb_set_inspect_iteration(vb_handle h, int iteration, int32_t k) {
  if (!h) return fail(VB_E_ARG, "vb_set_inspect_iteration: null handle");
  if (iteration > 0 && (k < 1 || k > VB_INSPECT_MAX_K))
    return fail(VB_E_ARG, "vb_set_inspect_iteration: k must be in [1, VB_INSPECT_MAX_K]");
  h->run.inspectIt = iteration > 0 ? iteration : 0;
  if (iteration > 0) h->run.inspectK = k;
  return 0;
}

int vb_inspection_result(vb_handle h, int32_t* kinds, int64_t* rows, double* score, double* v0, double* delta, double* v1,
                         double* grad_norm, int32_t* n_found, int64_t* n_compared) {
  if (!h) return fail(VB_E_ARG, "vb_inspection_result: null handle");
  return resultOut(h, kinds, rows, score, v0, delta, v1, grad_norm, n_found, n_compared);
}

int vb_inspect_device_ms(vb_handle h, double ms[3]) {
  if (!h || !ms) return fail(VB_E_ARG, "vb_inspect_device_ms: null argument");
  for (int i = 0; i < 3; i++) ms[i] = h->ins ? h->ins->ms[i] : 0.0;
  return 0;
}

}  // extern "C"
