// One owner for what the engine takes from the HIP runtime: device allocations, pinned host memory, events
// and streams.  A DevOwner remembers what it handed out and gives it back in release() and in its
// destructor; the raw pointers live wherever the kernels want them (Dev, the handle, a local), and are
// freed by address, so swapping two of them needs no care.  The handle keeps one owner per lifetime group
// (vb_handle_s), every per-call scratch is a local one.  No other file of csrc/ calls the runtime's
// allocate / create / free / destroy entries.  Every member returns 0 or the backend's error (lastError()).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <cstdint>
#include <type_traits>
#include <utility>
#include <vector>

namespace viba_host {

// process-wide: live device bytes, live pinned bytes, live events + streams (vb_debug_live_resources)
inline std::atomic<int64_t> g_live[3];

struct HipBackend {
  using Event = hipEvent_t;
  using Stream = hipStream_t;
  static int devAlloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void devFree(void* p) { (void)hipFree(p); }
  static int hostAlloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void hostFree(void* p) { (void)hipHostFree(p); }
  static int zero(void* p, size_t bytes) { return hipMemset(p, 0, bytes); }
  // st == nullptr: the blocking copy on the null stream
  static int copyIn(void* dst, const void* src, size_t bytes, Stream st) {
    return st ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, st) : hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
  }
  static int syncNull() { return hipStreamSynchronize(nullptr); }
  static int eventCreate(Event* e, unsigned flags) { return hipEventCreateWithFlags(e, flags); }
  static void eventDestroy(Event e) { (void)hipEventDestroy(e); }
  static int streamCreate(Stream* s) { return hipStreamCreateWithFlags(s, hipStreamNonBlocking); }
  static void streamDestroy(Stream s) { (void)hipStreamSynchronize(s), (void)hipStreamDestroy(s); }
};

template <class B = HipBackend>
class DevOwnerT {
 public:
  using Event = typename B::Event;
  using Stream = typename B::Stream;
  template <typename T>
  using Src = std::remove_const_t<T>;  // (not deduced: `out` alone fixes T, which may be const)

  DevOwnerT() = default;
  DevOwnerT(const DevOwnerT&) = delete;
  DevOwnerT& operator=(const DevOwnerT&) = delete;
  ~DevOwnerT() { release(); }

  // Every request: a count of zero still allocates one element; on failure *out is null and the owner holds
  // nothing of the request.
  // n elements, uninitialised
  template <typename T>
  int get(T** out, size_t n) {
    return make(out, n, false, nullptr, 0, Stream(), false);
  }
  // n elements, cleared.  hipMemset may return before the clear lands, and the engine's non-blocking streams do not
  // order behind it: a buffer allocated mid-run (the Gauss-Seidel pseudo-factor store) was once copied into
  // before its clear ran, leaving zero diagonal tiles (a "Cholesky breakdown" only in long test runs) --
  // hence the wait for the null stream
  template <typename T>
  int zeroed(T** out, size_t n) {
    return make(out, n, true, nullptr, 0, Stream(), true);
  }
  // n elements holding src[0, n), copied on stream st (nullptr: the blocking copy); no wait
  template <typename T>
  int put(T** out, const Src<T>* src, size_t n, Stream st) {
    return make(out, n, false, src, n, st, false);
  }
  // the elements of v.  The engine's streams are non-blocking: they do not order behind the null stream the copy
  // runs on, hence the wait for it
  template <typename T>
  int put(T** out, const std::vector<Src<T>>& v) {
    return make(out, v.size(), false, v.data(), v.size(), Stream(), true);
  }
  template <typename T>
  int pinned(T** out, size_t n) {
    *out = nullptr;
    void* p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if ((err_ = B::hostAlloc(&p, bytes))) return err_;
    pin_.push_back({p, bytes});
    g_live[1] += (int64_t)bytes;
    *out = (T*)p;
    return 0;
  }
  int event(Event* out, unsigned flags = 0) {
    *out = Event();
    Event e;
    if ((err_ = B::eventCreate(&e, flags))) return err_;
    ev_.push_back(e);
    g_live[2]++;
    *out = e;
    return 0;
  }
  int stream(Stream* out) {
    *out = Stream();
    Stream s;
    if ((err_ = B::streamCreate(&s))) return err_;
    st_.push_back(s);
    g_live[2]++;
    *out = s;
    return 0;
  }
  // gives everything back (a stream after its work has drained); the owner is then as new
  void release() {
    for (Event e : ev_) B::eventDestroy(e), g_live[2]--;
    for (const auto& m : dev_) B::devFree(m.first), g_live[0] -= (int64_t)m.second;
    for (const auto& m : pin_) B::hostFree(m.first), g_live[1] -= (int64_t)m.second;
    for (Stream s : st_) B::streamDestroy(s), g_live[2]--;
    ev_.clear(), dev_.clear(), pin_.clear(), st_.clear();
  }
  int lastError() const { return err_; }

 private:
  template <typename T>
  int make(T** out, size_t n, bool zero, const void* src, size_t nSrc, Stream st, bool sync) {
    *out = nullptr;
    void* p = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    if ((err_ = B::devAlloc(&p, bytes))) return err_;
    if (zero) err_ = B::zero(p, bytes);
    if (!err_ && nSrc) err_ = B::copyIn(p, src, nSrc * sizeof(T), st);
    if (!err_ && sync) err_ = B::syncNull();
    if (err_) {
      B::devFree(p);
      return err_;
    }
    dev_.push_back({p, bytes});
    g_live[0] += (int64_t)bytes;
    *out = (T*)p;
    return 0;
  }

  std::vector<std::pair<void*, size_t>> dev_, pin_;
  std::vector<Event> ev_;
  std::vector<Stream> st_;
  int err_ = 0;
};

using DevOwner = DevOwnerT<>;

}  // namespace viba_host
