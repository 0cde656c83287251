// Stand-alone check of the engine's resource owner (csrc/devmem.hpp) on the host, without a device: DevOwnerT
// over a counting fake backend that hands out malloc memory, can be told to fail its k-th call, and aborts on
// a free / destroy of something it did not hand out or has taken back already.
//   devmem_check <case>     exit 0, or 1 after printing what differs
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "../../visual_inertial_bundle_adjustment_amd/csrc/devmem.hpp"

namespace {

int failures = 0;
#define CHECK(c, ...)                                   \
  do {                                                  \
    if (!(c)) {                                         \
      std::printf("%s:%d: ", __FILE__, __LINE__);       \
      std::printf(__VA_ARGS__);                         \
      failures++;                                       \
    }                                                   \
  } while (0)

struct Fake {
  using Event = void*;
  using Stream = void*;
  static inline std::set<void*> dev, pin, ev, st;
  static inline int calls = 0, failAt = 0;   // failAt = k: the k-th call that can fail does
  static inline int frees = 0, nullSyncs = 0, asyncCopies = 0, drained = 0;
  static inline unsigned lastEventFlags = 0;

  static void reset() {
    calls = failAt = frees = nullSyncs = asyncCopies = drained = 0;
  }
  static bool failing() { return ++calls == failAt; }
  static void take(std::set<void*>& s, void* p, const char* what) {
    if (!s.erase(p)) {
      std::printf("%s of %p: not handed out, or given back already\n", what, p);
      std::abort();
    }
    std::free(p);
    frees++;
  }
  static int give(std::set<void*>& s, void** p, size_t bytes) {
    if (failing()) return 2;
    *p = std::malloc(bytes);
    std::memset(*p, 0xAB, bytes);
    s.insert(*p);
    return 0;
  }
  static int devAlloc(void** p, size_t bytes) { return give(dev, p, bytes); }
  static void devFree(void* p) { take(dev, p, "devFree"); }
  static int hostAlloc(void** p, size_t bytes) { return give(pin, p, bytes); }
  static void hostFree(void* p) { take(pin, p, "hostFree"); }
  static int zero(void* p, size_t bytes) {
    if (failing()) return 3;
    std::memset(p, 0, bytes);
    return 0;
  }
  static int copyIn(void* dst, const void* src, size_t bytes, Stream s) {
    if (failing()) return 4;
    std::memcpy(dst, src, bytes);
    if (s) asyncCopies++;
    return 0;
  }
  static int syncNull() {
    if (failing()) return 5;
    nullSyncs++;
    return 0;
  }
  static int eventCreate(Event* e, unsigned flags) {
    lastEventFlags = flags;
    return give(ev, e, 1);
  }
  static void eventDestroy(Event e) { take(ev, e, "eventDestroy"); }
  static int streamCreate(Stream* s) { return give(st, s, 1); }
  static void streamDestroy(Stream s) { drained++, take(st, s, "streamDestroy"); }
  static size_t live() { return dev.size() + pin.size() + ev.size() + st.size(); }
};
using Owner = viba_host::DevOwnerT<Fake>;

struct Counts {
  int64_t v[3];
  bool operator==(const Counts& o) const { return v[0] == o.v[0] && v[1] == o.v[1] && v[2] == o.v[2]; }
};
Counts counts() { return {{viba_host::g_live[0].load(), viba_host::g_live[1].load(), viba_host::g_live[2].load()}}; }
const Counts ZERO{{0, 0, 0}};

// the pointers of the twelve requests (all four kinds, every allocating member, a zero-length request)
struct Twelve {
  double *a = nullptr, *b = nullptr, *g = nullptr;
  const int32_t* c = nullptr;  // a pointer to const, as PreintArgs and CeArgs hold theirs
  int64_t *d = nullptr, *k = nullptr;
  float* z = nullptr;
  double* host = nullptr;
  void *e0 = nullptr, *e1 = nullptr, *s0 = nullptr, *s1 = nullptr;
};
const int32_t SRC[5] = {7, -1, 3, 9, 11};
const std::vector<int64_t> VEC = {5, 6, 7};

// runs the requests as the engine does (one || chain); returns the number that succeeded before the first failure
int twelve(Owner& m, Twelve& t, int* rc) {
  int n = 0;
  void* stream = (void*)&n;  // any non-null stream
  auto ok = [&](int r) { return r ? (*rc = r, false) : (n++, true); };
  *rc = 0;
  (void)(ok(m.get(&t.a, 10)) && ok(m.zeroed(&t.b, 4)) && ok(m.put(&t.c, SRC, 5, stream)) && ok(m.put(&t.d, VEC)) &&
         ok(m.pinned(&t.host, 32)) && ok(m.event(&t.e0)) && ok(m.event(&t.e1, 2u)) && ok(m.stream(&t.s0)) &&
         ok(m.zeroed(&t.z, 0)) && ok(m.get(&t.g, 0)) && ok(m.put(&t.k, std::vector<int64_t>())) && ok(m.stream(&t.s1)));
  return n;
}
const void* nth(const Twelve& t, int i) {
  const void* p[12] = {t.a, t.b, t.c, t.d, t.host, t.e0, t.e1, t.s0, t.z, t.g, t.k, t.s1};
  return p[i];
}

void scopeExit() {
  Fake::reset();
  {
    Owner m;
    Twelve t;
    int rc;
    CHECK(twelve(m, t, &rc) == 12 && rc == 0, "the twelve requests: rc %d\n", rc);
    for (int i = 0; i < 12; i++) CHECK(nth(t, i) != nullptr, "request %d left a null pointer\n", i);
    CHECK(Fake::dev.size() == 7 && Fake::pin.size() == 1 && Fake::ev.size() == 2 && Fake::st.size() == 2, "live sets\n");
    const Counts c = counts();
    // 10 + 4 doubles, 5 int32, 3 int64, one float, one double, one int64 (zero-length requests: one element)
    CHECK(c.v[0] == 80 + 32 + 20 + 24 + 4 + 8 + 8 && c.v[1] == 256 && c.v[2] == 4, "counters %lld %lld %lld\n",
          (long long)c.v[0], (long long)c.v[1], (long long)c.v[2]);
    CHECK(t.b[0] == 0.0 && t.b[3] == 0.0 && t.z[0] == 0.0f, "zeroed() did not clear\n");
    CHECK(std::memcmp(t.c, SRC, sizeof(SRC)) == 0 && std::memcmp(t.d, VEC.data(), 24) == 0, "put() did not copy\n");
    // zeroed() and the vector put() wait for the null stream, get() and the stream put() do not
    CHECK(Fake::nullSyncs == 4 && Fake::asyncCopies == 1, "null-stream waits %d, stream copies %d\n", Fake::nullSyncs,
          Fake::asyncCopies);
    CHECK(Fake::lastEventFlags == 2u, "event flags not passed on\n");
  }
  CHECK(Fake::live() == 0 && Fake::frees == 12 && Fake::drained == 2, "after scope exit: %zu live, %d frees\n", Fake::live(),
        Fake::frees);
  CHECK(counts() == ZERO, "counters not back to zero\n");
}

void releaseReuse() {
  Fake::reset();
  Owner m;
  Twelve t;
  int rc;
  twelve(m, t, &rc);
  m.release();
  CHECK(Fake::live() == 0 && Fake::frees == 12 && counts() == ZERO, "release() left something\n");
  m.release();  // nothing to give back: the fake aborts on a second free
  Twelve u;
  CHECK(twelve(m, u, &rc) == 12 && Fake::live() == 12 && counts().v[2] == 4, "the owner cannot be used after release()\n");
  m.release();
  CHECK(Fake::live() == 0 && Fake::frees == 24 && counts() == ZERO, "second release() left something\n");
}

void zeroLength() {
  Fake::reset();
  Owner m;
  double *a = nullptr, *b = nullptr, *h = nullptr;
  int32_t *c = nullptr, *d = nullptr;
  CHECK(!m.get(&a, 0) && !m.zeroed(&b, 0) && !m.put(&c, (const int32_t*)nullptr, 0, nullptr) &&
            !m.put(&d, std::vector<int32_t>()) && !m.pinned(&h, 0),
        "a zero-length request failed\n");
  CHECK(a && b && c && d && h, "a zero-length request returned null\n");
  CHECK(b[0] == 0.0, "one cleared element\n");
  a[0] = 1.0, c[0] = 1, d[0] = 1, h[0] = 1.0;  // one element each is there to write (AddressSanitizer checks)
  CHECK(counts().v[0] == 8 + 8 + 4 + 4 && counts().v[1] == 8, "one element each counted\n");
}

void failureSweep() {
  Fake::reset();
  int total;
  {
    Owner m;
    Twelve t;
    int rc;
    twelve(m, t, &rc);
    total = Fake::calls;
  }
  // one call per request; + clear and wait (zeroed, twice), + copy (the stream put), + copy and wait (the vector
  // put), + wait (the empty vector)
  CHECK(total == 12 + 2 * 2 + 1 + 2 + 1, "calls of the sequence: %d\n", total);
  for (int k = 1; k <= total; k++) {
    Fake::reset();
    Fake::failAt = k;
    Owner m;
    Twelve t;
    int rc;
    const int done = twelve(m, t, &rc);
    CHECK(done < 12 && rc != 0 && m.lastError() == rc, "k = %d: the sequence did not report the failure\n", k);
    CHECK(nth(t, done) == nullptr, "k = %d: the failing request %d left a pointer\n", k, done);
    for (int i = 0; i < done; i++) CHECK(nth(t, i) != nullptr, "k = %d: request %d before the failure is null\n", k, i);
    // the owner holds the requests before the failing one, nothing of the failing one
    CHECK((int)Fake::live() == done, "k = %d: %zu live after %d requests\n", k, Fake::live(), done);
    m.release();
    CHECK(Fake::live() == 0 && counts() == ZERO, "k = %d: release() left something\n", k);
  }
}

void twoOwners() {
  Fake::reset();
  {
    Owner a;
    double* p = nullptr;
    void* e = nullptr;
    a.get(&p, 100), a.event(&e);
    {
      Owner b;
      double *q = nullptr, *h = nullptr;
      void* s = nullptr;
      b.zeroed(&q, 50), b.pinned(&h, 4), b.stream(&s);
      const Counts c = counts();
      CHECK(c.v[0] == 800 + 400 && c.v[1] == 32 && c.v[2] == 2, "two owners do not add up\n");
      std::swap(p, q);  // pointers are freed by address, wherever they were kept
    }
    const Counts c = counts();
    CHECK(c.v[0] == 800 && c.v[1] == 0 && c.v[2] == 1, "after the inner owner\n");
  }
  CHECK(counts() == ZERO && Fake::live() == 0, "two owners: not back to zero\n");
}

}  // namespace

int main(int argc, char** argv) {
  static_assert(!std::is_copy_constructible<Owner>::value && !std::is_move_constructible<Owner>::value &&
                    !std::is_copy_assignable<Owner>::value && !std::is_move_assignable<Owner>::value,
                "an owner is neither copied nor moved");
  const std::string c = argc > 1 ? argv[1] : "";
  if (c == "scope_exit") scopeExit();
  else if (c == "release") releaseReuse();
  else if (c == "zero_length") zeroLength();
  else if (c == "failure_sweep") failureSweep();
  else if (c == "two_owners") twoOwners();
  else return std::printf("unknown case '%s'\n", c.c_str()), 2;
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
