// Host-only drive of the factor store's bookkeeping (gpmp_amd/csrc/factor_store.h) with the device stubbed out: "device" memory is
// malloc, copies are memcpy, events are counters.  Built with the host sanitizers and run directly by tests/test_factor_store_cpu.py;
// prints FACTOR-STORE-HOST-OK and exits 0 when every check holds.
#include <cmath>
#include <cstdio>
#include <string>
#include "../gpmp_amd/csrc/factor_store.h"

struct FakeDev {
  typedef int Stream;
  typedef int Event;
  static long live_allocs, live_events, waits, syncs;
  static size_t alloc_limit;
  static std::string log;
  static int alloc(void** p, size_t bytes) {
    if (bytes > alloc_limit) return 1;
    *p = std::malloc(bytes);
    ++live_allocs;
    return *p == nullptr;
  }
  static void free(void* p) { std::free(p); --live_allocs; }
  static int event_create(Event* e) { static int next = 1; *e = next++; ++live_events; return 0; }
  static void event_destroy(Event) { --live_events; }
  static int event_record(Event e, Stream s) { log += "R" + std::to_string(e % 2) + "s" + std::to_string(s) + " "; return 0; }
  static int stream_wait(Stream s, Event e) { ++waits; log += "W" + std::to_string(e % 2) + "s" + std::to_string(s) + " "; return 0; }
  static int event_sync(Event) { ++syncs; return 0; }
  static int copy(void* dst, const void* src, size_t bytes, Stream) { std::memcpy(dst, src, bytes); return 0; }
  static int compare(const double* x, const double* xcopy, size_t elems, const int* info, Stream, int* flag_dev, int* differ) {
    *flag_dev = (*info != 0) || std::memcmp(x, xcopy, sizeof(double) * elems) != 0;
    *differ = *flag_dev;
    return 0;
  }
};
long FakeDev::live_allocs = 0, FakeDev::live_events = 0, FakeDev::waits = 0, FakeDev::syncs = 0;
size_t FakeDev::alloc_limit = ~(size_t)0;
std::string FakeDev::log;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++failures; } } while (0)

int main() {
  using namespace gpmp;
  typedef FactorStore<FakeDev> Store;
  // ---- key bytes
  const double th[5] = {0.1, 0.2, 0.3, 0.4, 0.5};
  double th2[5] = {0.1, 0.2, 0.3, 0.4, 0.5};
  const auto k0 = factor_key_bytes(100, 3, 2, 0, 112, 16384, 0, 1e-10, th);
  CHECK(factor_key_equal(k0, factor_key_bytes(100, 3, 2, 0, 112, 16384, 0, 1e-10, th2)));
  th2[3] = std::nextafter(th2[3], 1.0);
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 2, 0, 112, 16384, 0, 1e-10, th2)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(101, 3, 2, 0, 112, 16384, 0, 1e-10, th)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 3, 0, 112, 16384, 0, 1e-10, th)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 2, 1, 112, 16384, 0, 1e-10, th)));      // one more parameter: another length
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 2, 0, 128, 16384, 0, 1e-10, th)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 2, 0, 112, 16384, 0, 2e-10, th)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 2, 2, 0, 112, 16384, 0, 1e-10, th)));
  CHECK(!factor_key_equal(k0, factor_key_bytes(100, 3, 2, 0, 112, 16384, 1, 1e-10, th)));      // factored by the other schedule
  const double zneg[4] = {-0.0, 0, 0, 0}, zpos[4] = {0.0, 0, 0, 0};                           // bit patterns, not values
  CHECK(!factor_key_equal(factor_key_bytes(4, 3, 2, 0, 16, 1, 0, 0.0, zneg), factor_key_bytes(4, 3, 2, 0, 16, 1, 0, 0.0, zpos)));
  // ---- budget arithmetic
  const size_t GiB = (size_t)1 << 30;
  CHECK(factor_store_budget(nullptr, 8 * GiB) == 2 * GiB);
  CHECK(factor_store_budget(nullptr, 400 * GiB) == 32 * GiB);
  CHECK(factor_store_budget(nullptr, 0) == 0);
  CHECK(factor_store_budget("0", 8 * GiB) == 0);
  CHECK(factor_store_budget("-5", 8 * GiB) == 0);
  CHECK(factor_store_budget("junk", 8 * GiB) == 0);
  CHECK(factor_store_budget("", 8 * GiB) == 0);
  CHECK(factor_store_budget("1.5", 0) == 1572864);
  CHECK(factor_store_budget("1e300", 0) == ~(size_t)0);
  CHECK(factor_store_bytes(100, 20, 3) == 8 * 123 + 256);
  // ---- the entry: publish / hit / miss / invalidate / release
  {
    Store s;
    const size_t le = 40, de = 16, xe = 12, big = 1 << 20;
    std::vector<double> x(xe, 1.0), x2(xe, 1.0);
    int info_ok = 0, info_bad = 7, mode = -1;
    double *L = nullptr, *dinv = nullptr;
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS && L && dinv == L + le);
    CHECK(!s.valid() && FakeDev::live_allocs == 1 && FakeDev::live_events == 2 && s.held_bytes() == factor_store_bytes(le, de, xe));
    for (size_t i = 0; i < le + de; ++i) L[i] = (double)i;            // "factor" into the store: every element is writable
    CHECK(s.publish(&info_ok, 1) == 0 && s.valid() && s.done(1) == 0);
    // same key, same points (another buffer), another stream: a hit behind the ready event
    FakeDev::log.clear();
    double* L2 = nullptr;
    CHECK(s.acquire(k0, x2.data(), xe, le, de, big, 2, &mode, &L2, &dinv) == 0 && mode == Store::HIT && L2 == L && L2[5] == 5.0);
    CHECK(FakeDev::log.rfind("W", 0) == 0 && FakeDev::log.find("s2") != std::string::npos);
    CHECK(s.done(2) == 0 && s.hits() == 1 && s.misses() == 1);
    // one entry of the points changed by one ulp, in place: a miss that waits for the reader on stream 2 before it overwrites
    x2[7] = std::nextafter(x2[7], 2.0);
    FakeDev::log.clear();
    CHECK(s.acquire(k0, x2.data(), xe, le, de, big, 3, &mode, &L, &dinv) == 0 && mode == Store::MISS && !s.valid());
    CHECK(FakeDev::log.find("W0s3") != std::string::npos && FakeDev::log.find("W1s3") != std::string::npos);   // both events
    // non-positive pivot: published with its info word, never hit, replaced by the next call
    CHECK(s.publish(&info_bad, 3) == 0 && s.done(3) == 0);
    CHECK(s.acquire(k0, x2.data(), xe, le, de, big, 3, &mode, &L, &dinv) == 0 && mode == Store::MISS);
    CHECK(s.publish(&info_ok, 3) == 0 && s.done(3) == 0);
    CHECK(s.acquire(k0, x2.data(), xe, le, de, big, 3, &mode, &L, &dinv) == 0 && mode == Store::HIT && s.done(3) == 0);
    // a call that fails between acquire and publish leaves no entry
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS && s.done(1) == 0 && !s.valid());
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS);
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    s.invalidate();
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS);
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    // another key (a larger problem): the buffers grow, the old ones are waited for and freed
    const auto k1 = factor_key_bytes(200, 3, 2, 0, 208, 32768, 0, 1e-10, th);
    const long syncs0 = FakeDev::syncs;
    CHECK(s.acquire(k1, x.data(), xe, 4 * le, 2 * de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS && dinv == L + 4 * le);
    CHECK(FakeDev::syncs == syncs0 + 2 && FakeDev::live_allocs == 1 && FakeDev::live_events == 2);
    for (size_t i = 0; i < 4 * le + 2 * de; ++i) L[i] = 1.0;
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    // ... and back to the smaller one: a miss in the buffers that are there
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS && FakeDev::live_allocs == 1);
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    // below the budget of the entry: bypass, nothing held, no error; likewise when the allocation fails; budget 0 releases
    CHECK(s.acquire(k0, x.data(), xe, le, de, factor_store_bytes(le, de, xe) - 1, 1, &mode, &L, &dinv) == 0 && mode == Store::BYPASS);
    CHECK(L == nullptr && !s.valid() && FakeDev::live_allocs == 0 && FakeDev::live_events == 0 && s.held_bytes() == 0);
    FakeDev::alloc_limit = 16;
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::BYPASS && FakeDev::live_allocs == 0);
    FakeDev::alloc_limit = ~(size_t)0;
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS);
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    CHECK(s.acquire(k0, x.data(), xe, le, de, 0, 1, &mode, &L, &dinv) == 0 && mode == Store::BYPASS && FakeDev::live_allocs == 0);
    // release: idempotent, everything returned
    CHECK(s.acquire(k0, x.data(), xe, le, de, big, 1, &mode, &L, &dinv) == 0 && mode == Store::MISS);
    CHECK(s.publish(&info_ok, 1) == 0 && s.done(1) == 0);
    CHECK(s.release() == 0 && s.release() == 0 && !s.valid());
  }
  CHECK(FakeDev::live_allocs == 0 && FakeDev::live_events == 0);
  if (failures == 0) std::printf("FACTOR-STORE-HOST-OK\n");
  return failures == 0 ? 0 : 1;
}
