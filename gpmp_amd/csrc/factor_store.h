// The factor store: at most ONE Cholesky factor of K(xi, xi; theta) per device, kept across calls of the fused drivers (drivers.hip).
// A call whose observation points and covariance parameters are exactly those of the stored factor skips the Gram build and the
// factorisation and reads L from here (GPMP_FACTOR_STORE_MB).  Its readers are the drivers that leave L as it
// is -- the predictions, gpmp_nll_zero_mean, gpmp_reml, gpmp_posterior_weights -- and gpmp_whiten, through which the Python zero-mean
// likelihood (core/likelihood.py) finds the factor a prediction or an earlier evaluation on the same data left here.
// This header is host-only C++ without a HIP include: every device operation goes through the policy class `Dev`, which linalg.hip
// fills with HIP calls and tests/factor_store_host.cpp with host stand-ins, so the bookkeeping below runs under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace gpmp {

// Everything the stored bits depend on besides the points themselves, as bytes for memcmp: sizes, layout constants, the route the
// factorisation took (the one-stream and the look-ahead schedule round differently, and a hit must return what the caller's own
// factorisation would have), the covariance parameters (theta_host: 1 + noise + d doubles) and what the Gram gains on its diagonal.
// Doubles are compared as bit patterns.
inline std::vector<unsigned char> factor_key_bytes(int n, int d, int p, int noise, long ldn, size_t dinv_elems, int route, double diag,
                                                   const double* theta_host) {
  const long long head[7] = {n, d, p, noise, ldn, (long long)dinv_elems, route};
  const size_t nth = (size_t)(1 + (noise ? 1 : 0) + d);
  std::vector<unsigned char> key(sizeof(head) + sizeof(double) * (1 + nth));
  std::memcpy(key.data(), head, sizeof(head));
  std::memcpy(key.data() + sizeof(head), &diag, sizeof(double));
  std::memcpy(key.data() + sizeof(head) + sizeof(double), theta_host, sizeof(double) * nth);
  return key;
}

inline bool factor_key_equal(const std::vector<unsigned char>& a, const std::vector<unsigned char>& b) {
  return a.size() == b.size() && std::memcmp(a.data(), b.data(), a.size()) == 0;
}

// Budget of the store in bytes.  env: the value of GPMP_FACTOR_STORE_MB or NULL; a value that is not a positive number disables the
// store.  Unset: a quarter of the device memory that was free at first use, at most 32 GiB.
inline size_t factor_store_budget(const char* env, size_t free_at_first_use) {
  if (env != nullptr) {
    const double mb = std::strtod(env, nullptr);
    if (!(mb > 0.0)) return 0;
    return mb >= 1.6e13 ? ~(size_t)0 : (size_t)(mb * 1048576.0);
  }
  const size_t cap = (size_t)32 << 30, quarter = free_at_first_use / 4;
  return quarter < cap ? quarter : cap;
}

// Bytes one entry holds: L (n x ldn), the inverted diagonal blocks with their scratch, the copy of the points, two words
inline size_t factor_store_bytes(size_t l_elems, size_t dinv_elems, size_t x_elems) {
  return sizeof(double) * (l_elems + dinv_elems + x_elems) + 256;
}

// Dev provides (all static, 0 = success unless said otherwise):
//   typedef Stream, Event
//   int alloc(void** p, size_t bytes)         non-zero: out of memory (not an error of the call: the store is bypassed)
//   void free(void* p)
//   int event_create(Event* e);  void event_destroy(Event e);  int event_record(Event e, Stream s);
//   int stream_wait(Stream s, Event e);  int event_sync(Event e)
//   int copy(void* dst, const void* src, size_t bytes, Stream s)          device to device, asynchronous
//   int compare(const double* x, const double* xcopy, size_t elems, const int* info, Stream s, int* flag_dev, int* differ)
//       *differ = 0 iff x and xcopy agree as 64-bit patterns AND *info == 0; waits for the stream
template <class Dev>
class FactorStore {
 public:
  typedef typename Dev::Stream Stream;
  typedef typename Dev::Event Event;
  enum Mode { BYPASS = 0, HIT = 1, MISS = 2 };

  // Looks the key and the points up on stream s.  HIT: *L / *dinv hold the stored factor, ordered behind its factorisation.
  // MISS: *L / *dinv are the store's buffers for the caller to factor into (ordered behind every earlier reader); the entry is
  // invalid until publish().  BYPASS: the entry does not fit `budget` or could not be allocated; the caller uses its own workspace.
  // The caller holds the device's mutex from here to done().  Returns 0, or the first failing Dev call's code (*mode = BYPASS).
  int acquire(const std::vector<unsigned char>& key, const double* x, size_t x_elems, size_t l_elems, size_t dinv_elems, size_t budget,
              Stream s, int* mode, double** L, double** dinv) {
    *mode = BYPASS;
    *L = *dinv = nullptr;
    int rc = 0;
    const size_t bytes = factor_store_bytes(l_elems, dinv_elems, x_elems);
    if (cap_bytes_ > budget && (rc = release())) return rc;      // (a budget of 0 disables the store; what it held goes)
    if (bytes > budget) return 0;
    if (valid_ && factor_key_equal(key, key_)) {
      int differ = 1;
      if ((rc = Dev::stream_wait(s, ready_)) || (rc = Dev::compare(x, x_, x_elems, info_, s, flag_, &differ))) return rc;
      if (differ == 0) {
        ++hits_;
        *mode = HIT;
        *L = L_;
        *dinv = dinv_;
        return 0;
      }
    }
    // a miss: the newest factor replaces the old one
    valid_ = false;
    if (bytes > cap_bytes_) {
      if ((rc = release())) return rc;
      void* p = nullptr;
      if (Dev::alloc(&p, bytes) != 0) return 0;
      base_ = p;
      cap_bytes_ = bytes;
      if ((rc = Dev::event_create(&ready_))) { Dev::free(base_); base_ = nullptr; cap_bytes_ = 0; return rc; }
      if ((rc = Dev::event_create(&last_reader_))) { Dev::event_destroy(ready_); Dev::free(base_); base_ = nullptr; cap_bytes_ = 0; return rc; }
      have_events_ = true;
    } else {
      // the buffers are about to be overwritten: behind the factorisation that filled them and behind everything that read them
      if (recorded_ready_ && (rc = Dev::stream_wait(s, ready_))) return rc;
      if (recorded_reader_ && (rc = Dev::stream_wait(s, last_reader_))) return rc;
    }
    double* b = static_cast<double*>(base_);
    flag_ = reinterpret_cast<int*>(b);            // 256 bytes in front: [0] the compare flag, [1] the factorisation's info word
    info_ = flag_ + 1;
    L_ = b + 32;
    dinv_ = L_ + l_elems;
    x_ = dinv_ + dinv_elems;
    if ((rc = Dev::copy(x_, x, sizeof(double) * x_elems, s))) return rc;
    key_ = key;
    ++misses_;
    *mode = MISS;
    *L = L_;
    *dinv = dinv_;
    return 0;
  }

  // After a MISS, once the factorisation is enqueued on s: the info word it leaves goes with the entry (an entry whose word is
  // non-zero -- a non-positive pivot -- never hits: the compare reports it as different), and readers order themselves behind here.
  int publish(const int* info_dev, Stream s) {
    int rc = 0;
    if ((rc = Dev::copy(info_, info_dev, sizeof(int), s)) || (rc = Dev::event_record(ready_, s))) return rc;
    recorded_ready_ = true;
    valid_ = true;
    return 0;
  }

  // At the end of a HIT or MISS call: everything the call reads from the store has been enqueued on s.  One event stands for
  // all readers: s first waits for the reader before it, so the event's completion implies theirs.
  int done(Stream s) {
    int rc = 0;
    if (recorded_reader_ && (rc = Dev::stream_wait(s, last_reader_))) return rc;
    if ((rc = Dev::event_record(last_reader_, s))) return rc;
    recorded_reader_ = true;
    return 0;
  }

  void invalidate() { valid_ = false; }

  // Waits for the factorisation and the readers, then frees everything.  The first failure is returned; everything is freed anyway.
  int release() {
    int first = 0;
    valid_ = false;
    if (have_events_) {
      int rc;
      if (recorded_ready_ && (rc = Dev::event_sync(ready_)) && !first) first = rc;
      if (recorded_reader_ && (rc = Dev::event_sync(last_reader_)) && !first) first = rc;
      Dev::event_destroy(ready_);
      Dev::event_destroy(last_reader_);
      have_events_ = recorded_ready_ = recorded_reader_ = false;
    }
    if (base_ != nullptr) Dev::free(base_);
    base_ = nullptr;
    cap_bytes_ = 0;
    key_.clear();
    return first;
  }

  bool valid() const { return valid_; }
  size_t held_bytes() const { return cap_bytes_; }
  long hits() const { return hits_; }
  long misses() const { return misses_; }

 private:
  void* base_ = nullptr;
  size_t cap_bytes_ = 0;
  int* flag_ = nullptr;
  int* info_ = nullptr;
  double* L_ = nullptr;
  double* dinv_ = nullptr;
  double* x_ = nullptr;
  std::vector<unsigned char> key_;
  bool valid_ = false, have_events_ = false, recorded_ready_ = false, recorded_reader_ = false;
  Event ready_{}, last_reader_{};
  long hits_ = 0, misses_ = 0;
};

}  // namespace gpmp
