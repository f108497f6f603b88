// Ownership of device memory, for every handle and call of the library: one owner per array, so that freeing and the
// memory figures (sfmloc_map_info::hbm_bytes: Map and Ctx charge an account, nothing else does) need no list kept in
// step by hand.  No HIP here: raw allocation goes through two functions that capi.hip defines over hipMalloc / hipFree
// (and tests/cpp/devmem.cpp over malloc), and every transfer through two more ("Transfers" below states their rules).
// Below the device arrays: the kernels' dynamic-LDS limits, then the owners of streams, events and pinned host memory.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/sfmloc.h"
#include <atomic>
#include <memory>
#include <type_traits>
#include <utility>

struct ihipStream_t;  // what hipStream_t and hipEvent_t point to: opaque here as they are in HIP's own headers
struct ihipEvent_t;

namespace sfmloc {

int dev_raw_alloc(void **p, size_t bytes);  // SFMLOC_OK, or an error code with the error text set; *p null on failure
void dev_raw_free(void *p);
void set_error(const char *fmt, ...);  // (capi.hip: the calling thread's error text)

// ---------------------------------------------------------------------------
// Transfers: every copy into, out of or between device arrays, and every clear, goes through the two raw functions
// below (capi.hip: hipMemcpyAsync / hipMemsetAsync, the only places that name them) and names its stream.
//   - A stream: asynchronous on that stream, ordered with the rest of its work.
//   - A NULL stream: the operation HAS COMPLETED when the call returns (the raw function issues it on the null stream
//     and waits for that stream).  For an object that has no stream yet and must not create one just to fill its
//     tables; nothing else may rely on the null stream, which no non-blocking stream is ordered with.
// Counts are elements of the device array's type, so no site restates a sizeof; zero elements: no raw call, no error.
// A host pointer is void, or its elements make up the device array's (float for float2), or the device array is bytes.
// The members of an owned DevBuf refuse a span outside the array (SFMLOC_EINVAL, nothing issued); a pointer into a
// record or a borrowed array has no size to check.
// ---------------------------------------------------------------------------
enum class CopyKind { kHostToDevice, kDeviceToHost, kDeviceToDevice };
int dev_raw_copy(void *dst, const void *src, size_t bytes, CopyKind kind, ihipStream_t *s);  // codes as dev_raw_alloc
int dev_raw_fill(void *dst, int byte, size_t bytes, ihipStream_t *s);
void stream_raw_sync(void *s);  // (one of the owners' raw functions, below: waits for everything queued on s)

template <class T, class H>
constexpr bool host_type_fits() {
  if constexpr (std::is_void_v<H>) return true;
  else return sizeof(T) % sizeof(H) == 0 || sizeof(T) == 1;
}
template <class T>
inline int dev_fill(T *d, int byte, size_t n, ihipStream_t *s) {
  return n ? dev_raw_fill(d, byte, n * sizeof(T), s) : 0;
}
template <class T>
inline int dev_zero(T *d, size_t n, ihipStream_t *s) {
  return dev_fill(d, 0, n, s);
}
template <class T, class H>
inline int dev_upload(T *d, const H *h, size_t n, ihipStream_t *s) {
  static_assert(host_type_fits<T, H>(), "host elements that make up the device array's");
  return n ? dev_raw_copy(d, h, n * sizeof(T), CopyKind::kHostToDevice, s) : 0;
}
template <class T, class H>
inline int dev_download(H *h, const T *d, size_t n, ihipStream_t *s) {
  static_assert(host_type_fits<T, H>(), "host elements that make up the device array's");
  return n ? dev_raw_copy(h, d, n * sizeof(T), CopyKind::kDeviceToHost, s) : 0;
}
template <class T>
inline int dev_copy(T *d, const T *src, size_t n, ihipStream_t *s) {
  return n ? dev_raw_copy(d, src, n * sizeof(T), CopyKind::kDeviceToDevice, s) : 0;
}
// the blocking read: downloaded on s, and s waited for -- the host may read h when this returns SFMLOC_OK
template <class T, class H>
inline int dev_read(H *h, const T *d, size_t n, ihipStream_t *s) {
  const int rc = dev_download(h, d, n, s);
  if (!rc && n) stream_raw_sync(s);
  return rc;
}

// One device array, untyped: owned (freed here, its bytes charged to an account while held) or borrowed (never freed,
// never charged).  Move-only, and its address cannot be taken: an array gets in through alloc / borrow only, never
// through a `(void **)&member` handed to an allocator, which would leave it unowned.
class DevMem {
 public:
  DevMem() = default;
  DevMem(const DevMem &) = delete;
  DevMem &operator=(const DevMem &) = delete;
  DevMem(DevMem &&o) noexcept { take(o); }
  DevMem &operator=(DevMem &&o) noexcept {
    if (this != std::addressof(o)) {
      reset();
      take(o);
    }
    return *this;
  }
  ~DevMem() { reset(); }
  DevMem *operator&() = delete;

  // `acct` (may be null) grows by `bytes` now and shrinks by them when the array is freed; it outlives the buffer.
  // Zero bytes: an empty buffer, no charge, no error.
  int alloc_bytes(uint64_t *acct, size_t bytes) {
    reset();
    if (bytes == 0) return 0;
    int rc = dev_raw_alloc(&p_, bytes);
    if (rc) {
      p_ = nullptr;
      return rc;
    }
    bytes_ = bytes;
    acct_ = acct;
    if (acct_) *acct_ += bytes_;
    return 0;
  }
  void borrow_raw(void *p) {
    reset();
    p_ = p;
  }
  void reset() {
    if (bytes_) {  // (owned: a borrowed pointer has no bytes)
      dev_raw_free(p_);
      if (acct_) *acct_ -= bytes_;
    }
    p_ = nullptr;
    bytes_ = 0;
    acct_ = nullptr;
  }
  size_t bytes() const { return bytes_; }

 protected:
  // elements off .. off + n of an owned array of `elem`-byte elements lie inside it (a borrowed one is not checked)
  int span_inside(size_t elem, size_t off, size_t n) const {
    const size_t size = bytes_ / elem;
    if (!bytes_ || (off <= size && n <= size - off)) return 0;
    set_error("transfer of %zu elements from element %zu of a device array of %zu", n, off, size);
    return SFMLOC_EINVAL;
  }
  void *p_ = nullptr;

 private:
  void take(DevMem &o) {
    p_ = std::exchange(o.p_, nullptr);
    bytes_ = std::exchange(o.bytes_, 0);
    acct_ = std::exchange(o.acct_, nullptr);
  }
  size_t bytes_ = 0;
  uint64_t *acct_ = nullptr;
};

// ... typed: reads as the T* it replaces (kernel arguments, pointer arithmetic, null tests); get() where a conversion
// cannot apply (reinterpret_cast, varargs)
template <class T>
class DevBuf : public DevMem {
 public:
  int alloc(uint64_t *acct, size_t n) { return alloc_bytes(acct, n * sizeof(T)); }
  void borrow(const void *p) { borrow_raw(const_cast<void *>(p)); }  // the caller's array: never freed here
  T *get() const { return static_cast<T *>(p_); }
  operator T *() const { return get(); }

  // transfers (rules: above) of n elements from element `off` on; without a count: the whole owned array
  size_t size() const { return bytes() / sizeof(T); }
  int fill(int byte, size_t n, ihipStream_t *s, size_t off = 0) {
    const int rc = span_inside(sizeof(T), off, n);
    return rc ? rc : dev_fill(get() + off, byte, n, s);
  }
  int fill(int byte, ihipStream_t *s) { return fill(byte, size(), s); }
  int zero(size_t n, ihipStream_t *s, size_t off = 0) { return fill(0, n, s, off); }
  int zero(ihipStream_t *s) { return fill(0, size(), s); }
  template <class H>
  int upload(const H *h, size_t n, ihipStream_t *s, size_t off = 0) {
    const int rc = span_inside(sizeof(T), off, n);
    return rc ? rc : dev_upload(get() + off, h, n, s);
  }
  template <class H>
  int download(H *h, size_t n, ihipStream_t *s, size_t off = 0) const {
    const int rc = span_inside(sizeof(T), off, n);
    return rc ? rc : dev_download(h, get() + off, n, s);
  }
  int copy_from(const T *src, size_t n, ihipStream_t *s, size_t off = 0) {
    const int rc = span_inside(sizeof(T), off, n);
    return rc ? rc : dev_copy(get() + off, src, n, s);
  }
  template <class H>
  int read(H *h, size_t n, ihipStream_t *s, size_t off = 0) const {  // the blocking read
    const int rc = span_inside(sizeof(T), off, n);
    return rc ? rc : dev_read(h, get() + off, n, s);
  }
};

// All or nothing: the arrays of a set are allocated into the group and reach their owners (whose previous arrays are
// freed then) only through commit(), which the caller reaches only when ok().  A group that is dropped frees what it
// allocated and leaves every owner as it was.
class DevGroup {
 public:
  static constexpr int kMax = 12;
  explicit DevGroup(uint64_t *acct) : acct_(acct) {}
  template <class T>
  void add(DevBuf<T> &owner, size_t n) {
    if (rc_) return;
    if (n_ == kMax) {  // (more members than a group holds: refused like a failed allocation, never dropped)
      rc_ = -1;
      return;
    }
    owner_[n_] = std::addressof(owner);
    rc_ = fresh_[n_].alloc_bytes(acct_, n * sizeof(T));
    if (rc_) failed_bytes_ = n * sizeof(T);
    else ++n_;
  }
  bool ok() const { return rc_ == 0; }
  int rc() const { return rc_; }
  int failed_index() const { return n_; }  // when !ok(): which add() failed, and what it asked for
  size_t failed_bytes() const { return failed_bytes_; }
  void commit() {
    for (int i = 0; i < n_; ++i) *owner_[i] = std::move(fresh_[i]);
    n_ = 0;
  }

 private:
  uint64_t *acct_;
  DevMem fresh_[kMax];
  DevMem *owner_[kMax] = {};
  int n_ = 0, rc_ = 0;
  size_t failed_bytes_ = 0;
};

// ---------------------------------------------------------------------------
// Dynamic-LDS limits: before a launch that asks for more dynamic LDS than the default 48 KiB, the kernel's limit is
// raised through the raw function below (capi.hip: hipFuncSetAttribute on the device that is current, the only place
// that names it).  One rule for every kernel (launch.h applies it to every launch): remembered per kernel AND per device
// ordinal is the mark, the largest size for which the raw call has succeeded, 48 KiB to begin with.  A launch asking for
// more than the mark makes one raw call and raises the mark; one asking for that much or less makes none; a raw call
// that fails answers its code, leaves the mark, and the launch does not happen.
// Whether the runtime needs the call at all has not been measured: HIP's own header calls the function attributes of AMD
// devices "hints and controls" that "are ignored".  Per device is the conservative reading, nothing more is claimed.
// No lock: two host threads may both make the raw call for one kernel, which is harmless, and the lower of two marks
// stored at once only costs a later call.  A kernel the table has no slot left for, or a device ordinal beyond it, has
// no mark: the raw call is made before each of its launches above 48 KiB -- correct, but one runtime call per launch
// and nothing reports it, so kLdsKernels stays well above the number of such kernels (their gang forms included).
// ---------------------------------------------------------------------------
int dev_raw_lds_limit(const void *kernel, uint32_t bytes);  // codes as dev_raw_alloc

constexpr uint32_t kLdsDefaultLimit = 48 * 1024;
constexpr int kLdsDevices = 16, kLdsKernels = 256;  // (a dozen kernels and their gang forms ask for more than the default)
struct LdsMarks {
  std::atomic<const void *> kernel;
  std::atomic<uint32_t> mark[kLdsDevices];  // 0: nothing raised yet
};
inline LdsMarks g_lds_marks[kLdsKernels];  // (static storage: zeroed)

inline std::atomic<uint32_t> *lds_mark(const void *kernel, int device) {
  if (device < 0 || device >= kLdsDevices) return nullptr;
  const size_t h = (size_t)((reinterpret_cast<uintptr_t>(kernel) >> 3) * 0x9E3779B97F4A7C15ull >> 40);
  for (int probe = 0; probe < kLdsKernels; ++probe) {
    LdsMarks &e = g_lds_marks[(h + probe) % kLdsKernels];
    const void *k = e.kernel.load(std::memory_order_relaxed);
    if (!k && e.kernel.compare_exchange_strong(k, kernel, std::memory_order_relaxed)) k = kernel;  // (else k: who won)
    if (k == kernel) return &e.mark[device];
  }
  return nullptr;
}
// the limit of `kernel` on device ordinal `device` (the current one) allows `bytes` of dynamic LDS from here on
inline int lds_allow(const void *kernel, int device, uint32_t bytes) {
  if (bytes <= kLdsDefaultLimit) return 0;
  std::atomic<uint32_t> *mark = lds_mark(kernel, device);
  if (mark && bytes <= mark->load(std::memory_order_relaxed)) return 0;
  const int rc = dev_raw_lds_limit(kernel, bytes);
  if (!rc && mark) mark->store(bytes, std::memory_order_relaxed);
  return rc;
}

// ---------------------------------------------------------------------------
// The other three resources a handle or a call holds: a stream, an event, a block of pinned host memory.  Same rules as
// above (move-only, no address, empty after a failed creation, released exactly once), and raw creation goes through
// capi.hip / tests/cpp/devmem.cpp in the same way; it never counts as a typed device buffer for failure injection.
// Nothing is created in a constructor: a stream that merely exists shares a hardware queue with streams that work.
//
// Order of destruction, stated once: a handle (or a call) declares its Stream BEFORE its DevBufs, so the buffers are
// freed first -- kernels on the stream may still run then, which is safe because freeing waits for the device -- and
// the stream is drained and destroyed after them.
// ---------------------------------------------------------------------------
int stream_raw_create(void **s);  // a non-blocking stream; codes and *s as dev_raw_alloc (stream_raw_sync: above)
void stream_raw_destroy(void *s);
int event_raw_create(void **e, bool timing);
void event_raw_destroy(void *e);
int host_raw_alloc(void **p, size_t bytes);
void host_raw_free(void *p);

// one raw handle H*: owned (let go through Drop, once) or borrowed (never let go); reads as the H* it replaces
template <class H, void (*Drop)(void *)>
class RawOwner {
 public:
  RawOwner() = default;
  RawOwner(const RawOwner &) = delete;
  RawOwner &operator=(const RawOwner &) = delete;
  RawOwner(RawOwner &&o) noexcept : h_(std::exchange(o.h_, nullptr)), own_(std::exchange(o.own_, false)) {}
  RawOwner &operator=(RawOwner &&o) noexcept {
    if (this != std::addressof(o)) {
      reset();
      h_ = std::exchange(o.h_, nullptr);
      own_ = std::exchange(o.own_, false);
    }
    return *this;
  }
  ~RawOwner() { reset(); }
  RawOwner *operator&() = delete;
  void borrow(H *h) {  // somebody else's: never let go here
    reset();
    h_ = h;
  }
  void reset() {
    if (own_) Drop(h_);
    h_ = nullptr;
    own_ = false;
  }
  H *get() const { return h_; }
  operator H *() const { return h_; }

 protected:
  int adopt(int rc, void *h) {  // what a raw creation answered, after reset(): owned on SFMLOC_OK, empty otherwise
    if (rc) return rc;
    h_ = static_cast<H *>(h);
    own_ = true;
    return 0;
  }
  H *h_ = nullptr;
  bool own_ = false;
};

inline void stream_drain_destroy(void *s) {
  stream_raw_sync(s);
  stream_raw_destroy(s);
}
// a non-blocking stream (reads as hipStream_t): an owned one is synchronised, then destroyed; a borrowed one neither
class Stream : public RawOwner<ihipStream_t, stream_drain_destroy> {
 public:
  int create() {
    reset();  // (first: a previous one goes before the new one comes into being)
    void *s = nullptr;
    const int rc = stream_raw_create(&s);
    return adopt(rc, s);
  }
  int ensure() { return h_ ? 0 : create(); }  // created at first use
};

constexpr bool kTimingEvent = true, kOrderingEvent = false;  // (an ordering event cannot be timed and is cheaper)
// an event (reads as hipEvent_t)
class Event : public RawOwner<ihipEvent_t, event_raw_destroy> {
 public:
  int create(bool timing) {
    reset();
    void *e = nullptr;
    const int rc = event_raw_create(&e, timing);
    return adopt(rc, e);
  }
  int ensure(bool timing) { return h_ ? 0 : create(timing); }
};
struct EventPair {  // the two ends of a timed bracket
  Event a, b;
};

// pinned host memory, typed like DevBuf<T>.  Zero elements: an empty block, no error.
template <class T>
class HostBuf : public RawOwner<T, host_raw_free> {
 public:
  int alloc(size_t n) {
    this->reset();
    if (n == 0) return 0;
    void *p = nullptr;
    const int rc = host_raw_alloc(&p, n * sizeof(T));
    return this->adopt(rc, p);
  }
};

}  // namespace sfmloc
