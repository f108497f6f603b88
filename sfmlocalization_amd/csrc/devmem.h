// Ownership of device memory, for every handle and call of the library: one owner per array, so that freeing and the
// memory figures (sfmloc_map_info::hbm_bytes: Map and Ctx charge an account, nothing else does) need no list kept in
// step by hand.  No HIP here: raw allocation goes through two functions that capi.hip defines over hipMalloc / hipFree
// (and tests/cpp/devmem.cpp over malloc).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <memory>
#include <utility>

namespace sfmloc {

int dev_raw_alloc(void **p, size_t bytes);  // SFMLOC_OK, or an error code with the error text set; *p null on failure
void dev_raw_free(void *p);

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

}  // namespace sfmloc
