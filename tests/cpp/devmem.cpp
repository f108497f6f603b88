// Host check of the device-memory owners (sfmlocalization_amd/csrc/devmem.h, the header Map, Ctx and Query are built
// from): raw allocation is supplied here over malloc, with a count of live allocations, the account the buffers are
// charged to, and an index at which the next allocations fail -- so every expectation below is a literal.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>

#include "../../sfmlocalization_amd/csrc/devmem.h"

static int g_live = 0;         // allocations not yet freed
static int g_frees = 0;        // calls of dev_raw_free
static int g_fail_in = -1;     // the allocation that many calls from now fails (-1: none)
static void *g_last_freed = nullptr;

namespace sfmloc {
int dev_raw_alloc(void **p, size_t bytes) {
  *p = nullptr;
  if (g_fail_in >= 0 && g_fail_in-- == 0) return -2;
  *p = malloc(bytes);
  if (!*p) return -2;
  ++g_live;
  return 0;
}
void dev_raw_free(void *p) {
  g_last_freed = p;
  ++g_frees;
  --g_live;
  free(p);
}
}  // namespace sfmloc

using namespace sfmloc;

// the address of a buffer cannot be taken, so no `(void **)&member` can hand one to an allocator behind its back
template <class T, class = void>
struct AddressTaken : std::false_type {};
template <class T>
struct AddressTaken<T, std::void_t<decltype(&std::declval<T &>())>> : std::true_type {};
static_assert(AddressTaken<int>::value && !AddressTaken<DevBuf<int>>::value && !AddressTaken<DevMem>::value,
              "operator& of a device buffer is deleted");

static int g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

// (a) a buffer charges its account when it is allocated and refunds it on reset, destruction and move-assignment over it
static void test_charge_and_refund() {
  uint64_t acct = 0;
  {
    DevBuf<double> a;
    CHECK(a.get() == nullptr && a.bytes() == 0);
    CHECK(a.alloc(&acct, 10) == 0);
    CHECK(a.get() != nullptr && a.bytes() == 80 && acct == 80 && g_live == 1);
    double *as_pointer = a;  // reads as the pointer it replaces
    CHECK(as_pointer == a.get() && a + 3 == a.get() + 3 && a);
    a.reset();
    CHECK(a.get() == nullptr && a.bytes() == 0 && acct == 0 && g_live == 0);
    CHECK(a.alloc(&acct, 4) == 0);
    CHECK(acct == 32 && g_live == 1);
    CHECK(a.alloc(&acct, 6) == 0);  // (allocating again lets the previous array go)
    CHECK(acct == 48 && g_live == 1);
    DevBuf<double> b;
    CHECK(b.alloc(&acct, 100) == 0);
    CHECK(acct == 848 && g_live == 2);
    double *const pb = b.get();
    a = std::move(b);  // over a live buffer: a's 48 bytes are refunded, b's 800 stay charged
    CHECK(a.get() == pb && a.bytes() == 800 && acct == 800 && g_live == 1);
  }
  CHECK(acct == 0 && g_live == 0);  // destruction
  DevBuf<uint32_t> unaccounted;
  CHECK(unaccounted.alloc(nullptr, 5) == 0 && unaccounted.bytes() == 20 && g_live == 1);
  unaccounted.reset();
  CHECK(g_live == 0);
}

// (b) a moved-from buffer is empty and frees nothing
static void test_moved_from() {
  uint64_t acct = 0;
  DevBuf<float> a;
  CHECK(a.alloc(&acct, 8) == 0);
  float *const p = a.get();
  const int frees = g_frees;
  {
    DevBuf<float> b(std::move(a));
    CHECK(a.get() == nullptr && a.bytes() == 0);
    CHECK(b.get() == p && b.bytes() == 32 && acct == 32 && g_live == 1);
    a.reset();
    CHECK(g_frees == frees && acct == 32 && g_live == 1);
    DevBuf<float> c;
    c = std::move(b);
    CHECK(b.get() == nullptr && c.get() == p && g_frees == frees);
  }
  CHECK(g_frees == frees + 1 && g_last_freed == p && acct == 0 && g_live == 0);
}

// (c) a borrowed pointer is never passed to dev_raw_free and charges nothing
static void test_borrowed() {
  static uint32_t callers[4];
  const int frees = g_frees;
  {
    DevBuf<uint32_t> v;
    v.borrow(callers);
    CHECK(v.get() == callers && v.bytes() == 0 && g_live == 0);
    DevBuf<uint32_t> w(std::move(v));
    CHECK(w.get() == callers && v.get() == nullptr);
    w.reset();
    CHECK(w.get() == nullptr);
    w.borrow(callers);
  }
  CHECK(g_frees == frees && g_live == 0);
  uint64_t acct = 0;
  DevBuf<uint32_t> o;
  CHECK(o.alloc(&acct, 4) == 0);
  o.borrow(callers);  // (the owned array goes, the borrowed one is not charged)
  CHECK(g_frees == frees + 1 && acct == 0 && g_live == 0 && o.get() == callers);
}

// (d) a 12-member group that fails at index 0, 5 and 11 leaves the live count, the account and the owners as they were;
// (e) a successful one replaces the old set
static void test_group() {
  uint64_t acct = 0;
  DevBuf<uint64_t> owner[12];
  void *old[12];
  for (int i = 0; i < 12; ++i) {
    CHECK(owner[i].alloc(&acct, (size_t)i + 1) == 0);
    old[i] = owner[i].get();
  }
  CHECK(g_live == 12 && acct == 8 * 78);  // 1 + 2 + ... + 12 = 78 elements
  const int fail_at[3] = {0, 5, 11};
  for (int k : fail_at) {
    g_fail_in = k;
    {
      DevGroup g(&acct);
      for (int i = 0; i < 12; ++i) g.add(owner[i], 100 + (size_t)i);
      CHECK(!g.ok() && g.rc() == -2 && g.failed_index() == k && g.failed_bytes() == 8 * (100 + (size_t)k));
      CHECK(g_live == 12 + k);  // (what it got so far is still held ...)
    }
    g_fail_in = -1;
    CHECK(g_live == 12 && acct == 8 * 78);  // (... and goes with the group)
    for (int i = 0; i < 12; ++i) CHECK(owner[i].get() == old[i] && owner[i].bytes() == 8 * ((size_t)i + 1));
  }
  {
    DevGroup g(&acct);
    for (int i = 0; i < 12; ++i) g.add(owner[i], 100 + (size_t)i);
    CHECK(g.ok() && g.rc() == 0);
    CHECK(g_live == 24 && acct == 8 * 78 + 8 * 1266);  // old and new side by side until the commit: 1200 + 66 elements
    for (int i = 0; i < 12; ++i) CHECK(owner[i].get() == old[i]);
    g.commit();
    CHECK(g_live == 12 && acct == 8 * 1266);
  }
  CHECK(g_live == 12 && acct == 8 * 1266);  // (a committed group owns nothing)
  for (int i = 0; i < 12; ++i) CHECK(owner[i].get() != nullptr && owner[i].bytes() == 8 * (100 + (size_t)i));
  {  // a group over owners that are still empty (a lazily made set): a failure leaves none of them set
    DevBuf<float> lazy[3];
    g_fail_in = 2;
    {
      DevGroup g(&acct);
      for (auto &b : lazy) g.add(b, 7);
      CHECK(!g.ok() && g.failed_index() == 2);
    }
    g_fail_in = -1;
    for (auto &b : lazy) CHECK(b.get() == nullptr);
    CHECK(g_live == 12 && acct == 8 * 1266);
  }
  {  // a 13th member is refused, not dropped: the group fails and nothing is committed
    DevBuf<float> many[13];
    DevGroup g(&acct);
    for (auto &b : many) g.add(b, 1);
    CHECK(!g.ok() && g.rc() != 0 && g_live == 24);
  }
  CHECK(g_live == 12 && acct == 8 * 1266);
  for (auto &b : owner) b.reset();
  CHECK(g_live == 0 && acct == 0);
}

// (f) a zero-length allocation gives a null buffer, charges nothing, and is not an error
static void test_zero_length() {
  uint64_t acct = 0;
  DevBuf<int32_t> z;
  g_fail_in = 0;  // (the raw allocator is not even asked)
  CHECK(z.alloc(&acct, 0) == 0);
  CHECK(g_fail_in == 0);
  g_fail_in = -1;
  CHECK(z.get() == nullptr && z.bytes() == 0 && acct == 0 && g_live == 0);
  DevBuf<int32_t> a;
  CHECK(a.alloc(&acct, 3) == 0);
  CHECK(a.alloc(&acct, 0) == 0);  // ... and lets a previous array go
  CHECK(a.get() == nullptr && acct == 0 && g_live == 0);
  g_fail_in = 0;
  CHECK(a.alloc(&acct, 3) == -2);  // a failed allocation: empty, nothing charged
  g_fail_in = -1;
  CHECK(a.get() == nullptr && a.bytes() == 0 && acct == 0 && g_live == 0);
}

int main() {
  test_charge_and_refund();
  test_moved_from();
  test_borrowed();
  test_group();
  test_zero_length();
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
