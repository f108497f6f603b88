// Host check of the device-memory owners (sfmlocalization_amd/csrc/devmem.h, the header Map, Ctx and Query are built
// from): raw allocation is supplied here over malloc, with a count of live allocations, the account the buffers are
// charged to, and an index at which the next allocations fail -- so every expectation below is a literal.
// The owners of streams, events and pinned host memory (same header) are checked the same way: their raw functions are
// counters here, and every raw call -- dev_raw_free included -- leaves a letter in a log, so the order of a struct's
// destruction reads as a string.
// Transfers (same header): the two raw functions are memcpy / memset here and leave 'c' (copy) and 'f' (fill) in the log;
// a null stream adds the wait's 'y', as the library's do.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <type_traits>
#include <vector>

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
}  // namespace sfmloc

// streams, events, pinned blocks: live counts, and the log of raw calls -- 'F' dev_raw_free, 'S' stream created, 'y'
// synchronised, 's' destroyed, 'E' / 'e' event created / destroyed, 'H' / 'h' pinned block allocated / freed
static int g_streams = 0, g_events = 0, g_blocks = 0;
static int g_timing_events = 0;  // events created with the timing flag
static int g_fail_raw = 0;       // the next raw creation of a stream, event or pinned block fails with this code
static std::string g_log;
static int raw_create(void **h, int *live, char letter, size_t bytes) {
  *h = nullptr;
  if (g_fail_raw) {
    const int rc = g_fail_raw;
    g_fail_raw = 0;
    return rc;
  }
  *h = malloc(bytes);  // (a distinct address per handle; a double release is a double free under a sanitizer)
  ++*live;
  g_log += letter;
  return 0;
}

namespace sfmloc {
void dev_raw_free(void *p) {
  g_last_freed = p;
  ++g_frees;
  --g_live;
  g_log += 'F';
  free(p);
}
int stream_raw_create(void **s) { return raw_create(s, &g_streams, 'S', 1); }
void stream_raw_sync(void *) { g_log += 'y'; }
void stream_raw_destroy(void *s) {
  --g_streams;
  g_log += 's';
  free(s);
}
int event_raw_create(void **e, bool timing) {
  const int rc = raw_create(e, &g_events, 'E', 1);
  if (!rc && timing) ++g_timing_events;
  return rc;
}
void event_raw_destroy(void *e) {
  --g_events;
  g_log += 'e';
  free(e);
}
int host_raw_alloc(void **p, size_t bytes) { return raw_create(p, &g_blocks, 'H', bytes); }
void host_raw_free(void *p) {
  --g_blocks;
  g_log += 'h';
  free(p);
}
}  // namespace sfmloc

// transfers: the bytes and the direction of the last raw copy, the byte value of the last raw fill, the last error text
static size_t g_raw_bytes = 0;
static int g_raw_kind = -1, g_raw_byte = -1;
static char g_err[256] = "";
namespace sfmloc {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}
int dev_raw_copy(void *dst, const void *src, size_t bytes, CopyKind kind, ihipStream_t *s) {
  memcpy(dst, src, bytes);
  g_raw_bytes = bytes;
  g_raw_kind = (int)kind;
  g_log += 'c';
  if (!s) stream_raw_sync(nullptr);
  return 0;
}
int dev_raw_fill(void *dst, int byte, size_t bytes, ihipStream_t *s) {
  memset(dst, byte, bytes);
  g_raw_bytes = bytes;
  g_raw_byte = byte;
  g_log += 'f';
  if (!s) stream_raw_sync(nullptr);
  return 0;
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
static_assert(!AddressTaken<Stream>::value && !AddressTaken<Event>::value && !AddressTaken<HostBuf<double>>::value,
              "operator& of a stream, an event or a pinned block is deleted");
static_assert(!std::is_copy_constructible<Stream>::value && !std::is_copy_assignable<Event>::value &&
                  !std::is_copy_constructible<HostBuf<int>>::value && std::is_nothrow_move_constructible<Event>::value &&
                  std::is_nothrow_move_constructible<EventPair>::value,
              "the owners are move-only");

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

// ---- streams, events, pinned host memory ----

// (a) each owner releases exactly once: at scope exit, after reset() and after a move; a moved-from owner releases nothing
static void test_owners_release_once() {
  g_log.clear();
  {
    Stream s;
    Event e;
    HostBuf<double> h;
    CHECK(!s && !e && !h && g_log.empty());  // nothing is created by a constructor
    CHECK(s.create() == 0 && e.create(kTimingEvent) == 0 && h.alloc(4) == 0);
    CHECK(s && e && h && g_streams == 1 && g_events == 1 && g_blocks == 1 && g_timing_events == 1);
    ihipStream_t *raw_s = s;  // read as the raw handles they replace
    ihipEvent_t *raw_e = e;
    double *raw_h = h;
    CHECK(raw_s == s.get() && raw_e == e.get() && raw_h == h.get());
    h[3] = 2.5;  // (a pinned block is host memory of that many elements)
    CHECK(h.get()[3] == 2.5);
    CHECK(s.ensure() == 0 && e.ensure(kTimingEvent) == 0 && s.get() == raw_s && e.get() == raw_e);  // ensure: once
  }
  CHECK(g_log == "SEHheys");  // scope exit, in reverse: the block, the event, the stream synchronised then destroyed
  CHECK(g_streams == 0 && g_events == 0 && g_blocks == 0);
  g_log.clear();
  {
    Stream s;
    Event e;
    HostBuf<int> h;
    CHECK(s.ensure() == 0 && e.ensure(kOrderingEvent) == 0 && h.alloc(1) == 0 && g_timing_events == 1);
    s.reset();
    e.reset();
    h.reset();
    CHECK(g_log == "SEHyseh" && !s && !e && !h);
    s.reset();
    e.reset();
    h.reset();
  }
  CHECK(g_log == "SEHyseh");  // reset twice and the destructors: nothing more
  g_log.clear();
  {
    Stream a;
    Event b;
    HostBuf<int> c;
    CHECK(a.create() == 0 && b.create(kOrderingEvent) == 0 && c.alloc(2) == 0);
    ihipStream_t *const ra = a;
    {
      Stream a2(std::move(a));
      Event b2;
      b2 = std::move(b);
      HostBuf<int> c2(std::move(c));
      CHECK(!a && !b && !c && a2.get() == ra && b2 && c2 && g_log == "SEH");
      a.reset();
      b.reset();
      c.reset();
      CHECK(g_log == "SEH");  // moved-from: nothing to release
      Event b3;
      CHECK(b3.create(kOrderingEvent) == 0);
      b3 = std::move(b2);  // over a live owner: its own event goes, the other moves in
      CHECK(g_log == "SEHEe" && g_events == 1 && !b2);
    }
    CHECK(g_log == "SEHEe" "ehys");  // b3, c2, a2 -- and b2 released nothing
  }
  CHECK(g_log == "SEHEe" "ehys" && g_streams == 0 && g_events == 0 && g_blocks == 0);
  g_log.clear();
  {
    Stream s;
    CHECK(s.create() == 0 && s.create() == 0);  // creating again lets the previous one go
    CHECK(g_log == "SysS" && g_streams == 1);
  }
  CHECK(g_streams == 0);
}

// (b) a failed creation answers the raw function's code and leaves the owner empty
static void test_owner_failed_creation() {
  g_log.clear();
  Stream s;
  Event e;
  HostBuf<float> h;
  g_fail_raw = -5;
  CHECK(s.create() == -5 && !s);
  g_fail_raw = -6;
  CHECK(e.ensure(kTimingEvent) == -6 && !e);
  g_fail_raw = -2;
  CHECK(h.alloc(8) == -2 && !h);
  CHECK(g_log.empty() && g_streams == 0 && g_events == 0 && g_blocks == 0);
  CHECK(s.create() == 0);  // ... also over a live owner: the old handle goes, the owner is empty, nothing leaks
  g_fail_raw = -5;
  CHECK(s.create() == -5 && !s && g_log == "Sys" && g_streams == 0);
  CHECK(s.ensure() == 0 && s);  // (and an empty owner can be created later)
}

// (c) a borrowed stream is never synchronised or destroyed
static void test_borrowed_stream() {
  g_log.clear();
  {
    Stream lender;
    CHECK(lender.create() == 0);
    {
      Stream b;
      b.borrow(lender);
      CHECK(b.get() == lender.get() && b.ensure() == 0 && g_log == "S");  // (ensure: it has one)
      Stream b2(std::move(b));
      CHECK(!b && b2.get() == lender.get());
      b2.reset();
      b2.borrow(lender);
    }
    CHECK(g_log == "S" && g_streams == 1);
    Stream own;
    CHECK(own.create() == 0);
    own.borrow(lender);  // (its own stream goes, the borrowed one is not its to release)
    CHECK(g_log == "SSys" && g_streams == 1);
  }
  CHECK(g_log == "SSysys" && g_streams == 0);  // only the lender's own
}

// (d) a handle's stream is declared before its buffers: both are freed before the stream is synchronised and destroyed
static void test_destruction_order() {
  struct Handle {
    Stream stream;
    DevBuf<float> a;
    DevBuf<int> b;
  };
  g_log.clear();
  {
    Handle h;
    CHECK(h.stream.create() == 0 && h.a.alloc(nullptr, 3) == 0 && h.b.alloc(nullptr, 5) == 0);
  }
  CHECK(g_log == "SFFys" && g_live == 0 && g_streams == 0);
}

// (e) a vector of event pairs: all destroyed when the vector goes, none twice after push_back reallocates
static void test_event_pairs() {
  g_log.clear();
  {
    std::vector<EventPair> pool;
    for (int i = 0; i < 9; ++i) {  // (capacity 1, 2, 4, 8, 16: four reallocations)
      EventPair p;
      CHECK(p.a.create(kTimingEvent) == 0 && p.b.create(kTimingEvent) == 0);
      pool.push_back(std::move(p));
    }
    CHECK(g_events == 18 && g_log == std::string(18, 'E'));  // moved, never released, by the reallocations
    std::vector<std::pair<int, EventPair>> pending;
    pending.emplace_back(3, std::move(pool.back()));
    pool.pop_back();
    CHECK(g_events == 18 && pool.size() == 8 && pending[0].second.a && pending[0].second.b);
    pool.push_back(std::move(pending[0].second));  // (drained: back into the pool; the moved-from entry is cleared later)
    pending.clear();
    CHECK(g_events == 18 && g_log == std::string(18, 'E'));
  }
  CHECK(g_events == 0 && g_log == std::string(18, 'E') + std::string(18, 'e'));
}

// (f) a pinned block of zero length is empty, and no error
static void test_pinned_zero_length() {
  g_log.clear();
  HostBuf<uint32_t> z;
  g_fail_raw = -2;  // (the raw allocator is not even asked)
  CHECK(z.alloc(0) == 0 && !z && g_fail_raw == -2);
  g_fail_raw = 0;
  CHECK(z.alloc(3) == 0 && z && z.alloc(0) == 0 && !z);  // ... and lets a previous block go
  CHECK(g_log == "Hh" && g_blocks == 0);
}

// ---- transfers ----

// (a) upload then download of a DevBuf<double>: n * 8 bytes each way; with an offset the elements outside the span keep
// their sentinel on both sides
static void test_transfer_round_trip() {
  Stream st;
  CHECK(st.create() == 0);
  DevBuf<double> d;
  CHECK(d.alloc(nullptr, 6) == 0 && d.size() == 6);
  for (int i = 0; i < 6; ++i) d.get()[i] = -1.0;  // (the "device" array is host memory here)
  const double src[3] = {1.5, 2.5, 3.5};
  g_log.clear();
  CHECK(d.upload(src, 3, st) == 0);
  CHECK(g_log == "c" && g_raw_bytes == 24 && g_raw_kind == (int)CopyKind::kHostToDevice);
  CHECK(d.get()[0] == 1.5 && d.get()[2] == 3.5 && d.get()[3] == -1.0);
  CHECK(d.upload(src, 2, st, 4) == 0 && g_raw_bytes == 16);
  CHECK(d.get()[3] == -1.0 && d.get()[4] == 1.5 && d.get()[5] == 2.5);
  double back[5] = {-7.0, -7.0, -7.0, -7.0, -7.0};
  CHECK(d.download(back + 1, 3, st, 2) == 0);
  CHECK(g_log == "ccc" && g_raw_bytes == 24 && g_raw_kind == (int)CopyKind::kDeviceToHost);
  CHECK(back[0] == -7.0 && back[1] == 3.5 && back[2] == -1.0 && back[3] == 1.5 && back[4] == -7.0);
  DevBuf<double> e;
  CHECK(e.alloc(nullptr, 2) == 0);
  CHECK(e.copy_from(d.get() + 4, 2, st) == 0 && g_raw_kind == (int)CopyKind::kDeviceToDevice && g_raw_bytes == 16);
  CHECK(e.get()[0] == 1.5 && e.get()[1] == 2.5);
}

// (b) whole-buffer zero and fill(0xFF) of 1 and of 3 elements
static void test_transfer_fill() {
  Stream st;
  CHECK(st.create() == 0);
  const size_t sizes[2] = {1, 3};
  for (size_t n : sizes) {
    DevBuf<uint64_t> d;
    CHECK(d.alloc(nullptr, n) == 0);
    for (size_t i = 0; i < n; ++i) d.get()[i] = 0x1234;
    g_log.clear();
    CHECK(d.zero(st) == 0 && g_log == "f" && g_raw_bytes == 8 * n && g_raw_byte == 0);
    for (size_t i = 0; i < n; ++i) CHECK(d.get()[i] == 0);
    CHECK(d.fill(0xFF, st) == 0 && g_log == "ff" && g_raw_bytes == 8 * n && g_raw_byte == 0xFF);
    for (size_t i = 0; i < n; ++i) CHECK(d.get()[i] == ~0ull);
  }
  DevBuf<uint64_t> d;
  CHECK(d.alloc(nullptr, 3) == 0);
  CHECK(d.fill(0xFF, st) == 0 && d.zero(1, st, 1) == 0 && g_raw_bytes == 8);  // one element in the middle
  CHECK(d.get()[0] == ~0ull && d.get()[1] == 0 && d.get()[2] == ~0ull);
}

// (c) an owned buffer refuses a span outside it: nothing issued, the array unchanged, both numbers in the text.
// An offset beyond the array is refused for zero elements too (decided here: such an offset is a bug whatever the count).
static void test_transfer_bounds() {
  Stream st;
  CHECK(st.create() == 0);
  DevBuf<uint32_t> d;
  CHECK(d.alloc(nullptr, 4) == 0);
  for (int i = 0; i < 4; ++i) d.get()[i] = 9;
  const uint32_t src[5] = {1, 2, 3, 4, 5};
  uint32_t back[5] = {0, 0, 0, 0, 0};
  g_log.clear();
  CHECK(d.upload(src, 1, st, 3) == 0 && g_log == "c" && d.get()[3] == 1);  // offset + n == size
  d.get()[3] = 9;
  g_log.clear();
  g_err[0] = 0;
  CHECK(d.upload(src, 5, st) == SFMLOC_EINVAL && g_log.empty());  // size + 1
  CHECK(strstr(g_err, "5 elements") && strstr(g_err, "array of 4"));
  CHECK(d.upload(src, 2, st, 3) == SFMLOC_EINVAL && d.download(back, 5, st) == SFMLOC_EINVAL);
  CHECK(d.zero(5, st) == SFMLOC_EINVAL && d.fill(0xFF, 1, st, 4) == SFMLOC_EINVAL && d.read(back, 5, st) == SFMLOC_EINVAL);
  CHECK(d.copy_from(d.get(), (size_t)-1, st, 2) == SFMLOC_EINVAL);  // (offset + n wraps around)
  CHECK(d.upload(src, 0, st, 4) == 0);                 // nothing, at the end: fine
  CHECK(d.upload(src, 0, st, 5) == SFMLOC_EINVAL);     // nothing, beyond the end: refused
  CHECK(g_log.empty() && back[0] == 0);
  for (int i = 0; i < 4; ++i) CHECK(d.get()[i] == 9);
}

// (d) zero elements: no raw call, no error -- members and free forms, an empty buffer's whole-buffer zero too
static void test_transfer_nothing() {
  DevBuf<float> d, empty;
  CHECK(d.alloc(nullptr, 2) == 0);
  float h[2] = {1.f, 2.f};
  g_log.clear();
  CHECK(d.upload(h, 0, nullptr) == 0 && d.download(h, 0, nullptr) == 0 && d.zero(0, nullptr) == 0 && d.read(h, 0, nullptr) == 0);
  CHECK(d.copy_from(d.get(), 0, nullptr) == 0 && empty.zero(nullptr) == 0 && empty.fill(0xFF, nullptr) == 0);
  CHECK(dev_upload(d.get(), h, 0, nullptr) == 0 && dev_download(h, d.get(), 0, nullptr) == 0 && dev_zero(d.get(), 0, nullptr) == 0 &&
        dev_fill(d.get(), 1, 0, nullptr) == 0 && dev_copy(d.get(), d.get(), 0, nullptr) == 0 && dev_read(h, d.get(), 0, nullptr) == 0);
  CHECK(g_log.empty());
}

// (e) the stream argument: a null stream is waited for inside the raw call, a stream is not; the blocking read copies on
// the named stream and then waits for it
static void test_transfer_streams() {
  Stream st;
  CHECK(st.create() == 0);
  DevBuf<int32_t> d;
  CHECK(d.alloc(nullptr, 2) == 0);
  int32_t h[2] = {4, 5};
  g_log.clear();
  CHECK(d.upload(h, 2, nullptr) == 0 && g_log == "cy");
  CHECK(d.zero(nullptr) == 0 && g_log == "cyfy");
  CHECK(d.download(h, 2, nullptr) == 0 && g_log == "cyfycy" && h[0] == 0);
  g_log.clear();
  CHECK(d.upload(h, 2, st) == 0 && d.zero(st) == 0 && d.download(h, 2, st) == 0 && d.fill(1, st) == 0 && g_log == "cfcf");
  g_log.clear();
  CHECK(d.read(h, 2, st) == 0 && g_log == "cy" && h[1] == 0x01010101);
  g_log.clear();
  CHECK(dev_read(h, d.get(), 1, st.get()) == 0 && g_log == "cy" && g_raw_bytes == 4);
}

// (f) a borrowed buffer has no size: it transfers without a bounds refusal
static void test_transfer_borrowed() {
  static uint16_t callers[8];
  DevBuf<uint16_t> b;
  b.borrow(callers);
  const uint16_t src[3] = {7, 8, 9};
  g_log.clear();
  CHECK(b.upload(src, 3, nullptr, 5) == 0 && g_log == "cy" && g_raw_bytes == 6);
  CHECK(callers[4] == 0 && callers[5] == 7 && callers[7] == 9);
  CHECK(b.zero(2, nullptr, 6) == 0 && callers[5] == 7 && callers[6] == 0 && callers[7] == 0);
}

// (g) the free forms over a T * into a record touch exactly sizeof(member) bytes
static void test_transfer_record_members() {
  struct Record {
    int32_t before;
    double pose[3];
    int32_t status;
    uint32_t stats[3];
    int32_t after;
  };
  Record dev;  // (stands for a record in device memory, as Ctx::d_result)
  memset(&dev, 0x55, sizeof dev);
  Stream st;
  CHECK(st.create() == 0);
  g_log.clear();
  CHECK(dev_zero(&dev.status, 1, st.get()) == 0 && g_raw_bytes == sizeof dev.status);
  CHECK(dev_zero(dev.stats, 3, st.get()) == 0 && g_raw_bytes == sizeof dev.stats);
  CHECK(dev_fill(dev.pose, 0xFF, 3, st.get()) == 0 && g_raw_bytes == sizeof dev.pose);
  CHECK(dev.before == 0x55555555 && dev.after == 0x55555555 && dev.status == 0 && dev.stats[0] == 0 && dev.stats[2] == 0);
  const double one_pose[3] = {1.0, 2.0, 3.0};
  CHECK(dev_upload(dev.pose, one_pose, 3, st.get()) == 0 && g_raw_bytes == sizeof dev.pose);
  double back[3] = {0, 0, 0};
  CHECK(dev_download(back, dev.pose, 3, st.get()) == 0 && back[0] == 1.0 && back[2] == 3.0);
  int32_t status = -1;
  CHECK(dev_read(&status, &dev.status, 1, st.get()) == 0 && status == 0 && g_raw_bytes == sizeof dev.status);
  CHECK(dev.before == 0x55555555 && dev.after == 0x55555555 && g_log == "fffcccy");
}

int main() {
  test_transfer_round_trip();
  test_transfer_fill();
  test_transfer_bounds();
  test_transfer_nothing();
  test_transfer_streams();
  test_transfer_borrowed();
  test_transfer_record_members();
  test_owners_release_once();
  test_owner_failed_creation();
  test_borrowed_stream();
  test_destruction_order();
  test_event_pairs();
  test_pinned_zero_length();
  g_log.clear();
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
