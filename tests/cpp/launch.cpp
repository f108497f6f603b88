// Host check of the dynamic-LDS limits every launch of the library goes through (sfmlocalization_amd/csrc/devmem.h
// "Dynamic-LDS limits": lds_allow, which launch.h calls before a launch): the raw function is supplied here, logs each
// call (kernel, bytes) and can be told to fail, so every expectation below is a literal.  The marks are per process and
// never reset, so every case takes kernels (addresses) of its own.
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <vector>

#include "../../sfmlocalization_amd/csrc/devmem.h"

struct RawCall {
  const void *kernel;
  uint32_t bytes;
};
static std::vector<RawCall> g_calls;
static int g_fail_next = 0;  // the next raw call answers this code instead of raising anything

namespace sfmloc {
int dev_raw_lds_limit(const void *kernel, uint32_t bytes) {
  g_calls.push_back({kernel, bytes});
  const int rc = g_fail_next;
  g_fail_next = 0;
  return rc;
}
void set_error(const char *, ...) {}
}  // namespace sfmloc
using sfmloc::lds_allow;

static int g_failed = 0;
#define CHECK(cond)                                            \
  do {                                                         \
    if (!(cond)) {                                             \
      printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      ++g_failed;                                              \
    }                                                          \
  } while (0)

static char g_kernels[600];  // addresses that stand for kernels
static const void *kernel(int i) { return &g_kernels[i]; }
static bool last_call_is(const void *k, uint32_t bytes) {
  return !g_calls.empty() && g_calls.back().kernel == k && g_calls.back().bytes == bytes;
}
constexpr uint32_t KiB = 1024;

static void test_default_needs_no_call() {
  g_calls.clear();
  CHECK(lds_allow(kernel(0), 0, 0) == 0);
  CHECK(lds_allow(kernel(0), 0, 1) == 0);
  CHECK(lds_allow(kernel(0), 0, 48 * KiB) == 0);
  CHECK(g_calls.empty());
  CHECK(lds_allow(kernel(0), 0, 48 * KiB + 1) == 0);  // (the first byte above it does)
  CHECK(g_calls.size() == 1 && last_call_is(kernel(0), 48 * KiB + 1));
}

static void test_one_call_per_rise() {
  g_calls.clear();
  CHECK(lds_allow(kernel(1), 0, 64 * KiB) == 0);
  CHECK(g_calls.size() == 1 && last_call_is(kernel(1), 64 * KiB));
  CHECK(lds_allow(kernel(1), 0, 64 * KiB) == 0);  // the same
  CHECK(lds_allow(kernel(1), 0, 50 * KiB) == 0);  // smaller
  CHECK(lds_allow(kernel(1), 0, 4 * KiB) == 0);
  CHECK(g_calls.size() == 1);
  CHECK(lds_allow(kernel(1), 0, 64 * KiB + 16) == 0);  // larger: one more
  CHECK(g_calls.size() == 2 && last_call_is(kernel(1), 64 * KiB + 16));
  CHECK(lds_allow(kernel(1), 0, 160 * KiB) == 0);
  CHECK(g_calls.size() == 3 && last_call_is(kernel(1), 160 * KiB));
  CHECK(lds_allow(kernel(1), 0, 64 * KiB + 16) == 0);
  CHECK(g_calls.size() == 3);
}

static void test_mark_per_device() {
  g_calls.clear();
  CHECK(lds_allow(kernel(2), 0, 100 * KiB) == 0);
  CHECK(g_calls.size() == 1);
  CHECK(lds_allow(kernel(2), 1, 100 * KiB) == 0);  // the second device has raised nothing yet
  CHECK(g_calls.size() == 2 && last_call_is(kernel(2), 100 * KiB));
  CHECK(lds_allow(kernel(2), 1, 80 * KiB) == 0);
  CHECK(lds_allow(kernel(2), 0, 100 * KiB) == 0);
  CHECK(g_calls.size() == 2);
  CHECK(lds_allow(kernel(2), 1, 120 * KiB) == 0);  // ... and rises alone
  CHECK(g_calls.size() == 3);
  CHECK(lds_allow(kernel(2), 0, 120 * KiB) == 0);
  CHECK(g_calls.size() == 4 && last_call_is(kernel(2), 120 * KiB));
  // every ordinal the table holds has a mark of its own
  for (int d = 2; d < sfmloc::kLdsDevices; ++d) CHECK(lds_allow(kernel(2), d, 60 * KiB) == 0);
  CHECK(g_calls.size() == 4 + (size_t)sfmloc::kLdsDevices - 2);
  for (int d = 0; d < sfmloc::kLdsDevices; ++d) CHECK(lds_allow(kernel(2), d, 60 * KiB) == 0);
  CHECK(g_calls.size() == 4 + (size_t)sfmloc::kLdsDevices - 2);
}

static void test_mark_per_kernel() {
  g_calls.clear();
  CHECK(lds_allow(kernel(3), 0, 100 * KiB) == 0);
  CHECK(lds_allow(kernel(4), 0, 100 * KiB) == 0);  // another kernel has raised nothing yet
  CHECK(g_calls.size() == 2 && last_call_is(kernel(4), 100 * KiB));
  CHECK(lds_allow(kernel(4), 0, 130 * KiB) == 0);
  CHECK(g_calls.size() == 3);
  CHECK(lds_allow(kernel(3), 0, 100 * KiB) == 0);
  CHECK(g_calls.size() == 3);
  CHECK(lds_allow(kernel(3), 0, 130 * KiB) == 0);  // ... and kernel 4's rise was not kernel 3's
  CHECK(g_calls.size() == 4 && last_call_is(kernel(3), 130 * KiB));
}

static void test_failure_leaves_the_mark() {
  g_calls.clear();
  g_fail_next = -7;
  CHECK(lds_allow(kernel(5), 0, 64 * KiB) == -7);  // the raw call's own code
  CHECK(g_calls.size() == 1);
  CHECK(lds_allow(kernel(5), 0, 64 * KiB) == 0);  // the mark stayed at the default: the next request tries again
  CHECK(g_calls.size() == 2 && last_call_is(kernel(5), 64 * KiB));
  CHECK(lds_allow(kernel(5), 0, 64 * KiB) == 0);
  CHECK(g_calls.size() == 2);
  g_fail_next = -7;
  CHECK(lds_allow(kernel(5), 0, 96 * KiB) == -7);  // ... and a failed rise leaves the mark it had
  CHECK(lds_allow(kernel(5), 0, 64 * KiB) == 0);
  CHECK(g_calls.size() == 3);
  CHECK(lds_allow(kernel(5), 0, 96 * KiB) == 0);
  CHECK(g_calls.size() == 4 && last_call_is(kernel(5), 96 * KiB));
}

// what has no mark still launches: a device ordinal beyond the table, or a kernel the full table has no slot for, makes
// the raw call before each of its launches above the default
static void test_without_a_mark() {
  g_calls.clear();
  for (int rep = 0; rep < 2; ++rep) {
    CHECK(lds_allow(kernel(6), sfmloc::kLdsDevices, 64 * KiB) == 0);
    CHECK(lds_allow(kernel(6), -1, 64 * KiB) == 0);
  }
  CHECK(g_calls.size() == 4);
  CHECK(lds_allow(kernel(6), -1, 48 * KiB) == 0);
  CHECK(g_calls.size() == 4);
  g_calls.clear();
  // more kernels than slots: kernels 0 .. 5 of the cases above hold one each (kernel 6 never asked with an ordinal that has marks)
  const int first = 10, many = sfmloc::kLdsKernels + 40, left_out = 40 + 6;
  for (int i = first; i < first + many; ++i) CHECK(lds_allow(kernel(i), 0, 64 * KiB) == 0);
  CHECK(g_calls.size() == (size_t)many);
  for (int i = first; i < first + many; ++i) CHECK(lds_allow(kernel(i), 0, 64 * KiB) == 0);
  CHECK(g_calls.size() == (size_t)many + left_out);  // those that found no slot call again, the others do not
  CHECK(lds_allow(kernel(1), 0, 160 * KiB) == 0);  // and a kernel that has its slot keeps its mark
  CHECK(g_calls.size() == (size_t)many + left_out);
}

int main() {
  test_default_needs_no_call();
  test_one_call_per_rise();
  test_mark_per_device();
  test_mark_per_kernel();
  test_failure_leaves_the_mark();
  test_without_a_mark();  // (last: it fills the table)
  if (g_failed) {
    printf("%d check(s) failed\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
