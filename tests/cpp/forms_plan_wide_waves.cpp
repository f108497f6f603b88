// Host check of K3Plan::wide_waves (sfmlocalization_amd/csrc/forms.h): the waves per workgroup of the wide form's
// 1 024-match instance come from SFMLOC_K3_WIDE_WAVES (4 or 8, anything else: the default), the 2 048-match instance
// keeps four, a plan that is not wide -- a gang session, a list above 256 views -- has none, and nothing else of the
// plan depends on the knob.  The expected values are literals, as in forms_plan.cpp.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../sfmlocalization_amd/csrc/forms.h"

using namespace sfmloc;

static int g_failed = 0;
#define CHECK(cond)                                                 \
  do {                                                              \
    if (!(cond)) {                                                  \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_failed;                                                   \
    }                                                               \
  } while (0)

static K3In k3_in(uint32_t n_sel, bool gang, bool alone) {
  K3In in;
  in.n_sel = n_sel;
  in.ransac_round = 25;
  in.gang = gang;
  in.alone = alone;
  return in;
}

static bool same_but_wide_waves(K3Plan a, const K3Plan &b) {
  a.wide_waves = b.wide_waves;
  return a.wide == b.wide && a.wide_b0 == b.wide_b0 && a.max_m == b.max_m && a.k2 == b.k2 && a.waves == b.waves &&
         a.big == b.big && a.big_waves == b.big_waves && a.skip_le == b.skip_le;
}

int main() {
  CHECK(kK3WideWaves == 4 || kK3WideWaves == 8);
  CHECK(Knobs().k3_wide_waves == kK3WideWaves);
  for (int knob = 4; knob <= 8; knob += 4) {
    Knobs k;
    k.k3_wide_waves = knob;
    const Knobs d;
    for (int alone = 0; alone <= 1; ++alone) {
      // a short list outside a gang session: wide, on the knob's waves; the first batch is the 23 uniform iterations
      K3Plan p = plan_k3(k3_in(100, false, alone != 0), k);
      CHECK(p.wide && p.wide_waves == knob && p.wide_b0 == 23 && p.max_m == 1024 && p.skip_le == 1024);
      CHECK(same_but_wide_waves(p, plan_k3(k3_in(100, false, alone != 0), d)));
      p = plan_k3(k3_in(256, false, alone != 0), k);
      CHECK(p.wide && p.wide_waves == knob);
      // a list above 256 views: the plain forms, no wide waves, their own waves as before
      p = plan_k3(k3_in(257, false, alone != 0), k);
      CHECK(!p.wide && p.wide_waves == 0 && p.max_m == 512 && p.waves == (alone ? 16 : 4) && p.skip_le == 512);
      CHECK(same_but_wide_waves(p, plan_k3(k3_in(257, false, alone != 0), d)));
      // a gang session: plain
      p = plan_k3(k3_in(100, true, alone != 0), k);
      CHECK(!p.wide && p.wide_waves == 0 && p.max_m == 512 && p.waves == (alone ? 16 : 4));
      CHECK(same_but_wide_waves(p, plan_k3(k3_in(100, true, alone != 0), d)));
    }
    // the 2 048-match instance stays at four waves, whatever the knob; K2 in front of it as before
    K3In in = k3_in(100, false, true);
    in.huge_credit = 1;
    in.merge_deferred = true;
    K3Plan p = plan_k3(in, k);
    CHECK(p.wide && p.max_m == 2048 && p.wide_waves == 4 && p.k2 == K3Merge::kInFront);
    in.huge_credit = 0;
    p = plan_k3(in, k);
    CHECK(p.wide && p.max_m == 1024 && p.wide_waves == knob && p.k2 == K3Merge::kFolded);
    // SFMLOC_K3_WIDE = 2 in a gang session: wide, and then on the knob's waves
    k.k3_wide = 2;
    p = plan_k3(k3_in(100, true, true), k);
    CHECK(p.wide && p.wide_waves == knob);
  }
  // the environment: 4 and 8 are taken, anything else is the default
  static const struct { const char *v; int expect; } t[] = {
      {"4", 4}, {"8", 8}, {"0", kK3WideWaves}, {"16", kK3WideWaves}, {"6", kK3WideWaves}, {"", kK3WideWaves}, {"x", kK3WideWaves},
  };
  for (const auto &e : t) {
    setenv("SFMLOC_K3_WIDE_WAVES", e.v, 1);
    CHECK(read_knobs().k3_wide_waves == e.expect);
  }
  unsetenv("SFMLOC_K3_WIDE_WAVES");
  CHECK(read_knobs().k3_wide_waves == kK3WideWaves);
  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
