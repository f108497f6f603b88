// Host check of the kernel-form policy (sfmlocalization_amd/csrc/forms.h, the header the launch functions include):
// every boundary of DESIGN.md's "Kernel forms" table, with the expected plans written out as literals -- worked out from
// the launch code this header replaced and from that table, not from a second copy of the rules.
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

// ---------------------------------------------------------------------------------------------------------------------
static K1In k1_in(uint32_t nq, uint32_t blocks, bool use_list, bool may_slice) {
  K1In in;
  in.nq = nq;
  in.n_work_blocks = blocks;
  in.n_cu = 256;
  in.use_list = use_list;
  in.may_slice = may_slice;
  return in;
}

static void test_k1() {
  const Knobs d;
  // screened from 12 heads of query rows on; exact below, with exact_rows, with a split scan
  CHECK(!plan_k1(k1_in(767, 312500, false, true), d).screened());
  CHECK(plan_k1(k1_in(768, 312500, false, true), d).screened());
  {
    K1In in = k1_in(2000, 312500, false, true);
    in.exact_rows = true;
    CHECK(plan_k1(in, d).form == K1Form::kExact);
    in.exact_rows = false;
    in.split = 2;
    CHECK(plan_k1(in, d).form == K1Form::kExact);
    CHECK(plan_k1(in, d).exact_waves == 8);
  }
  // the exact form's geometry either side of 32 wave-blocks per compute unit (8 192), and its lane-ops
  CHECK(plan_k1(k1_in(500, 8191, false, true), d).exact_waves == 4);
  CHECK(plan_k1(k1_in(500, 8192, false, true), d).exact_waves == 8);
  {
    K1In in = k1_in(500, 4096, true, true);
    in.split = 2;
    CHECK(plan_k1(in, d).exact_waves == 8);
    in.n_work_blocks = 4095;
    CHECK(plan_k1(in, d).exact_waves == 4);
  }
  {
    const K1Plan p = plan_k1(k1_in(500, 100, true, true), d);
    CHECK(p.form == K1Form::kExact && p.exact_waves == 4 && p.lane_ops_per_row == 17500);
    CHECK(!p.shared_head && !p.clear_flagmask);
  }
  // the full bank, no list: the lean form in one slice
  {
    const K1Plan p = plan_k1(k1_in(2000, 312500, false, true), d);
    CHECK(p.form == K1Form::kLean && p.slices == 1 && p.head == 64 && !p.shared_head && !p.clear_flagmask);
    CHECK(p.lane_ops_per_row == 42896 && p.finish_ops == 17);  // 64 x 35 + 1 936 x 21
    CHECK(plan_k1(k1_in(2000, 312500, false, false), d).form == K1Form::kLean);
  }
  // a shortlist while the GPU is shared: the matrix cores, or with params.k1_mfma = 0 the popcount shortlist form
  {
    K1In in = k1_in(2000, 3150, true, false);
    K1Plan p = plan_k1(in, d);
    CHECK(p.form == K1Form::kMfma && p.slices == 1 && !p.shared_head && !p.clear_flagmask);
    CHECK(p.lane_ops_per_row == 4776 && p.finish_ops == 0);
    in.k1_mfma = false;
    p = plan_k1(in, d);
    CHECK(p.form == K1Form::kShortlist && p.slices == 1 && p.finish_ops == 17);
    CHECK(p.lane_ops_per_row == 42896);
  }
  // a query alone: the batched tail below 16 blocks per compute unit (4 096), sliced, on a shared head
  {
    K1Plan p = plan_k1(k1_in(2000, 3150, true, true), d);
    CHECK(p.form == K1Form::kBatchedTail && p.slices == 7 && p.shared_head && p.clear_flagmask && p.head == 64);
    CHECK(p.lane_ops_per_row == 42896 && p.finish_ops == 17);
    p = plan_k1(k1_in(2000, 4095, true, true), d);
    CHECK(p.form == K1Form::kBatchedTail && p.slices == 3);
    p = plan_k1(k1_in(2000, 4095, false, true), d);
    CHECK(p.form == K1Form::kBatchedTail && p.slices == 3);
    p = plan_k1(k1_in(2000, 4096, true, true), d);  // a sliced scan of a view list: the popcount shortlist form
    CHECK(p.form == K1Form::kShortlist && p.slices == 2 && p.shared_head && p.clear_flagmask);
    p = plan_k1(k1_in(2000, 4096, false, true), d);
    CHECK(p.form == K1Form::kLean && p.slices == 2 && p.shared_head);
    p = plan_k1(k1_in(2000, 8192, true, true), d);  // a long list, alone: unsliced, the matrix cores
    CHECK(p.form == K1Form::kMfma && p.slices == 1);
    // shared: never the batched tail, never sliced
    p = plan_k1(k1_in(2000, 4095, true, false), d);
    CHECK(p.form == K1Form::kMfma && p.slices == 1);
    p = plan_k1(k1_in(2000, 4095, false, false), d);
    CHECK(p.form == K1Form::kLean && p.slices == 1);
    p = plan_k1(k1_in(2000, 4096, true, false), d);
    CHECK(p.form == K1Form::kMfma && p.slices == 1);
  }
  // SFMLOC_K1_SCREEN_BATCH 1 / 4, SFMLOC_K1_QSPLIT
  {
    Knobs k;
    k.k1_screen_batch = 1;  // alone, but lean: the slice model still counts three workgroups per compute unit
    K1Plan p = plan_k1(k1_in(2000, 3150, true, true), k);
    CHECK(p.form == K1Form::kShortlist && p.slices == 7 && p.shared_head);
    k.k1_qsplit = 1;
    p = plan_k1(k1_in(2000, 3150, true, true), k);
    CHECK(p.form == K1Form::kMfma && p.slices == 1 && !p.shared_head);
    k = Knobs();
    k.k1_screen_batch = 4;  // shared, but the batched tail
    p = plan_k1(k1_in(2000, 3150, true, false), k);
    CHECK(p.form == K1Form::kBatchedTail && p.slices == 1 && !p.shared_head);
    p = plan_k1(k1_in(2000, 4096, true, false), k);
    CHECK(p.form == K1Form::kMfma);
    k = Knobs();
    k.k1_qsplit = 4;  // a shared shortlist scan forced into slices: off the matrix cores
    p = plan_k1(k1_in(2000, 3150, true, false), k);
    CHECK(p.form == K1Form::kShortlist && p.slices == 4 && p.shared_head && p.clear_flagmask);
    k.k1_screen_head = 128;
    CHECK(plan_k1(k1_in(2000, 3150, true, false), k).head == 128);
  }
  // the slice count (256 compute units, head 64)
  {
    static const struct { uint32_t blocks, nq, slices; } t[] = {
        {3150, 2000, 7}, {3150, 768, 3},  {3535, 2262, 5}, {4095, 2000, 3}, {4096, 2000, 2},
        {6144, 2000, 4}, {8191, 2000, 1}, {8192, 2000, 1}, {100, 2000, 8},  {3150, 64, 1},
    };
    for (const auto &e : t) {
      CHECK(k1_slices(k1_in(e.nq, e.blocks, true, true), d) == e.slices);
      CHECK(k1_slices(k1_in(e.nq, e.blocks, false, true), d) == e.slices);
      CHECK(k1_slices(k1_in(e.nq, e.blocks, true, false), d) == 1);  // never when other queries are queued
      for (int q = 0; q <= 18; ++q) {  // SFMLOC_K1_QSPLIT 1 .. 16 is the slice count, alone or not
        Knobs k;
        k.k1_qsplit = q;
        CHECK(k1_slices(k1_in(e.nq, e.blocks, true, true), k) == ((q >= 1 && q <= 16) ? (uint32_t)q : e.slices));
        CHECK(k1_slices(k1_in(e.nq, e.blocks, true, false), k) == ((q >= 1 && q <= 16) ? (uint32_t)q : 1u));
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static K3In k3_in(uint32_t n_sel, bool gang, bool alone) {
  K3In in;
  in.n_sel = n_sel;
  in.ransac_round = 1024;
  in.gang = gang;
  in.alone = alone;
  return in;
}

static void test_k3() {
  const Knobs d;
  // wide for view lists up to 256 outside gang sessions: the 1 024 instance, one launch
  {
    K3Plan p = plan_k3(k3_in(256, false, true), d);
    CHECK(p.wide && p.wide_b0 == 32 && p.max_m == 1024 && p.skip_le == 1024 && p.k2 == K3Merge::kDone && !p.big);
    p = plan_k3(k3_in(256, false, false), d);  // alone or shared
    CHECK(p.wide && p.max_m == 1024 && p.skip_le == 1024);
    p = plan_k3(k3_in(257, false, true), d);
    CHECK(!p.wide && p.max_m == 512 && p.waves == 16 && !p.big && p.skip_le == 512 && p.k2 == K3Merge::kDone);
    p = plan_k3(k3_in(100, true, true), d);
    CHECK(!p.wide && p.max_m == 512 && p.skip_le == 512);
  }
  // SFMLOC_K3_WIDE 0 / 1 / 2
  {
    Knobs k;
    k.k3_wide = 0;
    CHECK(!plan_k3(k3_in(100, false, true), k).wide);
    k.k3_wide = 2;
    CHECK(plan_k3(k3_in(100, true, true), k).wide);
    CHECK(plan_k3(k3_in(100, false, false), k).wide);
    CHECK(!plan_k3(k3_in(257, false, true), k).wide);
    // a first batch of fewer than two iterations: never
    K3In in = k3_in(100, false, true);
    in.ransac_round = 1;
    CHECK(!plan_k3(in, k).wide && plan_k3(in, k).wide_b0 == 1);
    CHECK(!plan_k3(in, d).wide);
    in.ransac_round = 2;
    CHECK(plan_k3(in, d).wide && plan_k3(in, d).wide_b0 == 2);
    in.ransac_round = 20;  // 18 uniform iterations
    CHECK(plan_k3(in, d).wide && plan_k3(in, d).wide_b0 == 18);
    in.ransac_round = 36;  // 33
    CHECK(plan_k3(in, d).wide_b0 == 32);
  }
  // the 2 048 instance: huge credit 0 / 1, SFMLOC_K3_WIDE_2048 0 / 1 / 2; K2 folded in at 1 024, in front at 2 048
  for (int knob = 0; knob <= 2; ++knob)
    for (int credit = 0; credit <= 1; ++credit)
      for (int deferred = 0; deferred <= 1; ++deferred) {
        Knobs k;
        k.k3_wide_2048 = knob;
        K3In in = k3_in(100, false, true);
        in.huge_credit = credit;
        in.merge_deferred = deferred != 0;
        static const bool expect_huge[3][2] = {{false, false}, {false, true}, {true, true}};  // [knob][credit]
        const bool huge = expect_huge[knob][credit];
        K3Plan p = plan_k3(in, k);
        CHECK(p.wide && p.max_m == (huge ? 2048 : 1024) && p.skip_le == (huge ? 2048 : 1024));
        CHECK(p.k2 == (!deferred ? K3Merge::kDone : huge ? K3Merge::kInFront : K3Merge::kFolded));
        in.gang = true;  // not wide: no 2 048 instance either, and K2 goes into the plain launch
        p = plan_k3(in, k);
        CHECK(!p.wide && p.max_m == 512 && p.skip_le == 512);
        CHECK(p.k2 == (deferred ? K3Merge::kFolded : K3Merge::kDone));
      }
  // plain: waves per view
  {
    Knobs k;
    CHECK(plan_k3(k3_in(300, false, true), k).waves == 16);
    CHECK(plan_k3(k3_in(300, false, false), k).waves == 4);
    k.k3_waves_alone = 8;
    CHECK(plan_k3(k3_in(300, false, true), k).waves == 8);
    CHECK(plan_k3(k3_in(300, false, false), k).waves == 4);
    k.k3_waves_shared = 16;
    CHECK(plan_k3(k3_in(300, false, false), k).waves == 16);
    k.k3_waves_shared = 8;
    CHECK(plan_k3(k3_in(300, false, false), k).waves == 8);
    k.k3_waves_alone = 5;  // anything else: 8
    CHECK(plan_k3(k3_in(300, false, true), k).waves == 8);
    k.k3_waves_alone = 4;
    CHECK(plan_k3(k3_in(300, false, true), k).waves == 4);
  }
  // plain: the 513 .. 1 024 launch, big credit 0 / 1, SFMLOC_K3_BIG 0 / 1 / 2
  for (int knob = 0; knob <= 2; ++knob)
    for (int credit = 0; credit <= 1; ++credit)
      for (int alone = 0; alone <= 1; ++alone) {
        Knobs k;
        k.k3_big = knob;
        K3In in = k3_in(300, false, alone != 0);
        in.big_credit = credit;
        static const bool expect_big[3][2] = {{false, false}, {false, true}, {true, true}};  // [knob][credit]
        const bool big = expect_big[knob][credit];
        const K3Plan p = plan_k3(in, k);
        CHECK(!p.wide && p.max_m == 512 && p.big == big && p.skip_le == (big ? 1024 : 512));
        if (big) CHECK(p.big_waves == (alone ? 8 : 4));
        in.n_sel = 100;  // wide: its one launch holds those views already
        CHECK(!plan_k3(in, k).big && plan_k3(in, k).skip_le == 1024);
      }
}

// ---------------------------------------------------------------------------------------------------------------------
static K5In k5_in(uint32_t query_n, int small_credit, bool gang, bool busy) {
  K5In in;
  in.query_n = query_n;
  in.small_credit = small_credit;
  in.gang = gang;
  in.others_busy = busy;
  return in;
}

static void test_k5() {
  const Knobs d;
  // the small form: at most 512 features, or 8 small queries in a row
  CHECK(plan_k5_query(k5_in(512, 0, false, false), d).small);
  CHECK(!plan_k5_query(k5_in(513, 0, false, false), d).small);
  CHECK(!plan_k5_query(k5_in(513, 7, false, false), d).small);
  CHECK(plan_k5_query(k5_in(513, 8, false, false), d).small);
  CHECK(plan_k5_query(k5_in(2000, 64, false, false), d).small);
  {
    Knobs k;
    k.p3p_small = 0;
    CHECK(!plan_k5_query(k5_in(100, 64, false, false), k).small);
    k.p3p_small = 2;
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).small);
  }
  CHECK(!k5_small_refuted(512));
  CHECK(k5_small_refuted(513));
  // rounds and batches
  {
    K5QueryPlan p = plan_k5_query(k5_in(2000, 0, false, false), d);
    CHECK(p.first_rounds == 9 && p.later_rounds == 6 && kP3pFirstBatch == 64 && kP3pLaterBatch == 256);
    CHECK(p.adapt_quarters == 12 && p.adapt_floor == 64);
    p = plan_k5_query(k5_in(2000, 0, true, false), d);
    CHECK(p.first_rounds == 12 && p.later_rounds == 6);
    Knobs k;
    k.p3p_rounds = 20;
    CHECK(plan_k5_query(k5_in(2000, 0, true, false), k).first_rounds == 20);
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).first_rounds == 20);
    k.p3p_rounds = 3;
    CHECK(plan_k5_query(k5_in(2000, 0, true, false), k).first_rounds == 12);
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).first_rounds == 3);
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).later_rounds == 6);
    k.p3p_adapt_quarters = 8;
    k.p3p_adapt_floor = 32;
    p = plan_k5_query(k5_in(2000, 0, false, false), k);
    CHECK(p.adapt_quarters == 8 && p.adapt_floor == 32);
  }
  // adaptive batches: from the load, or the knob
  {
    Knobs k;
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).adaptive_batch == 0);
    CHECK(plan_k5_query(k5_in(2000, 0, false, true), k).adaptive_batch == 1);
    k.p3p_adaptive = 0;
    CHECK(plan_k5_query(k5_in(2000, 0, false, true), k).adaptive_batch == 0);
    k.p3p_adaptive = 1;
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).adaptive_batch == 1);
  }
  // hypotheses prepared ahead: knob unset / 0 / 1 / 2, gang or not, shared or not; never for six points
  {
    static const struct { int knob; bool gang, busy; int expect; } t[] = {
        {-1, false, false, 0}, {-1, false, true, 0}, {-1, true, false, 0}, {-1, true, true, 1},
        {0, false, false, 0},  {0, false, true, 0},  {0, true, false, 0},  {0, true, true, 0},
        {1, false, false, 0},  {1, false, true, 1},  {1, true, false, 0},  {1, true, true, 1},
        {2, false, false, 1},  {2, false, true, 1},  {2, true, false, 1},  {2, true, true, 1},
    };
    for (const auto &e : t) {
      Knobs k;
      k.p3p_prep_ahead = e.knob;
      K5In in = k5_in(2000, 0, e.gang, e.busy);
      CHECK(plan_k5_query(in, k).prep_ahead == e.expect);
      in.uncal = true;
      CHECK(plan_k5_query(in, k).prep_ahead == 0);
    }
    Knobs k;
    k.p3p_adaptive = 1;  // the adaptive rule by knob counts as shared
    k.p3p_prep_ahead = 1;
    CHECK(plan_k5_query(k5_in(2000, 0, false, false), k).prep_ahead == 1);
    k.p3p_adaptive = 0;
    CHECK(plan_k5_query(k5_in(2000, 0, true, true), k).prep_ahead == 0);
  }
  // a round: wide above 512 features while the wide credit lasts, clamped to 128 hypotheses, four workgroups each
  {
    K5In in;
    in.query_n = 513;
    in.wide_credit = 1;
    K5RoundPlan p = plan_k5_round(in, 256, d);
    CHECK(!p.six_point && p.form == K5Form::kWide && p.batch == 128 && p.grid == 512);
    p = plan_k5_round(in, 64, d);
    CHECK(p.form == K5Form::kWide && p.batch == 64 && p.grid == 256);
    in.small = true;  // wide wins over a small prediction
    CHECK(plan_k5_round(in, 256, d).form == K5Form::kWide);
    in.wide_credit = 0;
    p = plan_k5_round(in, 256, d);
    CHECK(p.form == K5Form::kSmall && p.batch == 256 && p.grid == 256);
    in.small = false;
    p = plan_k5_round(in, 256, d);
    CHECK(p.form == K5Form::kPlain && p.batch == 256 && p.grid == 256);
    CHECK(plan_k5_round(in, 64, d).grid == 64);
    in.query_n = 512;
    in.wide_credit = 64;
    CHECK(plan_k5_round(in, 256, d).form == K5Form::kPlain);
    Knobs k;
    k.p3p_wide_always = true;
    p = plan_k5_round(in, 256, k);
    CHECK(p.form == K5Form::kWide && p.batch == 128 && p.grid == 512);
    // six points: never wide
    in.query_n = 2000;
    in.uncal = true;
    p = plan_k5_round(in, 256, k);
    CHECK(p.six_point && p.form == K5Form::kPlain && p.batch == 256 && p.grid == 256);
    in.small = true;
    p = plan_k5_round(in, 256, d);
    CHECK(p.six_point && p.form == K5Form::kSmall && p.batch == 256 && p.grid == 256);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static int ld(const std::atomic<int> &a) { return a.load(std::memory_order_relaxed); }

static void test_credits() {
  {
    FormCredits c;
    CHECK(ld(c.p3p_wide) == 0 && ld(c.p3p_small) == 0 && ld(c.k3_huge) == 0 && ld(c.k3_big) == 0);
    c.note_p3p_set(100);
    CHECK(ld(c.p3p_wide) == 0 && ld(c.p3p_small) == 1);
    c.note_p3p_set(600);
    CHECK(ld(c.p3p_wide) == 64 && ld(c.p3p_small) == 0);
    for (int i = 1; i <= 70; ++i) {
      c.note_p3p_set(100);
      CHECK(ld(c.p3p_wide) == (i < 64 ? 64 - i : 0));
      CHECK(ld(c.p3p_small) == (i < 64 ? i : 64));
    }
    CHECK(ld(c.p3p_wide) == 0 && ld(c.p3p_small) == 64);
    c.note_p3p_set(512);
    CHECK(ld(c.p3p_wide) == 0 && ld(c.p3p_small) == 64);
    c.note_p3p_set(513);
    CHECK(ld(c.p3p_wide) == 64 && ld(c.p3p_small) == 0);
    CHECK(ld(c.k3_huge) == 0 && ld(c.k3_big) == 0);
  }
  {
    FormCredits c;
    c.note_k3_largest_view(400);
    CHECK(ld(c.k3_huge) == 0 && ld(c.k3_big) == 0);
    c.note_k3_largest_view(700);
    CHECK(ld(c.k3_huge) == 0 && ld(c.k3_big) == 64);
    c.note_k3_largest_view(1500);
    CHECK(ld(c.k3_huge) == 64 && ld(c.k3_big) == 0);
    c.note_k3_largest_view(3000);
    CHECK(ld(c.k3_huge) == 63 && ld(c.k3_big) == 0);
    for (int i = 1; i <= 70; ++i) {
      c.note_k3_largest_view(400);
      CHECK(ld(c.k3_huge) == (i < 63 ? 63 - i : 0));
      CHECK(ld(c.k3_big) == 0);
    }
    CHECK(ld(c.p3p_wide) == 0 && ld(c.p3p_small) == 0);
  }
  {  // the big credit counts down too, and the edges of the three ranges
    FormCredits c;
    c.note_k3_largest_view(513);
    CHECK(ld(c.k3_big) == 64 && ld(c.k3_huge) == 0);
    for (int i = 1; i <= 70; ++i) {
      c.note_k3_largest_view(512);
      CHECK(ld(c.k3_big) == (i < 64 ? 64 - i : 0));
    }
    c.note_k3_largest_view(1024);
    CHECK(ld(c.k3_big) == 64 && ld(c.k3_huge) == 0);
    c.note_k3_largest_view(1025);
    CHECK(ld(c.k3_big) == 0 && ld(c.k3_huge) == 64);
    c.note_k3_largest_view(2049);
    CHECK(ld(c.k3_big) == 0 && ld(c.k3_huge) == 63);
    c.note_k3_largest_view(2048);
    CHECK(ld(c.k3_big) == 0 && ld(c.k3_huge) == 64);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
static void test_knobs_from_the_environment() {
  static const char *const names[] = {
      "SFMLOC_K1_QSPLIT",    "SFMLOC_K1_SCREEN_BATCH",    "SFMLOC_K1_SCREEN_HEAD",  "SFMLOC_K3_WIDE",
      "SFMLOC_K3_WIDE_2048", "SFMLOC_K3_BIG",             "SFMLOC_K3_WAVES_ALONE",  "SFMLOC_K3_WAVES_SHARED",
      "SFMLOC_P3P_SMALL",    "SFMLOC_P3P_PREP_AHEAD",     "SFMLOC_P3P_ADAPTIVE",    "SFMLOC_P3P_ADAPT_QUARTERS",
      "SFMLOC_P3P_ADAPT_FLOOR", "SFMLOC_P3P_ROUNDS",      "SFMLOC_P3P_WIDE_ALONE",
  };
  for (const char *n : names) unsetenv(n);
  Knobs k = read_knobs();
  CHECK(k.k1_qsplit == 0 && k.k1_screen_batch == 0 && k.k1_screen_head == 64);
  CHECK(k.k3_wide == 1 && k.k3_wide_2048 == 1 && k.k3_big == 1 && k.k3_waves_alone == 16 && k.k3_waves_shared == 4);
  CHECK(k.p3p_small == 1 && k.p3p_prep_ahead == -1 && k.p3p_adaptive == -1 && k.p3p_adapt_quarters == 12);
  CHECK(k.p3p_adapt_floor == 64 && k.p3p_rounds == 9 && !k.p3p_wide_always);
  static const struct { const char *v; int rounds; uint32_t head; bool wide; } t[] = {
      {"0", 9, 64, false},  {"1", 1, 64, false},    {"2", 2, 2, true},     {"64", 64, 64, false},
      {"65", 9, 65, false}, {"256", 9, 256, false}, {"257", 9, 64, false},
  };
  for (const auto &e : t) {
    setenv("SFMLOC_P3P_ROUNDS", e.v, 1);
    setenv("SFMLOC_K1_SCREEN_HEAD", e.v, 1);
    setenv("SFMLOC_P3P_WIDE_ALONE", e.v, 1);
    k = read_knobs();
    CHECK(k.p3p_rounds == e.rounds && k.k1_screen_head == e.head && k.p3p_wide_always == e.wide);
  }
  for (const char *n : names) setenv(n, "3", 1);
  k = read_knobs();
  CHECK(k.k1_qsplit == 3 && k.k1_screen_batch == 3 && k.k1_screen_head == 3 && k.k3_wide == 3 && k.k3_wide_2048 == 3);
  CHECK(k.k3_big == 3 && k.k3_waves_alone == 3 && k.k3_waves_shared == 3 && k.p3p_small == 3 && k.p3p_prep_ahead == 3);
  CHECK(k.p3p_adaptive == 3 && k.p3p_adapt_quarters == 3 && k.p3p_adapt_floor == 3 && k.p3p_rounds == 3);
  CHECK(!k.p3p_wide_always);
  for (const char *n : names) unsetenv(n);
}

int main() {
  test_k1();
  test_k3();
  test_k5();
  test_credits();
  test_knobs_from_the_environment();
  if (g_failed) {
    printf("%d checks failed\n", g_failed);
    return 1;
  }
  printf("OK\n");
  return 0;
}
