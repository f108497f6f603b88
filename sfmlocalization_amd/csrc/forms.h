// Which text of K1 / K3 / K5 a query's stages run as ("Kernel forms: one table"), decided on the host:
// the size thresholds the policy shares with the kernels, the environment's knobs, the map's credits and, per stage, a
// pure function from what the host knows to a plan of enums and integers.  The launch functions (hamming.hip,
// acransac.hip, capi.hip) fill the input, call the plan and launch what it says.  Host only: no HIP header, plain
// C++17 -- tests/cpp/forms_plan.cpp walks the boundaries on the CPU.  Every form gives the same bits; the plans only
// choose cost.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <atomic>

namespace sfmloc {

// Thresholds.  K1
constexpr int kScreenWaves = 8;       // waves per workgroup of every screened scan, one bank block each
constexpr int kScreenNW = 10;         // dwords of the screening prefix: the "some lane still below its threshold" vote fires
                                      // for ~3 % of the pairs on the bench data at ratio 0.6 (9 is past the cliff: half the
                                      // lanes pass; profiles/r01_k1_screen_sweep.txt)
constexpr uint32_t kScreenHead = 64;  // measured: 64 and 128 within 1 %, 256+ slower (profiles/r01_k1_screen_sweep.txt)
// (below ~12 heads' worth of query rows the exact head and the second launch eat the saving:
// profiles/r01_k1_screen_on_akaze_descriptors.jsonl)
constexpr uint32_t kScreenMinNq = 12 * kScreenHead;
constexpr uint32_t kK1SliceBlocksPerCu = 32;    // below this many work blocks per compute unit a scan may be sliced / the
                                                // exact form takes 4-wave workgroups
constexpr uint32_t kK1BatchedBlocksPerCu = 16;  // fewer than four waves per SIMD: the batched tail pays

// K3
constexpr int kF2MaxM = 512;       // putative matches per view of the register form (one wave sorts one model's residuals)
constexpr int kF2BigM = 1024;      // ... of its 16-residuals-per-lane instance
constexpr int kF2HugeM = 2048;     // ... of its 32-residuals-per-lane instance (wide only)
constexpr int kFMaxM = 2048;       // putative matches per view the block-wide LDS sort holds (k_fmatrix_filter)
constexpr int kF2Batch = 32;       // uniform iterations solved speculatively per batch
constexpr int kK3WideViews = 256;  // view lists the wide form takes (its result slots: 2 MB per context)
constexpr int kK3WideWaves = 4;    // waves per workgroup of the wide form's kF2BigM instance unless the knob says otherwise

// K5
constexpr int kP3pSmallN = 512;  // correspondences the small form of a round holds
// result slots of a round: one per hypothesis (at most kP3pBatchMax), or (wide launches) four, one per model.  A slot's
// inlier list is kP3pMaxN ints: 8 MB per context (16 MB while wide rounds could be 256 hypotheses: ADVICE r03)
constexpr int kP3pSlots = 512;
// the first round's size, alone or while the GPU is shared: after the geometric filter the first hypothesis is nearly
// always the one that switches sampling to its inliers, and everything behind it is thrown away
constexpr int kP3pFirstBatch = 64;
// hypotheses a launch of a query's rounds carries after the first: as many rounds as with 512 (an improvement of the model
// comes early in a round or not at all), 3-5 % more queries per second because fewer speculative hypotheses are evaluated
// for nothing
constexpr int kP3pLaterBatch = 256;
// wide rounds are nominally 128 hypotheses, not 256: on large sets most rounds evaluate 16 .. 64 (p3p_next_batch_limit)
// and every workgroup of the 4 x batch launched has to be dispatched with its LDS and registers even to find that it has
// nothing to do: image-in frames 0.86 -> 0.71 ms of PnP alone, 1 229 -> 1 302 images/s, profiles/r04_k5_forms.txt.
// (A wide launch sized for fewer hypotheses, each workgroup taking several in turn, cost the small form's text 10 % of a
// headline round; not kept, same profile.)
constexpr int kP3pWideBatch = 128;
static_assert(4 * kP3pWideBatch <= kP3pSlots, "a wide round's results are four slots per hypothesis");
constexpr int kP3pLargeBatch = 64;  // hypotheses per round beyond kP3pMaxN correspondences (global-memory sort segments)
constexpr int kP3pLaterRounds = 6;  // rounds a later call queues (ctx_resection_wait)
// (in a gang session a surplus round costs a fraction of a launch, and a member that needs more than were queued gets
// them alone on the gang's stream: three more up front)
constexpr int kP3pGangRounds = 12;
constexpr int kCreditMax = 64;      // a credit just refreshed; it then counts finished queries
constexpr int kP3pSmallAfter = 8;   // small queries in a row after which the next one's rounds are queued small

// Knobs: the SFMLOC_K1_* / SFMLOC_K3_* / SFMLOC_P3P_* switches of the environment (INTEGRATION.md lists them)
struct Knobs {
  int k1_qsplit = 0;                  // SFMLOC_K1_QSPLIT 1..16: the slice count of every screened scan
  int k1_screen_batch = 0;            // SFMLOC_K1_SCREEN_BATCH 4 / 1: the batched-tail / the lean form, whatever the load
  uint32_t k1_screen_head = kScreenHead;  // SFMLOC_K1_SCREEN_HEAD 2..256: exact head rows
  int k3_wide = 1;                    // SFMLOC_K3_WIDE 0 never, 2 always (tests, campaigns)
  int k3_wide_2048 = 1;               // SFMLOC_K3_WIDE_2048 0 never, 2 always
  int k3_big = 1;                     // SFMLOC_K3_BIG 0 never, 2 always
  int k3_wide_waves = kK3WideWaves;   // SFMLOC_K3_WIDE_WAVES 4 / 8: waves per workgroup of the wide 1 024-match instance
  int k3_waves_alone = 16;            // SFMLOC_K3_WAVES_ALONE / _SHARED: 16, 4, anything else 8
  int k3_waves_shared = 4;
  int p3p_small = 1;                  // SFMLOC_P3P_SMALL 0 never, 2 always
  int p3p_prep_ahead = -1;            // SFMLOC_P3P_PREP_AHEAD 0 never, 1 whenever the GPU is shared, 2 always
  int p3p_adaptive = -1;              // SFMLOC_P3P_ADAPTIVE 0 / 1 overrides the shared-GPU rule (measurements)
  int p3p_adapt_quarters = 12;        // SFMLOC_P3P_ADAPT_QUARTERS, _FLOOR: next batch = max(floor, quarters/4 * iterations
  int p3p_adapt_floor = 64;           // since the switch)
  int p3p_rounds = 9;                 // SFMLOC_P3P_ROUNDS 1..64: rounds queued by a query's first call
  bool p3p_wide_always = false;       // SFMLOC_P3P_WIDE_ALONE=2 (tools/run_fuzz.sh FORMS=wide)
};

inline Knobs read_knobs() {
  const auto env_int = [](const char *name, int dflt) {
    const char *e = getenv(name);
    return e ? atoi(e) : dflt;
  };
  Knobs k;
  k.k1_qsplit = env_int("SFMLOC_K1_QSPLIT", 0);
  k.k1_screen_batch = env_int("SFMLOC_K1_SCREEN_BATCH", 0);
  const int head = env_int("SFMLOC_K1_SCREEN_HEAD", (int)kScreenHead);
  k.k1_screen_head = (head >= 2 && head <= 4 * (int)kScreenHead) ? (uint32_t)head : kScreenHead;
  k.k3_wide = env_int("SFMLOC_K3_WIDE", 1);
  k.k3_wide_2048 = env_int("SFMLOC_K3_WIDE_2048", 1);
  k.k3_big = env_int("SFMLOC_K3_BIG", 1);
  const int wide_waves = env_int("SFMLOC_K3_WIDE_WAVES", kK3WideWaves);
  k.k3_wide_waves = (wide_waves == 4 || wide_waves == 8) ? wide_waves : kK3WideWaves;
  k.k3_waves_alone = env_int("SFMLOC_K3_WAVES_ALONE", 16);
  k.k3_waves_shared = env_int("SFMLOC_K3_WAVES_SHARED", 4);
  k.p3p_small = env_int("SFMLOC_P3P_SMALL", 1);
  k.p3p_prep_ahead = env_int("SFMLOC_P3P_PREP_AHEAD", -1);
  k.p3p_adaptive = env_int("SFMLOC_P3P_ADAPTIVE", -1);
  k.p3p_adapt_quarters = env_int("SFMLOC_P3P_ADAPT_QUARTERS", 12);
  k.p3p_adapt_floor = env_int("SFMLOC_P3P_ADAPT_FLOOR", 64);
  const int rounds = env_int("SFMLOC_P3P_ROUNDS", 9);
  k.p3p_rounds = (rounds >= 1 && rounds <= 64) ? rounds : 9;
  k.p3p_wide_always = env_int("SFMLOC_P3P_WIDE_ALONE", 0) == 2;
  return k;
}
inline const Knobs &knobs() {  // read once per process
  static const Knobs k = read_knobs();
  return k;
}

// Credits: what a map remembers of its finished queries' sizes.  The host queues a query's launches before it knows
// the sizes they will meet, so it predicts them from the last queries; the kernels correct a wrong guess (a form that
// does not hold a view or a set leaves it to the next one), so a stale value costs time, never bits -- hence relaxed.
struct FormCredits {
  std::atomic<int> p3p_wide{0};   // > 0 while recent queries had more than kP3pSmallN 2D-3D correspondences
  std::atomic<int> p3p_small{0};  // finished queries in a row whose set had at most kP3pSmallN
  std::atomic<int> k3_huge{0};    // > 0 while recent queries' largest view had kF2BigM + 1 .. kF2HugeM putative matches
  std::atomic<int> k3_big{0};     // ... kF2MaxM + 1 .. kF2BigM

  static void count_down(std::atomic<int> &c) {
    if (c.load(std::memory_order_relaxed) > 0) c.fetch_sub(1, std::memory_order_relaxed);
  }
  // a query's resection is done: its number of correspondences
  void note_p3p_set(int n) {
    if (n > kP3pSmallN) {
      p3p_wide.store(kCreditMax, std::memory_order_relaxed);
      p3p_small.store(0, std::memory_order_relaxed);
    } else {
      count_down(p3p_wide);
      if (p3p_small.load(std::memory_order_relaxed) < kCreditMax) p3p_small.fetch_add(1, std::memory_order_relaxed);
    }
  }
  // a query has ended: the putative matches of its largest view.  (A query with a view beyond the instance it would
  // refresh gains nothing from that instance: the launches run one after the other, and the block-wide form of its
  // largest view is what it waits for either way -- measured on the dense lab frames, +0.2 ms.)
  void note_k3_largest_view(uint32_t v) {
    if (v > (uint32_t)kF2BigM && v <= (uint32_t)kF2HugeM) k3_huge.store(kCreditMax, std::memory_order_relaxed);
    else count_down(k3_huge);
    if (v > (uint32_t)kF2BigM) k3_big.store(0, std::memory_order_relaxed);
    else if (v > (uint32_t)kF2MaxM) k3_big.store(kCreditMax, std::memory_order_relaxed);
    else count_down(k3_big);
  }
};

// K1: the Hamming scan
struct K1In {
  uint32_t nq = 0, n_work_blocks = 0, split = 1;  // the query's descriptors, the scan's bank blocks, the caller's query splits
  int n_cu = 256;
  bool use_list = false;  // the blocks come from a view list (a shortlist), not the whole bank
  bool exact_rows = false, k1_mfma = true;  // params
  bool may_slice = true;  // Ctx::k1_may_slice: no other context of the map had work queued when the query began
};
enum class K1Form {
  kExact,        // k_hamming_top2<1, exact_waves>
  kLean,         // k_hamming_screen<8, 10, 1>: the full-bank scan, the roofline kernel
  kBatchedTail,  // k_hamming_screen<8, 10, 4>
  kMfma,         // k_hamming_screen_mfma
  kShortlist,    // k_hamming_screen_shortlist: the lean text on a view list
};
struct K1Plan {
  K1Form form = K1Form::kExact;
  int exact_waves = 0;             // kExact: waves per workgroup
  uint32_t slices = 1, head = 0;   // screened: query slices (gridDim.y), exact head rows
  bool shared_head = false;        // one exact pass over the head (k_hamming_top2) seeds every slice
  bool clear_flagmask = false;     // the slices OR into the flag mask: it must be zero before them
  uint64_t lane_ops_per_row = 0;  // sfmloc_kernel_stats::hamming_lane_ops per bank row scanned, the deterministic part
  int finish_ops = 0;          // lane-ops per finished pair (counted on the device, Ctx::k1_finish_ops)
  bool screened() const { return form != K1Form::kExact; }
};

// Query slices for a short block list: aim at 8 waves per SIMD (3 200 blocks in one slice leave the fullest SIMDs 4 waves
// and the average 3.1: 0.39 ms; four slices: 0.33 ms).  The head is shared, so a slice costs no head of its own; a
// workgroup's fixed costs -- its bank rows, its query slice into LDS, two barriers -- stop amortising below ~500 query
// rows per slice (profiles/r02_k1_qsplit_sweep.txt: a shortlisted query takes 0.95 / 0.93 / 0.89 / 1.02 / 1.29 ms with
// 1 / 2 / 4 / 8 / 16 slices).  HOW MANY slices is chosen for the launch's last generation of workgroups.  A lone query's
// 3 150 blocks in four slices are 1 576 workgroups for 768 places (three of the batched form per compute unit): two full
// generations and 40 stragglers that start when the second ends and run a third of a generation alone -- 48 of the scan's
// 268 us.  With s slices a workgroup takes 1 / s of the time and the launch G(s) generations, the last one -- a fraction r
// of the places -- about 0.45 + 0.55 r of a full one (fewer waves per SIMD run faster, not proportionally); each slice
// costs its workgroups' fixed part (~1 %).  Measured on the headline's lone query, putMatch with 4 / 5 / 7 / 8 / 10 / 14
// slices: 0.323 / 0.301 / 0.291 / 0.300 / 0.296 / 0.294 ms.
inline uint32_t k1_slices(const K1In &in, const Knobs &k) {
  const uint32_t head = k.k1_screen_head;
  uint32_t slices = 1;
  if ((uint64_t)in.n_work_blocks < (uint64_t)kK1SliceBlocksPerCu * (uint64_t)in.n_cu) {
    const uint32_t wg_per_slice = (in.n_work_blocks + kScreenWaves - 1) / kScreenWaves;
    // (68 VGPRs, three per compute unit.  plan_k1 also asks for the batched-tail knob before it takes that form: the two
    // disagree under SFMLOC_K1_SCREEN_BATCH; repairing it changes launches and is a change of its own)
    const bool batched = in.n_work_blocks < kK1BatchedBlocksPerCu * (uint32_t)in.n_cu;
    const double places = (double)((batched ? 3 : 4) * in.n_cu);
    double best = 1e30;
    for (uint32_t s = 1; s <= 8; ++s) {
      if (s > 1 && (in.nq <= head || (in.nq - head) / s < 3 * head)) break;  // (a slice keeps at least three heads of query rows)
      const double g = (double)wg_per_slice * s / places;
      const double full = floor(g), r = g - full;
      const double cost = (full + (r > 0.0 ? 0.45 + 0.55 * r : 0.0)) / s * (1.0 + 0.012 * s);
      if (cost < best) {
        best = cost;
        slices = s;
      }
    }
  }
  if (!in.may_slice) slices = 1;  // other queries are queued on the GPU: their scans fill it, slices only add work
  if (k.k1_qsplit >= 1 && k.k1_qsplit <= 16) slices = (uint32_t)k.k1_qsplit;
  return slices;
}

inline K1Plan plan_k1(const K1In &in, const Knobs &k) {
  K1Plan p;
  if (in.split != 1 || in.exact_rows || in.nq < kScreenMinNq) {
    // Measured on MI355X (profiles/r01_valu_rates.jsonl, profiles/r01_k1_lab.txt): v_xor_b32 issues at 2 cycles per
    // wave64, v_bcnt_u32_b32 / v_med3 / v_lshl_or at ~4, and one wave alone gets an instruction only every ~4.8 cycles,
    // so the loop reaches the VALU issue rate of its instruction mix only with >= 4 waves per SIMD.  LDS vs scalar-cache
    // query reads, register prefetch of the query row and split popcount chains all time within 5 % of each other: the
    // loop is VALU-issue bound.  Geometry: one bank block per wave (42 VGPRs), 8-wave workgroups, 32 KiB LDS slices -> 4
    // workgroups = 32 waves per CU; a scan too short to fill that takes 4-wave workgroups
    // (profiles/r01_k1_geometry_sweep.txt).
    const uint64_t wave_blocks = (uint64_t)in.n_work_blocks * in.split;
    p.exact_waves = wave_blocks >= (uint64_t)in.n_cu * kK1SliceBlocksPerCu ? 8 : 4;
    p.lane_ops_per_row = (uint64_t)in.nq * 35;
    return p;
  }
  p.head = k.k1_screen_head;
  p.slices = k1_slices(in, k);
  p.shared_head = p.clear_flagmask = p.slices > 1;
  // (the batched-tail form has 68 VGPRs against 48: while the GPU is shared the lean one leaves the other queries'
  // latency-bound stages more of the register file, +1.6 % queries/s; alone the two are equal)
  const bool batched_tail = k.k1_screen_batch ? k.k1_screen_batch == 4 : in.may_slice;
  if (batched_tail && in.n_work_blocks < kK1BatchedBlocksPerCu * (uint32_t)in.n_cu) p.form = K1Form::kBatchedTail;
  else if (in.use_list && p.slices == 1 && in.k1_mfma) p.form = K1Form::kMfma;  // a shortlist while the GPU is shared, a long list
  else if (in.use_list) p.form = K1Form::kShortlist;  // params.k1_mfma = 0, or a sliced scan of a view list
  else p.form = K1Form::kLean;
  // executed VALU lane-ops, deterministic part (the finished pairs are counted on the device)
  if (p.form == K1Form::kMfma) {
    // what the matrix-core form issues on the VALU (the MFMA work itself is not lane-ops): per 64 bank rows x 32 query
    // rows 8 x 7 expansion + 16 v_max3 instructions = 2.25 lane-ops per pair; the head's value-only top-2 adds 64
    // instructions per such step (2 per pair); expanding a wave's bank rows once is 112 instructions (112 per row)
    const uint64_t nq32 = ((uint64_t)in.nq + 31) & ~31ull, head32 = ((uint64_t)p.head + 31) & ~31ull;
    p.lane_ops_per_row = nq32 * 9 / 4 + (head32 < nq32 ? head32 : nq32) * 2 + 112;
    p.finish_ops = 0;
  } else {
    // exact head 35 per pair (a sliced scan shares ONE head), screened tail 2 NW + 1, 2 (16 - NW) + 5 per finished pair
    p.lane_ops_per_row = (uint64_t)p.head * 35 + (uint64_t)(in.nq - p.head) * (2 * kScreenNW + 1);
    p.finish_ops = 2 * (16 - kScreenNW) + 5;
  }
  return p;
}

// K3: the fundamental-matrix filter
struct K3In {
  uint32_t n_sel = 0;           // views in the list
  int ransac_round = 0;         // params.ransac_round
  bool gang = false, alone = true;  // the context is recording for a gang session; Ctx::k1_may_slice
  bool merge_deferred = false;  // K2 was left to this stage (QueryPass)
  int huge_credit = 0, big_credit = 0;
};
enum class K3Merge { kDone, kFolded, kInFront };  // K2: ran already / inside k_fmatrix_fast / a launch of its own first
struct K3Plan {
  bool wide = false;  // one workgroup per iteration of a view's first batch (fmatrix_fast.body.inc)
  int wide_b0 = 0;    // ... that many
  int wide_waves = 0;  // wide: waves per workgroup (the view's tail runs on them); the kF2HugeM instance has four
  int max_m = kF2MaxM;  // the instance of the first k_fmatrix_fast launch
  K3Merge k2 = K3Merge::kDone;
  int waves = 4;      // plain: waves per view (F2SharedT)
  bool big = false;   // plain: the kF2BigM instance follows for views of kF2MaxM + 1 .. kF2BigM matches
  int big_waves = 0;
  int skip_le = kF2MaxM;  // k_fmatrix_filter leaves views of at most that many matches alone: a launch above took them
};

inline K3Plan plan_k3(const K3In &in, const Knobs &k) {
  K3Plan p;
  // The wide form for a short view list, whether or not other contexts have work queued: its kF2BigM instance takes every
  // view the register forms hold, in one launch, K2 included.  (Until the matrix-core scan it was a lone query's form:
  // the popcount scan filled the chip and K3's registers were the scans'.  Since then the chip is mostly idle under load
  // and a query's time is the length of its chain, DESIGN.md 4 "Where the time goes after the matrix-core scan".)  Gang
  // sessions keep the plain form.
  const int n_uniform = in.ransac_round - in.ransac_round / 10;
  p.wide_b0 = n_uniform < kF2Batch ? n_uniform : kF2Batch;
  p.wide = p.wide_b0 >= 2 && in.n_sel <= (uint32_t)kK3WideViews && (k.k3_wide == 2 || (k.k3_wide == 1 && !in.gang));
  // (views of kF2BigM + 1 .. kF2HugeM matches -- 32 residuals per lane in the register sort, one workgroup per compute
  // unit -- only while the map's queries have had such views lately: k_fmatrix_filter's block-wide sort took 0.6 of a
  // lone 1080p frame's 0.95 ms in this stage)
  const bool huge = p.wide && (k.k3_wide_2048 == 2 || (k.k3_wide_2048 == 1 && in.huge_credit > 0));
  // k_fmatrix_fast runs on every selected view, whatever its size, so it can build the view's lists itself; in the wide
  // form every workgroup of a view does.  The kF2HugeM instance keeps K2 as a launch of its own: its workgroups are one
  // per compute unit, the views of the frames that bring it have thousands of rows and hundreds of flagged ones, and ~23
  // workgroups per view each reading the view's flag words or repeating its merge cost a lone 1080p frame 0.12 ms here
  if (in.merge_deferred) p.k2 = huge ? K3Merge::kInFront : K3Merge::kFolded;
  if (p.wide) {
    p.max_m = p.skip_le = huge ? kF2HugeM : kF2BigM;
    // (four waves: at 229 VGPRs an eight-wave workgroup is a compute unit's whole register file, a headline query's ~460
    // first-batch workgroups then need two generations of the chip and the other queries' kernels wait for whole compute
    // units -- 4 540 -> 3 940 queries/s -- while the tail it would widen is at most the two reserve iterations at the
    // default budget: profiles/k3tail_split_after.txt.  Eight stay reachable for larger budgets and the tests.)
    p.wide_waves = (!huge && k.k3_wide_waves == 8) ? 8 : 4;
    return p;
  }
  // 16 waves per view for a query alone on the GPU, 4 when other contexts have work queued
  const int waves = in.alone ? k.k3_waves_alone : k.k3_waves_shared;
  p.waves = (waves == 16 || waves == 4) ? waves : 8;
  // views with kF2MaxM + 1 .. kF2BigM putative matches (a query that nearly duplicates a map frame): the same kernel
  // with 16 residuals per lane -- while the map's queries have had such views lately: a launch whose 100 workgroups all
  // leave at once still costs a launch
  p.big = k.k3_big == 2 || (k.k3_big == 1 && in.big_credit > 0);
  if (p.big) {
    p.big_waves = in.alone ? 8 : 4;
    p.skip_le = kF2BigM;
  }
  return p;
}

// K5: the resection's AC-RANSAC rounds
struct K5In {
  uint32_t query_n = 0;      // the query's features: its set has at most one correspondence each
  bool uncal = false;        // six-point resection
  bool gang = false, others_busy = false;  // the context is recording for a gang session; Ctx::others_busy
  bool small = false;        // a round: K5QueryPlan::small, not refuted since (Ctx::p3p_small)
  int small_credit = 0, wide_credit = 0;
};
struct K5QueryPlan {
  // The small form holds sets of at most kP3pSmallN correspondences in a fraction of the registers: a prediction from
  // the map's last queries -- or a certainty, when the query has no more features than that; k5_small_refuted corrects it
  bool small = false;
  // typically 6-8 rounds end the stage (one per improvement of the model); rounds enqueued past the end return at once
  // but still cost two launches each, so the first call queues 9 and later calls add more if needed
  int first_rounds = 0, later_rounds = kP3pLaterRounds;
  int adaptive_batch = 0;  // P3pArgs: trade rounds for fewer speculative hypotheses (p3p_next_batch_limit)
  int prep_ahead = 0;      // P3pArgs: the replaying workgroup solves the coming round's hypotheses
  int adapt_quarters = 0, adapt_floor = 0;
};

inline K5QueryPlan plan_k5_query(const K5In &in, const Knobs &k) {
  K5QueryPlan p;
  p.small = k.p3p_small == 2 ||
            (k.p3p_small == 1 && (in.query_n <= (uint32_t)kP3pSmallN || in.small_credit >= kP3pSmallAfter));
  p.first_rounds = in.gang ? (k.p3p_rounds > kP3pGangRounds ? k.p3p_rounds : kP3pGangRounds) : k.p3p_rounds;
  // a context that shares the GPU spends fewer speculative hypotheses per round
  p.adaptive_batch = k.p3p_adaptive >= 0 ? k.p3p_adaptive : (in.others_busy ? 1 : 0);
  // Hypotheses prepared ahead save issue cycles and cost the query's chain the 10-20 us the lone replaying workgroup
  // takes over them.  While the popcount scan filled the chip the cycles were what counted; since the matrix-core scan
  // the chip is mostly idle under load and the chain's length is what a query's time is made of: only a
  // gang session, whose launches carry up to 32 queries' rounds, still prepares ahead.
  p.prep_ahead = k.p3p_prep_ahead == 2 ||
                 (p.adaptive_batch && (k.p3p_prep_ahead == 1 || (k.p3p_prep_ahead < 0 && in.gang)));
  if (in.uncal) p.prep_ahead = 0;  // (the replay's hand-over solves P3P; k_resect6_prepare is the six-point kernel's)
  p.adapt_quarters = k.p3p_adapt_quarters;
  p.adapt_floor = k.p3p_adapt_floor;
  return p;
}

// the small rounds of a set that turned out larger than the form holds all returned at once: the full form from now on
inline bool k5_small_refuted(int set_n) { return set_n > kP3pSmallN; }

enum class K5Form {
  kSmall,  // k_p3p_round_small / k_resect6_round_small
  kPlain,  // k_p3p_round / k_resect6_round, one workgroup per hypothesis
  kWide,   // k_p3p_round, four workgroups per hypothesis, one model each (p3p_eval_hypothesis)
};
struct K5RoundPlan {
  bool six_point = false;  // k_resect6_prepare first, then the six-point round in `form`
  K5Form form = K5Form::kPlain;
  int batch = 0, grid = 0;  // hypotheses, workgroups
};

inline K5RoundPlan plan_k5_round(const K5In &in, int batch, const Knobs &k) {
  K5RoundPlan p;
  p.six_point = in.uncal;
  // Wide from kP3pSmallN + 1 features on -- a query may then have that many correspondences -- and only while queries of
  // this map HAVE had that many lately: the idle workgroups of a wide launch cost a small query ~15 us and 3 % of the
  // throughput, and the host cannot know the set's size when it queues the rounds.  Not for any query alone on the GPU:
  // with 4 x 256 workgroups the chip is NOT idle, four waves per SIMD share its f64 pipe and a headline round takes 47
  // us instead of 29 (profiles/r04_k5_forms.txt).  A six-point round has one model per hypothesis, nothing to spread.
  const bool wide = !in.uncal && ((in.query_n > (uint32_t)kP3pSmallN && in.wide_credit > 0) || k.p3p_wide_always);
  p.form = wide ? K5Form::kWide : in.small ? K5Form::kSmall : K5Form::kPlain;
  p.batch = wide && batch > kP3pWideBatch ? kP3pWideBatch : batch;
  p.grid = wide ? 4 * p.batch : p.batch;
  return p;
}

}  // namespace sfmloc
