// Internal declarations shared by the HIP translation units of libsfmloc_hip.so.
// Nothing here is part of the C ABI (include/sfmloc.h is).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <exception>
#include <new>
#include <stdio.h>
#include <stdlib.h>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "chain_device.h"
#include "devmem.h"
#include "forms.h"
#include "gang.h"
#include "launch.h"

namespace sfmloc {

void set_error(const char *fmt, ...);

// an integer switch of the environment (INTEGRATION.md lists them; the K1 / K3 / K5 ones are read in forms.h); callers keep
// the value in a function-local `static const`, so it is read once per process
inline int env_int(const char *name, int dflt) {
  const char *e = getenv(name);
  return e ? atoi(e) : dflt;
}

// (hip_code, the SFMLOC code of a failed HIP call: launch.h)
#define SFM_HIP(call)                                                                          \
  do {                                                                                         \
    hipError_t e_ = (call);                                                                    \
    if (e_ != hipSuccess) {                                                                    \
      ::sfmloc::set_error("%s:%d %s -> %s", __FILE__, __LINE__, #call, hipGetErrorString(e_)); \
      return ::sfmloc::hip_code(e_);                                                           \
    }                                                                                          \
  } while (0)

#define SFM_CHECK(cond, code, ...)     \
  do {                                 \
    if (!(cond)) {                     \
      ::sfmloc::set_error(__VA_ARGS__); \
      return (code);                   \
    }                                  \
  } while (0)

// a step that answers an SFMLOC code: on anything but SFMLOC_OK the function returns it (variadic only so that the
// commas of a template argument list need no parentheses)
#define SFM_RC(...)               \
  do {                            \
    const int rc_ = (__VA_ARGS__); \
    if (rc_) return rc_;          \
  } while (0)

// The shell of an entry point that hands out a fresh handle: `fill` fills a new host-side Handle and answers an SFMLOC
// code; *out is the handle on SFMLOC_OK and null otherwise, and no exception crosses the C ABI.  `name`: the entry
// point the texts speak for.
template <class Handle, class Opaque, class Fill>
inline int make_handle(const char *name, Opaque **out, Fill &&fill) {
  SFM_CHECK(out, SFMLOC_EINVAL, "%s: null argument", name);
  *out = nullptr;
  Handle *h = new (std::nothrow) Handle();
  SFM_CHECK(h, SFMLOC_ENOMEM, "out of host memory");
  int rc;
  try {
    rc = fill(h);
  } catch (const std::bad_alloc &) {
    set_error("%s: out of host memory", name);
    rc = SFMLOC_ENOMEM;
  } catch (const std::exception &e) {  // (host-side containers sized by the caller's counts: std::length_error)
    set_error("%s: %s", name, e.what());
    rc = SFMLOC_EINVAL;
  }
  if (rc) {
    delete h;
    return rc;
  }
  *out = reinterpret_cast<Opaque *>(h);
  return SFMLOC_OK;
}

// the caller's options, or the entry point's defaults where it passed none
template <class Options>
inline Options options_or(const Options *opt, void (*defaults)(Options *)) {
  Options o;
  if (opt) o = *opt;
  else defaults(&o);
  return o;
}

// ---------------------------------------------------------------------------
// HBM layout of the descriptor bank ("tiled64").
// The .desc payload is row major, 64 B per descriptor.  A lane that owns one bank
// row needs all 64 B of it in registers; loading that straight from the row-major
// image makes every wave-instruction touch 64 different 64-B segments.  The bank is
// therefore re-tiled ONCE at map load: rows are grouped in blocks of 64 (one per
// lane of a wavefront) and each block is stored as 4 planes of 64 x 16 B:
//     tiled[(block*4 + plane)*64 + lane] = row(block*64 + lane).uint4[plane]
// so that the four global_load_dwordx4 a wave issues for a block are each one
// contiguous, fully coalesced 1 KiB.
// ---------------------------------------------------------------------------
constexpr uint32_t kBlockRows = 64;
constexpr int kK1CounterSlots = 64;  // Ctx::d_k1_counters
constexpr int kSelPairsSlot = 2 * kK1CounterSlots;  // the word after them: pairs scanned for device-built view lists
constexpr int kP3pMaxN = 4096;     // 2D-3D correspondences the P3P LDS sort holds
constexpr int kP3pBatchMax = 512;  // hypotheses evaluated per round
// (kP3pSlots, the batch sizes of a round and every other threshold the choice of a kernel form depends on: forms.h)
constexpr uint32_t kPartHeaderBytes = 16;  // candidate part: {u32 n_cand, pad[3]} then the candidates

using Pose = sfmloc_pose;

// one 2D-3D candidate (K4); `order` sorts candidates of one query feature exactly as the reference's
// sequential scan would meet them (distance, then view id, then position in the view's list)
struct Candidate {
  uint64_t order;
  uint32_t qfeat;
  uint32_t landmark_id;
  double X[3];
};

struct P3pState {
  int n, iter, n_iter, n_reserve, n_index, identity, n_in, done, rounds, status;
  unsigned arrive;  // workgroups of the current round that have delivered their hypothesis (k_p3p_round)
  int finished;     // the epilogue (pose, inlier pairs) has run (k_p3p_finish)
  int batch_limit;  // hypotheses the current round evaluates (<= the launch's grid); see p3p_next_batch_limit
  int switch_iter;  // iteration at which sampling switched to the best model's inliers
  // hypotheses prep_iter .. prep_iter + prep_n - 1 have their P3P models in P3pArgs::prep_models already: the workgroup
  // that replayed the previous round solved them, one hypothesis per lane (acransac.hip "Prepared ahead")
  int prep_iter, prep_n;
  // the lowest hypothesis index of the current round whose model is known to change the index set (NFA below the round's
  // starting NFA and below 0), or ~0u: a workgroup that STARTS after that is known -- while the GPU is shared a round's
  // workgroups trickle in -- evaluates nothing, because the replay throws everything behind that hypothesis away
  unsigned first_hit;
  double min_nfa, errmax;
  double model[12];
};

struct HostResult;
struct P3pArgs {
  P3pState *state;
  Pose *result;
  const HostResult *record;  // the context's result record in device memory (state, pose, status, inlier pairs) ...
  HostResult *host;          // ... and its pinned host copy, which k_p3p_finish fills itself (no copy launch)
  const uint32_t *ms_n, *ms_qfeat, *ms_landmark;
  const double *pt2d, *pt3d;
  double *xn;
  const double *L10;
  float *logc_n, *logc_k;
  int32_t *vec_index, *best_inl;
  double *hyp_nfa;
  int *hyp_k;
  double *hyp_err, *hyp_model;
  int32_t *hyp_inl;
  double *prep_models;  // [kP3pBatchMax][4][12] models of the coming round's hypotheses ("Prepared ahead"), and how many
  int *prep_nm;         // roots each has; prep_ahead = 0: every workgroup solves its own hypothesis
  int prep_ahead;
  uint32_t *pair_qfeat, *pair_landmark, *inlier_idx;
  uint64_t *ws_key;  // [kP3pLargeBatch * max_n] sort segments for more than kP3pMaxN correspondences, or null
  uint32_t *ws_idx;
  double *ws_terms;  // [max_n / 2 + 1]
  double focal, ppx, ppy;
  int max_iteration, min_resection_points, min_inliers, max_n, refine_pose;
  int adaptive_batch;  // other queries share the GPU: trade rounds for fewer speculative hypotheses
  int adapt_quarters, adapt_floor;  // next batch = max(floor, quarters/4 * iterations since the switch)
  uint64_t seed;
  uint32_t stream;
  int uncal;  // the query is uncalibrated: six-point resection (acransac.hip "resect6"); focal / ppx / ppy hold N1
};

// what a finished query copies back in one asynchronous transfer
struct HostResult {
  P3pState state;
  Pose pose;
  int status;
  uint32_t view_stats[3];  // views with >= min_putative matches, views passing the F filter, the largest view above 512
  uint32_t pair_qfeat[kP3pMaxN];
  uint32_t pair_landmark[kP3pMaxN];
};

// One array into device memory: allocated (at least min_alloc elements, for an array that must have an address when it
// is empty) and filled from the host on stream s.  acct: devmem.h.
template <class T>
inline int dev_upload(uint64_t *acct, DevBuf<T> &p, const T *h, size_t n, hipStream_t s, size_t min_alloc = 0) {
  SFM_RC(p.alloc(acct, n > min_alloc ? n : min_alloc));
  return p.upload(h, n, s);
}

// A call's stream and its two timing events, let go on every way out.  Declare it before the call's DevBuf locals
// (devmem.h, order of destruction).
struct CallScope {
  hipStream_t s = nullptr;  // (what the launchers read: own_'s, or the handle's)
  ~CallScope() {
    if (s) hipStreamSynchronize(s);  // a handle's stream too; then the events go, then a stream of its own
  }
  // `device` exists and is the current one
  static int use_device(int device) {
    int ndev = 0;
    const hipError_t e = hipGetDeviceCount(&ndev);
    SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV, "no HIP device visible; this library has no CPU fallback");
    SFM_CHECK(device >= 0 && device < ndev, SFMLOC_EINVAL, "device %d out of range (0..%d)", device, ndev - 1);
    SFM_HIP(hipSetDevice(device));
    return SFMLOC_OK;
  }
  // a stream of its own on the current device, or a handle's; *ms: 0 now, and time_end's figure if `timed`
  int open(bool timed, double *ms, hipStream_t borrowed = nullptr) {
    if (!borrowed) SFM_RC(own_.create());
    s = borrowed ? borrowed : own_.get();
    if (timed) {
      SFM_RC(e0_.create(kTimingEvent));
      SFM_RC(e1_.create(kTimingEvent));
    }
    ms_ = ms;
    *ms_ = 0.0;
    return SFMLOC_OK;
  }
  int time_begin() {
    if (e0_) SFM_HIP(hipEventRecord(e0_, s));
    return SFMLOC_OK;
  }
  int time_end() {  // (waits for the work between the two)
    if (!e0_) return SFMLOC_OK;
    SFM_HIP(hipEventRecord(e1_, s));
    SFM_HIP(hipEventSynchronize(e1_));
    float ms = 0.f;
    SFM_HIP(hipEventElapsedTime(&ms, e0_, e1_));
    *ms_ = ms;
    return SFMLOC_OK;
  }

 private:
  Stream own_;
  Event e0_, e1_;
  double *ms_ = nullptr;
};

// The timed part of a one-shot call on `device`: *last_ms is zeroed; with `work`, body(stream) runs between the two
// events of a stream of its own and *last_ms is their distance.  The body's DevBufs go before the stream does.
template <class Body>
inline int timed_call(int device, double *last_ms, bool work, Body &&body) {
  SFM_RC(CallScope::use_device(device));
  *last_ms = 0.0;
  if (!work) return SFMLOC_OK;  // nothing to launch
  CallScope d;
  SFM_RC(d.open(true, last_ms));
  SFM_RC(d.time_begin());
  SFM_RC(body(d.s));
  return d.time_end();
}

struct Ctx;

// Static, read-only after creation: the map as it sits in HBM.
struct Map {

  int device = 0;
  int n_cu = 256;
  sfmloc_params params{};

  uint64_t n_rows = 0;
  uint32_t n_blocks = 0;  // ceil(n_rows / 64)
  uint32_t max_view_blocks = 0;  // most 64-row blocks any one view overlaps (launch bound of a device-side selection)
  uint32_t max_view_rows = 0;    // most rows of any one view
  std::atomic<int> busy_ctx{0};  // contexts with work queued (begin .. end / sync): K1 slices a short scan only when alone
  FormCredits credits;  // the sizes its finished queries had: what the next ones' K3 / K5 launches are shaped for (forms.h)
  uint32_t n_views = 0;
  uint32_t n_landmarks = 0;
  std::vector<uint32_t> h_view_id, h_view_off, h_view_wh;
  std::vector<double> h_view_center;     // [n_views*3], maps opened from sfm_data.json only
  std::vector<std::string> h_view_file;  // view filenames, same
  DevBuf<uint4> d_bank;  // tiled64, n_blocks*64 rows (zero padded)
  // The view tables carry one extra, EMPTY view at index n_views ("phantom": no rows, id 0xFFFFFF): a device-built
  // selection whose length the host cannot know (the sharded BoW shortlist) is padded with it, and every kernel
  // treats it as a view without descriptors.  Per-view arrays of a context are sized n_views + 1 for the same reason.
  DevBuf<uint32_t> d_view_off;  // [n_views+2]  (view_off[n_views+1] = view_off[n_views] = n_rows)
  DevBuf<uint32_t> d_view_id;  // [n_views+1]
  DevBuf<uint32_t> d_view_wh;  // [(n_views+1)*2]
  DevBuf<float2> d_kpt;  // [n_rows]
  DevBuf<int32_t> d_row_landmark;
  DevBuf<uint32_t> d_landmark_id;
  DevBuf<double> d_landmark_X;
  double focal = 0, ppx = 0, ppy = 0, k1 = 0, k2 = 0, k3 = 0;
  uint32_t intrinsic_type = 0;  // 0 pinhole, 3 pinhole_radial_k3
  uint32_t bow_dim = 0;
  DevBuf<float> d_bow;
  DevBuf<double> d_L10;  // [65538] log10(i)
  DevBuf<uint16_t> d_ratio_cnt;  // [513]
  float ratio_cnt_for = -1.0f;      // ratio the table was built for
  bool have_geometry = false;       // kpts + landmarks + view sizes + intrinsic were supplied
  uint64_t hbm_bytes = 0;  // what the map's own buffers above hold (its contexts keep their own figure: map_hbm_bytes)

  Ctx *ctx0 = nullptr;              // the handle's own context (stage-level API)
  std::vector<Ctx *> pool;          // every other context of this map (owned by the map)
  std::vector<Ctx *> batch_ctx;     // the subset sfmloc_localize_batch round-robins over
};

// Everything one in-flight query needs: a stream and the workspace of every stage.  Several contexts
// of one map run concurrently (the latency-bound RANSAC stages of one query overlap the VALU-bound
// Hamming kernel of another).
struct Ctx : GangMember {  // (gang.h: stream, gang_recs, gang_head)
  Stream own_stream;  // what stream.own reads: its own, or borrowed from `lender` (first: devmem.h, order of destruction)
  Map *map = nullptr;
  Ctx *lender = nullptr;           // the context whose stream this one works on (sfmloc_context_create_sharing)
  bool merge_only = false;         // no workspace of the matching stages (sfmloc_context_create_merge)
  int borrowers = 0;               // contexts working on this one's stream
  bool zombie = false;             // destroyed while lent out: freed with its last borrower
  uint64_t hbm_bytes = 0;          // what the buffers below hold now (every DevBuf of the context is charged to it)

  // --- putative stage ---
  uint32_t max_split = 8;
  DevBuf<uint2> d_part;  // [n_blocks*64] partial (best0,best1), laid out [split][work block][lane]
  DevBuf<uint32_t> d_view_sel;  // [n_views] selected view indices
  DevBuf<uint32_t> d_view_widx0;  // [n_views] work-block index of each selected view's first bank block
  DevBuf<uint32_t> d_block_list;  // [n_blocks]
  HostBuf<uint32_t> h_pinned;  // pinned staging: view_sel | view_widx0 | block_list
  DevBuf<uint32_t> d_view_count;  // [n_views]
  DevBuf<uint32_t> d_match_i;  // [n_rows]
  DevBuf<uint32_t> d_match_key;  // [n_rows]  (d0<<16)|j0
  DevBuf<uint2> d_flagged;  // [n_blocks*64] rows the screening kernel could not reject {part index, bank row}
  DevBuf<uint32_t> d_n_flagged;
  DevBuf<unsigned long long> d_flagmask;  // [n_blocks] per work block: rows whose d_part slot is valid (screened scan)
  bool last_screened = false;
  DevBuf<uint2> d_rows_scratch;  // [rows_chunk_cap][8 slices][64] partial top-2 of the flagged-row pass
  DevBuf<uint32_t> d_rows_arrivals;  // [rows_chunk_cap] arrival counters of that pass (self-resetting)
  DevBuf<uint4> d_flagged_desc;  // [rows_chunk_cap][4][64] descriptors of the flagged rows (tiled like the bank)
  uint32_t rows_chunk_cap = 0;          // chunks of 64 flagged rows the sliced pass has scratch for (rest: fallback)
  // [kK1CounterSlots][2] finished wave-pairs, flagged rows (since stats reset): a wave adds to slot (its block & 63) -- one
  // pair of words for every wave of a scan was 300 000 atomics on the same address per full-bank scan; then one word
  // (kSelPairsSlot): bank rows x query rows of the scans whose block list a shortlist's workgroup built
  DevBuf<unsigned long long> d_k1_counters;
  int k1_finish_ops = 0;

  // --- geometric stages ---
  DevBuf<uint32_t> d_geo_count;  // [n_views]
  DevBuf<uint32_t> d_geo_idx;  // [n_rows]
  DevBuf<double> d_geo_model;  // [(n_views+1)*10] per view: AC-RANSAC's F (normalised frame, 9) + errorMax
  // guided matching (-gm): allocated on first use
  DevBuf<uint32_t> d_geo_j;  // [n_rows] query feature of each guided match (geo_idx then holds the map feature)
  DevBuf<uint32_t> d_guided_row;  // [n_rows] per bank row: its guided query feature or SFMLOC_NOMATCH
  bool geo_is_pairs = false;          // the last geometric stage left (i, j) lists, not indices into the putative lists
  // K3 for views with more putative matches than its LDS form holds (acransac.hip k_fmatrix_large): allocated on first use
  DevBuf<uint64_t> fl_key;
  DevBuf<uint32_t> fl_idx, fl_count, fl_list;
  DevBuf<unsigned char> d_k3_static;  // K3's per-context argument block on the device (FFilterStatic, acransac.hip) ...
  unsigned char k3_static_host[256] = {};  // ... and what was last written there
  bool k3_static_valid = false;
  DevBuf<unsigned char> d_k3_spec;  // k_fmatrix_fast's wide form: the first batch's K3Spec results per view slot (lazily)
  DevBuf<unsigned int> d_k3_arrive;  // ... and the arrivals
  DevBuf<int32_t> fl_vec_index, fl_best_inl;
  DevBuf<float> fl_logc_n, fl_logc_k;
  int fl_slot_m = 0;
  int *d_status = nullptr;  // (raw: inside d_result)
  DevBuf<unsigned char> d_cand_part;  // this context's candidate part: header + cand_cap candidates (one per query
                                      // feature at most, so 2^16 can never overflow)
  uint32_t cand_cap = 1u << 16;
  DevBuf<uint16_t> d_geo_dist;  // [n_rows] per geometric match: its featDist, or 0xFFFF = not a candidate
  DevBuf<unsigned long long> d_best64;  // [65536]
  DevBuf<uint32_t> d_winner;  // [65536]
  DevBuf<uint32_t> d_ms_n, d_ms_qfeat, d_ms_landmark;  // [65536]
  DevBuf<double> d_pt2d, d_pt3d;  // [65536*2], [65536*3]
  DevBuf<double> d_xn;  // [kP3pMaxN*2]
  DevBuf<float> d_logc_n, d_logc_k;  // [kP3pMaxN+1]
  DevBuf<int32_t> d_vec_index, d_best_inl;  // [kP3pMaxN]
  DevBuf<double> d_hyp_nfa, d_hyp_err, d_hyp_model, d_prep_models;
  DevBuf<int> d_prep_nm;
  DevBuf<int> d_hyp_k;
  DevBuf<int32_t> d_hyp_inl;  // [kP3pBatchMax * kP3pMaxN]
  uint32_t *d_pair_qfeat = nullptr, *d_pair_landmark = nullptr;  // [p3p_cap] raw: inside d_result, or the *_big arrays
  DevBuf<uint32_t> d_inlier_idx;  // [p3p_cap]
  // the P3P arrays hold p3p_cap correspondences: kP3pMaxN to begin with, regrown (ctx_p3p_reserve) when a query with
  // more features arrives; beyond kP3pMaxN the pair lists leave HostResult for buffers of their own and the sort of a
  // hypothesis gets a global-memory segment
  uint32_t p3p_cap = kP3pMaxN;
  bool p3p_small = false;  // this query's P3P rounds go out in the small form (decided when the first ones are queued)
  uint32_t p3p_query_n = 0;  // features of the query K5 is about to run for (ctx_p3p_reserve): launch shape of the rounds
  uint32_t p3p_stream = 0;   // K5's sampling stream (Philox key): 0 for queries; the view id when adjust.hip resects a view
  bool p3p_own_K = false;    // K5 uses p3p_K (focal, ppx, ppy) instead of the map's intrinsic (adjust.hip: per view)
  double p3p_K[3] = {0.0, 0.0, 0.0};
  bool p3p_uncal = false;    // the query K5 is about to run for is uncalibrated (Query::uncalibrated): six-point resection
  double p3p_N[3] = {1.0, 0.0, 0.0};  // ... normalised by N1 of its image: {sqrt(w h), w / 2, h / 2}
  DevBuf<uint32_t> d_pair_qfeat_big, d_pair_landmark_big;
  DevBuf<uint64_t> d_p3p_ws_key;
  DevBuf<uint32_t> d_p3p_ws_idx;
  DevBuf<double> d_p3p_terms;
  P3pState *d_p3p_state = nullptr;  // (raw: inside d_result)
  Pose *d_pose = nullptr;
  // one HostResult record; d_p3p_state, d_pose, d_status, d_view_stats (and, up to kP3pMaxN correspondences, d_pair_qfeat /
  // d_pair_landmark) are raw pointers into it
  DevBuf<unsigned char> d_result;
  uint32_t *d_view_stats = nullptr;  // [3] HostResult::view_stats (raw: inside d_result)
  DevBuf<float> d_bow_query;  // [bow_dim]
  DevBuf<uint32_t> d_bow_dist;  // [n_views]
  DevBuf<uint32_t> d_bow_cand;  // [n_views]
  DevBuf<uint32_t> d_bow_sel;  // [n_views]
  HostBuf<HostResult> h_result;  // pinned: what a finished query copies back in one go
  Event pinned_busy;  // recorded after the last upload out of h_pinned
  Event xev_out, xev_in;  // ordering against a caller's stream (sfmloc_context_signal / _wait)

  // What the context remembers from one call to the next.  last_*: the last putative call, which the staged API's
  // later stages and readers work on.  k1_may_slice (and p3p_small above) hold from a query's begin to its end;
  // p3p_init_fused (like p3p_uncal, p3p_N, p3p_own_K, p3p_stream, p3p_query_n above) is carried from the match set to the
  // resection, also across staged calls and by adjust.hip.  What holds for one entry-point call only is not here: the
  // call passes it down as a QueryPass.
  uint32_t last_split = 0;
  uint32_t last_nq = 0;
  uint32_t last_n_sel = 0;
  bool last_all_views = false;
  uint32_t last_n_work_blocks = 0;
  std::vector<uint32_t> last_blocks;  // host copy of the block list (empty = all)
  bool last_blocks_on_device = false; // the list was built by k_blocks_from_views: fetch it when a reader needs it
  bool counted_busy = false;          // this context is counted in Map::busy_ctx
  bool others_busy = false;           // other contexts of the map had work queued when this query began (ctx_mark_busy)
  bool k1_may_slice = true;           // K1's use of it: a short scan may be cut into query slices (= !others_busy)
  bool p3p_init_fused = false;        // k_match_set_finish has run K5's initialisation for the query in hand
  struct Query *last_query = nullptr;  // query of the last putative call
  struct Query *in_flight = nullptr;   // query of a begun, not yet ended, localisation
  double t_begin = 0.0;

  // --- measurement ---
  sfmloc_kernel_stats stats{};
  std::vector<std::pair<int, EventPair>> pending_events;
  std::vector<EventPair> event_pool;
};

// The gang form of dev_launch (launch.h), for a kernel that has one (Body: the kernel's body, gang.h): dev_launch on the
// member's stream, or -- while the member records for a gang session -- a record, which answers SFMLOC_OK: gang_flush
// launches it and reports.  `single` is the kernel itself.
template <class... Ts, size_t... Is, class... As>
inline void gang_store_args(void *dst, std::index_sequence<Is...>, As &&...as) {
  new (dst) Tup<Ts...>{TupLeaf<Is, Ts>{static_cast<Ts>(as)}...};
}
struct LaunchMember {  // the member, and where the launch is written (LaunchSite, launch.h)
  GangMember *m;
  LaunchSite at;
  LaunchMember(GangMember *m_, const char *file = __builtin_FILE(), int line = __builtin_LINE()) : m(m_), at{file, line} {}
};
template <class Body, class... Ts, class... As>
inline int sfm_launch(LaunchMember on, void (*single)(Ts...), dim3 grid, dim3 block, uint32_t shmem, As &&...as) {
  GangMember *c = on.m;
  if (!c->stream.gang) return dev_launch(single, grid, block, shmem, LaunchStream((hipStream_t)c->stream, on.at, c->device), as...);
  try {  // (a record is ~2 KB; no exception may cross the C ABI: the session's end reports it -- gang_flush)
    c->gang_recs.emplace_back();
  } catch (const std::bad_alloc &) {
    c->gang_oom = true;
    return SFMLOC_OK;
  }
  GangRec &r = c->gang_recs.back();
  r.key = GangLaunch<Body, Ts...>::key();
  r.cap = GangLaunch<Body, Ts...>::kCap;
  r.single = reinterpret_cast<const void *>(single);
  r.launch_one = &GangLaunch<Body, Ts...>::one;
  r.launch_many = &GangLaunch<Body, Ts...>::many;
  r.grid = grid;
  r.block = block;
  r.shmem = shmem;
  gang_store_args<Ts...>(r.args, std::index_sequence_for<Ts...>{}, as...);
  return SFMLOC_OK;
}

// what K5's plans (forms.h) are made from: the query the context is about to resect for
inline K5In k5_in(const Ctx *c) {
  K5In in;
  in.query_n = c->p3p_query_n;
  in.uncal = c->p3p_uncal;
  in.gang = c->stream.gang != nullptr;
  in.others_busy = c->others_busy;
  in.small = c->p3p_small;
  in.small_credit = c->map->credits.p3p_small.load(std::memory_order_relaxed);
  in.wide_credit = c->map->credits.p3p_wide.load(std::memory_order_relaxed);
  return in;
}
// acransac.hip: K5's kernel arguments for that query (K4's last kernel starts K5 and takes them too); library-internal
__attribute__((visibility("hidden"))) P3pArgs make_p3p_args(Ctx *c, const K5In &in);

struct Query {
  Map *map = nullptr;
  uint32_t n = 0, width = 0, height = 0;
  DevBuf<uint4> d_desc;  // [n_pad*4], row major, zero padded to a multiple of 64 rows
  DevBuf<float2> d_kpt;  // full precision (locFeat, AKAZEOpenCV.cpp:77-79): used for pt2D
  DevBuf<float2> d_kpt6;  // after the .feat text round trip (6 significant digits): used by the F-matrix filter
  DevBuf<float> d_bow;  // the query's BoW vector, resident (sfmloc_query_set_bow), [bow_dim] or null
  std::vector<float> h_kpt;
  bool is_view = false;  // the device arrays are borrowed from the caller (sfmloc_query_create_view)
  bool uncalibrated = false;  // sfmloc_query_set_uncalibrated: no intrinsic is assumed for this query's camera
};

// one of a query's own arrays (not part of any memory figure), for the hipError_t chains of the functions that fill them
hipError_t dev_raw_alloc_error();  // capi.hip: what hipMalloc answered to this thread's last dev_raw_alloc
template <class T>
inline hipError_t query_array(DevBuf<T> &b, size_t n) {
  return b.alloc(nullptr, n) == SFMLOC_OK ? hipSuccess : dev_raw_alloc_error();
}

// What ONE entry-point call has decided or already done for its query: created on the entry point's stack and passed
// down to the stages and launchers that act on it, so nothing of it outlives the call.  The staged entry points, which
// drive one stage per call, pass a default-constructed one.
struct QueryPass {
  bool chain_done = false;       // the shortlist kernel already cleared the counters and built the block list
  bool cleared = false;          // this query's counters are cleared (k_query_reset or that chain): the stages skip their memsets
  bool k3_follows = false;       // the caller runs K3 right after K1 on this context: K2 may be left to K3
  bool flagmask_zeroed = false;  // d_flagmask has just been cleared (with the device-built block list) for the coming scan
  bool merge_deferred = false;   // K2 was left to K3: launch_fmatrix_filter passes `merge` to k_fmatrix_fast
  MergeMaskedArgs merge{};
};

// The views a putative call matches against: all of the map, or ascending view indices in host or in device memory
// (device: the BoW shortlist -- the block list is then built by a kernel and the host never sees the views).
struct ViewSel {
  enum Kind { kAll, kHost, kDevice } kind = kAll;
  const uint32_t *views = nullptr;
  uint32_t n = 0;
  static ViewSel host(const uint32_t *v, uint32_t n) { return v ? ViewSel{kHost, v, n} : ViewSel{}; }  // (C ABI: null = all)
  static ViewSel device(const uint32_t *d, uint32_t n) { return ViewSel{kDevice, d, n}; }
};

// capi.hip: K1 + K2 of the selected views against q on context c (sfmloc_match_putative's body)
int match_putative_on(Ctx *c, Query *q, const uint32_t *view_sel, uint32_t n_sel);

// hamming.hip
int launch_tile_bank(const uint4 *d_rows, uint64_t row0, uint64_t n_rows_chunk, uint4 *d_bank, hipStream_t s);
int launch_hamming_top2(Ctx *c, const Query *q, QueryPass &pass, uint32_t n_work_blocks, bool use_list, uint32_t split);
int launch_blocks_from_views(Ctx *c, QueryPass &pass, const uint32_t *d_sel, uint32_t n_sel, uint32_t bound);
int launch_merge_ratio_compact(Ctx *c, const Query *q, QueryPass &pass, uint32_t n_sel, bool all_views, uint32_t split,
                               uint32_t n_work_blocks);


// bow.hip
struct BofModel {
  Stream stream;  // created by the first sfmloc_bof_compute (a model inside a sfmloc_imgbow works on that object's)
  int device = 0;
  int K = 0, cdim = 0, in_dim = 0, n_pca = 0, resized = 300, levels = 2, norm_type = 2, cells = 5;
  DevBuf<float> d_centers, d_pca_mean, d_pca_evec, d_pca_eval;
  // workspace of one call
  DevBuf<uint32_t> d_counts;
  DevBuf<double> d_out;
  DevBuf<float> d_desc, d_kxy;  // a call's descriptors and points: regrown together (sfmloc_bof_compute)
};
struct ChainArgs;  // chain_device.h: what the shortlist's workgroup does on top of the shortlist (may be null)
int launch_bow_select(Ctx *c, const float *d_query, const uint32_t *d_cand, uint32_t n_cand,
                      uint32_t k, uint32_t *d_dist_bits, uint32_t *d_out_sel, const ChainArgs *chain = nullptr);
// sharded shortlist: this shard's k best as sortable keys (distance bits << 32 | global view id), and
// the shard's part of the global k best among n_parts key lists
int launch_bow_keys(Ctx *c, const float *d_query, uint32_t k, uint32_t *d_dist_bits, uint32_t *d_sel_tmp,
                    unsigned long long *d_keys_out);
int launch_bow_merge_select(Ctx *c, const unsigned long long *d_keys, uint32_t n_parts,
                            uint64_t part_stride_keys, uint32_t k, uint32_t n_pad, uint32_t *d_sel_out,
                            const ChainArgs *chain = nullptr);
// d_desc8 non-null: the descriptors are rows of 64 bytes (a .desc row, the first in_dim bytes used) instead of floats
int launch_bof(const BofModel *b, hipStream_t s, const float *d_desc, const float *d_kxy, int n, uint32_t *d_counts,
               double *d_out, float *d_out_f32, const uint8_t *d_desc8 = nullptr);
int launch_bof_member(const BofModel *b, GangMember *m, const float *d_kxy, int n, uint32_t *d_counts, double *d_out,
                      float *d_out_f32, const uint8_t *d_desc8);

// dense.hip: the resize + gray + min-max front end with its tables resident (sfmloc_imgbow; sfmloc_dense_gray builds a
// temporary one).  src: h x w x channels (3 = BGR, 1 = gray: a colour read of a gray file has three equal channels,
// for which BGR2GRAY is the identity, so one channel is resized).
struct DenseGrayPlan {
  int w = 0, h = 0, channels = 3, size = 300;
  DevBuf<int> d_xo, d_yo;
  DevBuf<short> d_xa, d_ya;
  DevBuf<unsigned int> d_mm;
};
int dense_gray_plan_create(DenseGrayPlan *p, int w, int h, int channels, int size);
void dense_gray_plan_destroy(DenseGrayPlan *p);
int dense_gray_enqueue(const DenseGrayPlan *p, hipStream_t s, const uint8_t *d_src, uint8_t *d_gray_out);
int dense_gray_enqueue_member(const DenseGrayPlan *p, GangMember *m, const uint8_t *d_src, uint8_t *d_gray_out);

// akaze.hip: an extractor's device-resident pieces, for callers inside the library (imgbow.hip)
struct Akaze;
uint8_t *akaze_gray_dev(Akaze *a);           // [h*w] the image build_scale_space works on
uint8_t *akaze_desc_dev(Akaze *a);           // [n x 64] descriptors of the last describe
hipStream_t akaze_stream_now(Akaze *a);      // the stream its work is queued on (its own or a context's)
GangMember *akaze_member(Akaze *a);          // the extractor as a gang member (its launches can be recorded for a session)
// scale space of the image ALREADY in akaze_gray_dev (written on akaze_stream_now) + orientation and M-LDB at the
// device-resident keypoints d_kin [n x 4] (x, y, size, class_id); asynchronous
int akaze_compute_resident(Akaze *a, const float *d_kin, unsigned int n, int need_levels /*0: all*/);
// imgbow.hip: the dense grid of the BoW front end [n x 4] (x, y, size, class_id) and its points [n x 2] (kxy may be null);
// throws std::bad_alloc
void dense_grid_build(int size, std::vector<float> *grid, std::vector<float> *kxy);

// imread_dev.hip: a reader's resident image for a consumer inside the library (akaze.hip, imgbow.hip).
// imread_feed: checks that `which` is one image of the reader's last decode, on `device` and w x h (SFMLOC_EINVAL, text
// starting with `who`), makes stream s wait for the reader's work and gives the image's address.  imread_consumed: called
// once the consumer's reads are queued on s, so that the reader's next decode does not overwrite the image under them.
struct Imread;
int imread_feed(Imread *r, uint32_t which, int device, uint32_t w, uint32_t h, hipStream_t s, const uint8_t **dev, const char *who);
int imread_consumed(Imread *r, hipStream_t s);

// acransac.hip
int launch_fill_log10(double *d_L10, int n, hipStream_t s);
int launch_debug_math(int op, const double *d_in, int n, int in_stride, double *d_out, int out_stride, hipStream_t s);
// min_putative < 0: the map's params.min_putative (the query path's >=16 rule, localization.cpp:408-415)
int launch_fmatrix_filter(Ctx *c, const Query *q, QueryPass &pass, uint32_t n_sel, bool all_views, int min_putative = -1);
// guided.hip: GeometricFilter_FMatrix_AC::Geometry_guided_matching for the views that passed K3 (their geo lists are
// replaced by (map feature, query feature) lists in d_geo_idx / d_geo_j)
int ensure_guided_workspace(Ctx *c);
int launch_guided_matching(Ctx *c, const Query *q, uint32_t n_sel, bool all_views);
// k4_matchset.hip
int launch_match_set(Ctx *c, const Query *q, const QueryPass &pass, uint32_t n_sel, bool all_views);
int launch_emit_candidates(Ctx *c, const Query *q, const QueryPass &pass, uint32_t n_sel, bool all_views);
int launch_export_part(Ctx *c, void *dst_dev, uint32_t cap);
// packed_b > 0: `parts` are packed batch parts of packed_b queries (k4_matchset.hip PartLayout), cap = their budget,
// and this query is number packed_qi of the batch
int launch_select_candidates(Ctx *c, const Query *q, const QueryPass &pass, const unsigned char *parts, uint32_t n_parts,
                             uint64_t part_bytes, uint32_t cap, uint32_t packed_b = 0, uint32_t packed_qi = 0,
                             bool reset_status = false);  // (also clear the context's status word: sfmloc_merge_begin)
int launch_export_packed(Ctx *c, void *dst_dev, uint32_t n_queries, uint32_t budget, uint32_t qi);
uint64_t packed_part_bytes(uint32_t n_queries, uint32_t budget);
int ctx_p3p_reserve(Ctx *c, uint32_t n_query_rows);  // capi.hip: grow the P3P workspace to a query's feature count
int launch_merge_masked_now(Ctx *c, const MergeMaskedArgs &M, uint32_t n_sel);  // hamming.hip: a deferred K2 as a launch of its own
// acransac.hip
int launch_p3p_init(Ctx *c);
int launch_p3p_round(Ctx *c, int batch);
int launch_p3p_finish(Ctx *c);
// capi.hip: K5 on correspondences the caller has already written into the context's 2D-3D buffers (d_ms_n, d_pt2d,
// d_pt3d, d_ms_qfeat, d_ms_landmark) -- ctx_p3p_reserve first; _begin queues init + rounds + finish, _wait drains
// the stream and queues more rounds until the state machine is done (the query path's own ctx_resection_* steps)
int ctx_resection_begin(Ctx *c);
int ctx_resection_wait_done(Ctx *c);
// capi.hip: K5 of context c runs for q next -- calibrated or not (Ctx::p3p_uncal, p3p_N)
int ctx_set_query_camera(Ctx *c, const Query *q, const char *who);
void ctx_set_uncalibrated_camera(Ctx *c, uint32_t width, uint32_t height);  // ... from here on uncalibrated, image w x h

}  // namespace sfmloc
