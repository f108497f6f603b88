// C ABI of libsfmloc_hip.so (include/sfmloc.h): handles, HBM residency, streams, measurement.
//
// Two kinds of state:
//   Map  static, read-only after creation: tiled descriptor bank, view table, keypoints, landmarks, tables;
//   Ctx  one in-flight query: a HIP stream plus the workspace of every stage.
// The stage-level entry points (sfmloc_match_putative ... sfmloc_resection) run on the map's own context;
// sfmloc_localize_begin/_end run a whole query asynchronously on any context, so that several queries
// overlap (the latency-bound RANSAC kernels of one under the VALU-bound Hamming kernel of another).
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <exception>
#include <new>

#include "chain_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {

static thread_local char g_err[512] = "";

void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

namespace {

double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// test hooks (no environment variable: a stray one must not be able to fail a production allocation).
// sfmloc_debug_fail_next_alloc(k) arms the calling thread's g_fail_countdown: its k-th dev_raw_alloc from now fails, once.
// sfmloc_debug_fail_p3p_alloc(k): the k-th allocation of the NEXT regrowth fails; one shot, consumed atomically by the
// regrowth that sees it, which arms g_fail_countdown for its own allocations (ctx_p3p_reserve).
std::atomic<int> g_test_fail_alloc{-1};
thread_local int g_fail_countdown = -1;
thread_local hipError_t g_raw_alloc_err = hipSuccess;  // why the last dev_raw_alloc of this thread failed

}  // namespace

// devmem.h: every DevBuf allocates and frees through these two
int dev_raw_alloc(void **p, size_t bytes) {
  *p = nullptr;
  const bool injected = g_fail_countdown >= 0 && g_fail_countdown-- == 0;
  const hipError_t e = injected ? hipErrorOutOfMemory : hipMalloc(p, bytes);
  g_raw_alloc_err = e;
  if (e == hipSuccess) return SFMLOC_OK;
  if (!injected) (void)hipGetLastError();
  *p = nullptr;
  set_error("hipMalloc(%zu bytes) -> %s", bytes, hipGetErrorString(e));
  return hip_code(e);
}
void dev_raw_free(void *p) { (void)hipFree(p); }
hipError_t dev_raw_alloc_error() { return g_raw_alloc_err; }

// ... and every Stream, Event and HostBuf is created and let go through these (the only places that do)
static int raw_created(const char *what, hipError_t e, void **h) {
  if (e == hipSuccess) return SFMLOC_OK;
  (void)hipGetLastError();
  *h = nullptr;
  set_error("%s -> %s", what, hipGetErrorString(e));
  return hip_code(e);
}
int stream_raw_create(void **s) {
  hipStream_t h = nullptr;
  const hipError_t e = hipStreamCreateWithFlags(&h, hipStreamNonBlocking);
  *s = h;
  return raw_created("hipStreamCreateWithFlags(hipStreamNonBlocking)", e, s);
}
static int raw_done(const char *what, hipError_t e) {  // (as SFM_HIP answers: the error stays with the runtime)
  if (e == hipSuccess) return SFMLOC_OK;
  set_error("%s -> %s", what, hipGetErrorString(e));
  return hip_code(e);
}
void stream_raw_sync(void *s) { (void)hipStreamSynchronize(static_cast<hipStream_t>(s)); }
void stream_raw_destroy(void *s) { (void)hipStreamDestroy(static_cast<hipStream_t>(s)); }
int event_raw_create(void **ev, bool timing) {
  hipEvent_t h = nullptr;
  const hipError_t e = hipEventCreateWithFlags(&h, timing ? hipEventDefault : hipEventDisableTiming);
  *ev = h;
  return raw_created(timing ? "hipEventCreate" : "hipEventCreateWithFlags(hipEventDisableTiming)", e, ev);
}
void event_raw_destroy(void *e) { (void)hipEventDestroy(static_cast<hipEvent_t>(e)); }
int host_raw_alloc(void **p, size_t bytes) {
  return raw_created("hipHostMalloc", hipHostMalloc(p, bytes, hipHostMallocDefault), p);
}
void host_raw_free(void *p) { (void)hipHostFree(p); }

// ... and a kernel's dynamic-LDS limit is raised, on the device that is current, by this one (devmem.h "Dynamic-LDS
// limits"; nothing is launched after a failure, so the error does not stay with the runtime for a later launch's check)
int dev_raw_lds_limit(const void *kernel, uint32_t bytes) {
  const hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
  if (e == hipSuccess) return SFMLOC_OK;
  (void)hipGetLastError();
  set_error("hipFuncSetAttribute(MaxDynamicSharedMemorySize, %u bytes) -> %s", bytes, hipGetErrorString(e));
  return hip_code(e);
}

// ... and every transfer is issued by these two (devmem.h "Transfers": a null stream means done on return)
int dev_raw_copy(void *dst, const void *src, size_t bytes, CopyKind kind, hipStream_t s) {
  const hipMemcpyKind k = kind == CopyKind::kHostToDevice   ? hipMemcpyHostToDevice
                          : kind == CopyKind::kDeviceToHost ? hipMemcpyDeviceToHost
                                                            : hipMemcpyDeviceToDevice;
  const int rc = raw_done("hipMemcpyAsync", hipMemcpyAsync(dst, src, bytes, k, s));
  return rc || s ? rc : raw_done("hipStreamSynchronize(null stream)", hipStreamSynchronize(nullptr));
}
int dev_raw_fill(void *dst, int byte, size_t bytes, hipStream_t s) {
  const int rc = raw_done("hipMemsetAsync", hipMemsetAsync(dst, byte, bytes, s));
  return rc || s ? rc : raw_done("hipStreamSynchronize(null stream)", hipStreamSynchronize(nullptr));
}

namespace {

template <typename T>
int dev_alloc(uint64_t *acct, DevBuf<T> &p, size_t n) {
  return p.alloc(acct, n);
}

// The P3P arrays that grow with a query's feature count, for `cap` correspondences, as one all-or-nothing set: a new
// context's (cap = kP3pMaxN: the pair lists are inside HostResult and a hypothesis sorts in LDS, so those five arrays
// are not made) and every regrowth's (ctx_p3p_reserve).  The new set is complete before the stream is drained --
// kernels of the previous query may still read the old arrays -- and the old set is let go; on failure the context is
// exactly as it was.
int ctx_p3p_workspace(Ctx *c, uint32_t cap) {
  const bool big = cap > (uint32_t)kP3pMaxN;
  const size_t large = (size_t)kP3pLargeBatch * cap;  // hypotheses of a round beyond kP3pMaxN x their sort segments
  DevGroup g(&c->hbm_bytes);
  g.add(c->d_xn, (size_t)cap * 2);
  g.add(c->d_logc_n, (size_t)cap + 1);
  g.add(c->d_logc_k, (size_t)cap + 1);
  g.add(c->d_vec_index, (size_t)cap);
  g.add(c->d_best_inl, (size_t)cap);
  g.add(c->d_hyp_inl, std::max<size_t>((size_t)kP3pSlots * kP3pMaxN, large));  // kP3pSlots lists of kP3pMaxN, or `large`
  g.add(c->d_inlier_idx, (size_t)cap);
  if (big) {
    g.add(c->d_pair_qfeat_big, (size_t)cap);
    g.add(c->d_pair_landmark_big, (size_t)cap);
    g.add(c->d_p3p_ws_key, large);
    g.add(c->d_p3p_ws_idx, large);
    g.add(c->d_p3p_terms, (size_t)cap / 2 + 2);
  }
  if (!g.ok()) {
    if (!big) return g.rc();  // (a new context's first set: the allocation's own code and text, like its other arrays)
    set_error("P3P workspace for %u correspondences: allocation %d of 12 (%zu bytes) failed: %s", cap, g.failed_index(),
              g.failed_bytes(), hipGetErrorString(g_raw_alloc_err));
    return SFMLOC_ENOMEM;
  }
  if (c->d_xn) SFM_HIP(hipStreamSynchronize(c->stream));
  g.commit();
  if (big) {  // no longer inside the HostResult record
    c->d_pair_qfeat = c->d_pair_qfeat_big;
    c->d_pair_landmark = c->d_pair_landmark_big;
  }
  c->p3p_cap = cap;
  return SFMLOC_OK;
}

// sfmloc_map_info::hbm_bytes: the map's own buffers and what each context it owns holds now
uint64_t map_hbm_bytes(const Map *m) {
  uint64_t b = m->hbm_bytes + (m->ctx0 ? m->ctx0->hbm_bytes : 0);
  for (const Ctx *c : m->pool) b += c->hbm_bytes;
  return b;
}

// number of d0 in [0,512] for which the reference's expression holds (MatchUtils.cpp:347):
//   (0.0f + distMat.at<int>(i,0)) / distMat.at<int>(i,1) < fDistRatio
// evaluated here, on the host, in float32 exactly as written there.
void build_ratio_table(float ratio, uint16_t *cnt) {
  for (int d1 = 0; d1 <= 512; ++d1) {
    int c = 0;
    for (int d0 = 0; d0 <= 512; ++d0) {
      volatile float num = 0.0f + (float)d0;
      volatile float den = (float)d1;
      volatile float r = num / den;
      if (r < ratio) c = d0 + 1;  // monotone in d0, so the accepted set is a prefix
    }
    cnt[d1] = (uint16_t)c;
  }
}


struct EventScope {
  Ctx *c;
  int which;
  EventPair ev;
  bool on;
  EventScope(Ctx *c_, int which_)
      : c(c_), which(which_),
        on(c_->map->params.profile == 1 || (c_->map->params.profile == 2 && which_ == SFMLOC_K_HAMMING)) {
    if (!on) return;
    if (!c->event_pool.empty()) {
      ev = std::move(c->event_pool.back());
      c->event_pool.pop_back();
    } else if (ev.a.create(kTimingEvent) || ev.b.create(kTimingEvent)) {
      on = false;
      return;
    }
    hipEventRecord(ev.a, c->stream);
  }
  ~EventScope() {
    if (!on) return;
    hipEventRecord(ev.b, c->stream);
    c->pending_events.emplace_back(which, std::move(ev));
  }
};

// per_kind_ms (optional, [SFMLOC_K_COUNT]): the drained brackets' time by kind, for the caller's own bookkeeping
int drain_events(Ctx *c, double *per_kind_ms = nullptr) {
  for (auto &pe : c->pending_events) {
    float ms = 0.f;
    SFM_HIP(hipEventSynchronize(pe.second.b));
    SFM_HIP(hipEventElapsedTime(&ms, pe.second.a, pe.second.b));
    c->stats.total_ms[pe.first] += ms;
    if (per_kind_ms) per_kind_ms[pe.first] += ms;
    c->stats.launches[pe.first] += 1;
    c->event_pool.push_back(std::move(pe.second));
  }
  c->pending_events.clear();
  return SFMLOC_OK;
}

void free_ctx(Ctx *c) {
  if (!c) return;
  if (c->borrowers > 0) {  // its stream is lent out: the last borrower to go frees it (sfmloc_context_create_sharing)
    c->zombie = true;
    return;
  }
  if (c->stream.own) hipStreamSynchronize(c->stream.own);  // (a borrowed one too)
  Ctx *lender = c->lender;
  delete c;  // (devmem.h, order of destruction: events and pinned blocks, every DevBuf, then a stream of its own)
  if (lender && --lender->borrowers == 0 && lender->zombie) free_ctx(lender);
}

struct CtxFree {
  void operator()(Ctx *c) const { free_ctx(c); }
};

int make_ctx(Map *m, Ctx **out, Ctx *share = nullptr, bool merge_only = false) {
  *out = nullptr;
  std::unique_ptr<Ctx, CtxFree> owner(new (std::nothrow) Ctx());  // (let go, as far as it got, on every early return)
  Ctx *c = owner.get();
  SFM_CHECK(c, SFMLOC_ENOMEM, "out of host memory");
  c->map = m;
  c->device = m->device;
  if (share) {  // no stream (hardware queue) of its own: work is queued on the lender's
    c->own_stream.borrow(share->stream.own);
    c->lender = share;
    ++share->borrowers;
  } else {
    SFM_RC(c->own_stream.create());
  }
  c->stream.own = c->own_stream;
  const hipStream_t s = c->stream;  // every clear below is queued on it, and waited for before the context is handed out
  const uint64_t n_pad = (uint64_t)m->n_blocks * kBlockRows;
  uint64_t *acct = &c->hbm_bytes;
  c->merge_only = merge_only;
  // a context that only ever merges candidate parts and runs P3P (sfmloc_context_create_merge) has no use for the
  // per-bank-row arrays of the matching stages: 30 B per row and the 32 MB of the flagged-row pass
  const bool full = !merge_only;
  if (full) SFM_RC(dev_alloc(acct, c->d_part, (size_t)n_pad));
  SFM_RC(dev_alloc(acct, c->d_view_sel, (size_t)m->n_views + 1));
  SFM_RC(dev_alloc(acct, c->d_view_widx0, (size_t)m->n_views + 1));
  if (full) SFM_RC(dev_alloc(acct, c->d_block_list, (size_t)m->n_blocks));
  SFM_RC(dev_alloc(acct, c->d_view_count, (size_t)m->n_views + 1));  // + the phantom view (sfmloc_internal.h)
  if (full) SFM_RC(dev_alloc(acct, c->d_match_i, (size_t)m->n_rows));
  if (full) SFM_RC(dev_alloc(acct, c->d_match_key, (size_t)m->n_rows));
  if (full) SFM_RC(dev_alloc(acct, c->d_flagged, (size_t)n_pad));
  SFM_RC(dev_alloc(acct, c->d_n_flagged, (size_t)1));
  if (full) SFM_RC(dev_alloc(acct, c->d_flagmask, (size_t)m->n_blocks + 1));
  c->rows_chunk_cap = m->n_blocks < 4096 ? (m->n_blocks ? m->n_blocks : 1) : 4096;  // 4096 chunks = 262 k flagged rows, 16 MB
  if (full) {
    SFM_RC(dev_alloc(acct, c->d_rows_scratch, (size_t)c->rows_chunk_cap * 8 * 64));
    SFM_RC(dev_alloc(acct, c->d_rows_arrivals, (size_t)c->rows_chunk_cap));
    SFM_RC(dev_alloc(acct, c->d_flagged_desc, (size_t)c->rows_chunk_cap * 4 * 64));
    SFM_RC(c->d_rows_arrivals.zero(s));
  }
  SFM_RC(dev_alloc(acct, c->d_k1_counters, (size_t)kSelPairsSlot + 1));
  SFM_RC(c->d_k1_counters.zero(s));
  SFM_RC(dev_alloc(acct, c->d_geo_count, (size_t)m->n_views + 1));
  if (full) SFM_RC(dev_alloc(acct, c->d_geo_idx, (size_t)m->n_rows));
  SFM_RC(dev_alloc(acct, c->d_geo_model, ((size_t)m->n_views + 1) * 10));
  // everything a finished query reports lives in ONE device record laid out as HostResult: one D2H copy per query
  SFM_RC(dev_alloc(acct, c->d_result, sizeof(HostResult)));
  {
    HostResult *r = reinterpret_cast<HostResult *>(c->d_result.get());
    c->d_p3p_state = &r->state;
    c->d_pose = &r->pose;
    c->d_status = &r->status;
    c->d_view_stats = r->view_stats;
    c->d_pair_qfeat = r->pair_qfeat;
    c->d_pair_landmark = r->pair_landmark;
  }
  SFM_RC(dev_alloc(acct, c->d_cand_part, (size_t)kPartHeaderBytes + (size_t)c->cand_cap * sizeof(Candidate)));
  if (full) SFM_RC(dev_alloc(acct, c->d_geo_dist, (size_t)m->n_rows));
  SFM_RC(dev_alloc(acct, c->d_best64, (size_t)65536));
  SFM_RC(dev_alloc(acct, c->d_winner, (size_t)65536));
  SFM_RC(dev_alloc(acct, c->d_ms_n, (size_t)1));
  SFM_RC(dev_alloc(acct, c->d_ms_qfeat, (size_t)65536));
  SFM_RC(dev_alloc(acct, c->d_ms_landmark, (size_t)65536));
  SFM_RC(dev_alloc(acct, c->d_pt2d, (size_t)65536 * 2));
  SFM_RC(dev_alloc(acct, c->d_pt3d, (size_t)65536 * 3));
  SFM_RC(dev_alloc(acct, c->d_hyp_nfa, (size_t)kP3pSlots));
  SFM_RC(dev_alloc(acct, c->d_hyp_err, (size_t)kP3pSlots));
  SFM_RC(dev_alloc(acct, c->d_hyp_model, (size_t)kP3pSlots * 12));
  SFM_RC(dev_alloc(acct, c->d_hyp_k, (size_t)kP3pSlots));
  SFM_RC(dev_alloc(acct, c->d_prep_models, (size_t)kP3pBatchMax * 48));
  SFM_RC(dev_alloc(acct, c->d_prep_nm, (size_t)kP3pBatchMax));
  SFM_RC(ctx_p3p_workspace(c, kP3pMaxN));  // the arrays that ctx_p3p_reserve regrows
  if (m->bow_dim) {
    SFM_RC(dev_alloc(acct, c->d_bow_query, (size_t)m->bow_dim));
    SFM_RC(dev_alloc(acct, c->d_bow_dist, (size_t)m->n_views));
    SFM_RC(dev_alloc(acct, c->d_bow_cand, (size_t)m->n_views));
    SFM_RC(dev_alloc(acct, c->d_bow_sel, (size_t)m->n_views + 1));
  }
  SFM_RC(c->h_pinned.alloc((size_t)2 * m->n_views + m->n_blocks + 16));
  SFM_RC(c->h_result.alloc(1));
  memset(c->h_result, 0, sizeof(HostResult));
  SFM_RC(dev_zero(c->d_status, 1, s));
  SFM_RC(c->d_view_count.zero(s));
  SFM_RC(c->d_geo_count.zero(s));
  SFM_RC(c->d_ms_n.zero(s));
  SFM_RC(c->xev_out.create(kOrderingEvent));
  SFM_RC(c->xev_in.create(kOrderingEvent));
  SFM_RC(dev_zero(c->d_pose, 1, s));
  SFM_RC(dev_zero(c->d_p3p_state, 1, s));
  SFM_RC(dev_zero(c->d_view_stats, 3, s));
  // (the arrival counters of k_hamming_rows and K1's statistics among them: a first scan that met garbage arrival counters
  // merged nothing and left the head pass's seeds to K2 -- the one wrong first scan of round 4,
  // profiles/r04_pytest_gpu_failed_run_excerpt.txt -- so no clear of a context goes anywhere but its own stream)
  SFM_HIP(hipStreamSynchronize(s));
  *out = owner.release();
  return SFMLOC_OK;
}

void free_map(Map *m) {
  if (!m) return;
  hipSetDevice(m->device);
  for (Ctx *c : m->pool) free_ctx(c);
  free_ctx(m->ctx0);
  delete m;  // (its DevBufs free their arrays)
}

// ----- stages on a context --------------------------------------------------------------------------

// Every counter / flag the stages of one query start from, cleared by ONE launch instead of eight memsets (each a
// separate ~5 us dispatch on the query's critical path).  The stage functions keep their own memsets for callers
// that drive them one at a time (QueryPass::cleared says which applies).
struct QueryResetBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(QueryResetArgs R) {
    query_reset_items(R, blockIdx.x * 256 + threadIdx.x, gridDim.x * 256);  // chain_device.h
  }
};
__global__ __launch_bounds__(256) void k_query_reset(QueryResetArgs R) {
  QueryResetBody::run(R);
}

QueryResetArgs make_reset_args(Ctx *c, const Query *q) {
  QueryResetArgs R;
  R.view_count = c->d_view_count;
  R.geo_count = c->d_geo_count;
  R.n_views = c->map->n_views;
  R.best64 = c->d_best64;
  R.nq = q->n ? q->n : 1;
  R.n_flagged = c->d_n_flagged;
  R.status = c->d_status;
  R.cand_header = reinterpret_cast<uint32_t *>(c->d_cand_part.get());
  R.view_stats = c->d_view_stats;
  R.ms_n = c->d_ms_n;
  R.fl_count = c->fl_count;
  return R;
}

int ctx_reset_for_query(Ctx *c, const Query *q, QueryPass &pass) {
  Map *m = c->map;
  if (pass.chain_done) {  // the shortlist's workgroup already did it (chain_after_shortlist)
    pass.cleared = true;
    return SFMLOC_OK;
  }
  const uint32_t nq = q->n ? q->n : 1;
  const uint32_t n = m->n_views + 1 > nq ? m->n_views + 1 : nq;
  SFM_RC(sfm_launch<QueryResetBody>(c, k_query_reset, dim3((n + 255) / 256), dim3(256), 0, make_reset_args(c, q)));
  pass.cleared = true;
  return SFMLOC_OK;
}

// The chain a shortlist kernel runs after the shortlist (reset + block list of the knn selected views in d_sel)
ChainArgs make_chain_args(Ctx *c, const Query *q, const uint32_t *d_sel, uint32_t n_sel) {
  Map *m = c->map;
  ChainArgs C{};  // (keys_out = null: no key list)
  C.enabled = 1;
  C.reset = make_reset_args(c, q);
  C.blocks.sel = d_sel;
  C.blocks.n_sel = n_sel;
  C.blocks.view_off = m->d_view_off;
  C.blocks.view_sel_out = c->d_view_sel;
  C.blocks.widx0 = c->d_view_widx0;
  C.blocks.block_list = c->d_block_list;
  C.blocks.bound = (uint32_t)std::min<uint64_t>(m->n_blocks, (uint64_t)n_sel * m->max_view_blocks);
  C.blocks.flagmask = c->d_flagmask;
  C.blocks.pairs_out = c->d_k1_counters + kSelPairsSlot;
  C.blocks.nq = q->n;
  return C;
}

// A short scan is cut into query slices (more waves, better balance, ~7 % more arithmetic) only when the GPU has
// nothing else to fill it with, i.e. when no other context of the map has work queued.
static void ctx_mark_busy(Ctx *c) {
  Map *m = c->map;
  c->others_busy = m->busy_ctx.load(std::memory_order_relaxed) - (c->counted_busy ? 1 : 0) > 0;
  c->k1_may_slice = !c->others_busy;
  if (!c->counted_busy) {
    c->counted_busy = true;
    m->busy_ctx.fetch_add(1, std::memory_order_relaxed);
  }
}
static void ctx_mark_idle(Ctx *c) {
  if (c->counted_busy) {
    c->counted_busy = false;
    c->map->busy_ctx.fetch_sub(1, std::memory_order_relaxed);
  }
}

int ctx_match_putative(Ctx *c, Query *q, QueryPass &pass, const ViewSel &sel) {
  Map *m = c->map;
  SFM_CHECK(!c->merge_only, SFMLOC_EINVAL, "this context was created for sfmloc_merge_begin only (sfmloc_context_create_merge)");
  const bool all_views = sel.kind == ViewSel::kAll;
  const uint32_t n_sel = all_views ? m->n_views : sel.n;
  SFM_CHECK(n_sel <= m->n_views, SFMLOC_EINVAL, "view selection: n_sel %u > n_views %u", n_sel, m->n_views);

  // selected views -> ascending list of the 64-row bank blocks they overlap, plus per selected view the
  // position of its first block in that list
  uint32_t n_work_blocks = m->n_blocks;
  c->last_blocks.clear();
  c->last_blocks_on_device = false;
  if (sel.kind == ViewSel::kDevice) {
    // launch bound the host can know: every selected view overlaps at most max_view_blocks blocks
    const uint64_t bound = std::min<uint64_t>(m->n_blocks, (uint64_t)n_sel * m->max_view_blocks);
    n_work_blocks = (uint32_t)bound;
    if (n_sel && pass.chain_done) {
      pass.flagmask_zeroed = true;  // (built by the shortlist's workgroup, chain_after_shortlist)
    } else if (n_sel) {
      int rc = launch_blocks_from_views(c, pass, sel.views, n_sel, n_work_blocks);
      if (rc) return rc;
    }
    c->last_blocks_on_device = true;
  } else if (!all_views) {
    if (c->pinned_busy) SFM_HIP(hipEventSynchronize(c->pinned_busy));  // previous upload still reading the staging
    uint32_t *h_sel = c->h_pinned;
    uint32_t *h_w0 = c->h_pinned + m->n_views;
    uint32_t *h_blk = c->h_pinned + 2 * (size_t)m->n_views;
    uint32_t nb = 0;
    for (uint32_t k = 0; k < n_sel; ++k) {
      const uint32_t v = sel.views[k];
      SFM_CHECK(v < m->n_views, SFMLOC_EINVAL, "view selection: index %u out of range", v);
      SFM_CHECK(k == 0 || sel.views[k - 1] < v, SFMLOC_EINVAL, "view selection must be strictly ascending");
      h_sel[k] = v;
      h_w0[k] = 0;
      const uint32_t r0 = m->h_view_off[v], r1 = m->h_view_off[v + 1];
      if (r1 == r0) continue;
      const uint32_t b0 = r0 / kBlockRows, b1 = (r1 - 1) / kBlockRows;
      uint32_t b = b0;
      if (nb && h_blk[nb - 1] == b0) {  // the previous selected view ends in this view's first block
        h_w0[k] = nb - 1;
        b = b0 + 1;
      } else {
        h_w0[k] = nb;
      }
      for (; b <= b1; ++b) h_blk[nb++] = b;
    }
    n_work_blocks = nb;
    c->last_blocks.assign(h_blk, h_blk + nb);
    if (n_sel) {
      SFM_RC(c->d_view_sel.upload(h_sel, n_sel, c->stream));
      SFM_RC(c->d_view_widx0.upload(h_w0, n_sel, c->stream));
    }
    if (nb) SFM_RC(c->d_block_list.upload(h_blk, nb, c->stream));
    SFM_RC(c->pinned_busy.ensure(kOrderingEvent));
    SFM_HIP(hipEventRecord(c->pinned_busy, c->stream));
  }

  // query split: spread a short block list over the chip (partial top-2 are merged in K2); the partial
  // buffer holds n_blocks wave-blocks in all
  uint32_t split = 1;
  if (n_work_blocks && q->n >= 256) {
    const uint64_t want = (uint64_t)m->n_cu * 8;
    while (split < c->max_split && (uint64_t)n_work_blocks * split < want && q->n / (split * 2) >= 128 &&
           (uint64_t)n_work_blocks * split * 2 <= m->n_blocks)
      split *= 2;
  }

  if (!pass.cleared) SFM_RC(c->d_view_count.zero((size_t)m->n_views + 1, c->stream));
  c->last_split = split;
  c->last_nq = q->n;
  c->last_n_sel = n_sel;
  c->last_all_views = all_views;
  c->last_n_work_blocks = n_work_blocks;
  c->last_query = q;
  if (q->n == 0 || n_sel == 0) return SFMLOC_OK;

  int rc;
  {
    EventScope ev(c, SFMLOC_K_HAMMING);
    rc = launch_hamming_top2(c, q, pass, n_work_blocks, !all_views, split);
  }
  if (rc) return rc;
  // (the shortlist's workgroup counts the blocks of the list it builds, chain_device.h: n_work_blocks is only its launch
  // bound, and a shard that owns none of the shortlist scans nothing)
  if (!(sel.kind == ViewSel::kDevice && pass.chain_done))
    c->stats.hamming_pairs += (uint64_t)n_work_blocks * kBlockRows * q->n;
  c->stats.hamming_alg_bytes += (uint64_t)n_work_blocks * kBlockRows * 64 + (uint64_t)q->n * 64;
  {
    EventScope ev(c, SFMLOC_K_COMPACT);
    rc = launch_merge_ratio_compact(c, q, pass, n_sel, all_views, split, n_work_blocks);
  }
  return rc;
}

int check_stage(Ctx *c, Query *q, const char *who) {
  SFM_CHECK(c && q, SFMLOC_EINVAL, "%s: null argument", who);
  Map *m = c->map;
  SFM_CHECK(q->map == m, SFMLOC_EINVAL, "%s: query belongs to another map", who);
  SFM_CHECK(m->have_geometry, SFMLOC_EINVAL,
            "%s: the map was created without view sizes / keypoints / landmarks / intrinsics", who);
  SFM_CHECK(q->n == 0 || q->d_kpt, SFMLOC_EINVAL, "%s: the query was created without keypoints", who);
  SFM_CHECK(q->n == 0 || (q->width > 0 && q->height > 0), SFMLOC_EINVAL, "%s: query image size missing", who);
  SFM_CHECK(c->last_query == q, SFMLOC_EINVAL, "%s: run sfmloc_match_putative with this query first", who);
  return SFMLOC_OK;
}

int ctx_geometric_filter(Ctx *c, Query *q, QueryPass &pass) {
  Map *m = c->map;
  if (!pass.cleared) {
    SFM_RC(c->d_geo_count.zero((size_t)m->n_views + 1, c->stream));
    SFM_RC(dev_zero(c->d_status, 1, c->stream));
  }
  if (q->n == 0 || c->last_n_sel == 0) return SFMLOC_OK;
  EventScope ev(c, SFMLOC_K_FMATRIX);
  int rc = launch_fmatrix_filter(c, q, pass, c->last_n_sel, c->last_all_views);
  if (rc) return rc;
  // -gm (MatchUtils.cpp:413-415): the surviving views' matches are re-derived under the estimated F
  if (m->params.guided_matching) rc = launch_guided_matching(c, q, c->last_n_sel, c->last_all_views);
  return rc;
}

int ctx_match_set(Ctx *c, Query *q, const QueryPass &pass) {
  EventScope ev(c, SFMLOC_K_MATCHSET);
  return launch_match_set(c, q, pass, c->last_n_sel, c->last_all_views);
}

// What every begin starts with: the query's counters cleared, K1 + K2 of the selection and, unless the chain is cut
// after them (k3 = false: measurements), K3 -- whose per-view workgroups then build their own match lists where they can
int ctx_match_and_filter(Ctx *c, Query *q, QueryPass &pass, const ViewSel &sel, const char *who, bool k3 = true) {
  int rc = ctx_reset_for_query(c, q, pass);
  if (rc) return rc;
  pass.k3_follows = k3;
  rc = ctx_match_putative(c, q, pass, sel);
  if (rc) return rc;
  rc = check_stage(c, q, who);
  if (rc || !k3) return rc;
  return ctx_geometric_filter(c, q, pass);
}

// What the entry points of the sharded path check first (in_flight = false: the caller checks that later itself)
int check_sharded(const Ctx *c, const Query *q, const char *who, bool in_flight = true) {
  SFM_CHECK(q->map == c->map, SFMLOC_EINVAL, "%s: query belongs to another map", who);
  SFM_CHECK(!q->uncalibrated, SFMLOC_EINVAL,
            "%s: an uncalibrated query (sfmloc_query_set_uncalibrated) is not supported on the sharded path", who);
  SFM_CHECK(!in_flight || c->in_flight == nullptr, SFMLOC_EINVAL, "%s: context has a query in flight", who);
  return SFMLOC_OK;
}

}  // namespace

// Which camera K5 assumes for the query the context is about to serve (sfmloc.h "Uncalibrated queries"): the map's
// intrinsic, or none -- the six-point resection on points conditioned by N1 of the query's image.
void ctx_set_uncalibrated_camera(Ctx *c, uint32_t width, uint32_t height) {
  c->p3p_uncal = true;  // N1 of the image: x' = (x - w / 2) / sqrt(w h)
  c->p3p_N[0] = sqrt((double)width * (double)height);
  c->p3p_N[1] = 0.5 * (double)width;
  c->p3p_N[2] = 0.5 * (double)height;
}
int ctx_set_query_camera(Ctx *c, const Query *q, const char *who) {
  c->p3p_uncal = false;
  if (!q->uncalibrated) return SFMLOC_OK;
  SFM_CHECK(!c->stream.gang, SFMLOC_EINVAL, "%s: an uncalibrated query is not supported in a gang session", who);
  SFM_CHECK(q->width > 0 && q->height > 0, SFMLOC_EINVAL, "%s: query image size missing", who);
  ctx_set_uncalibrated_camera(c, q->width, q->height);
  return SFMLOC_OK;
}

namespace {

// Enqueues P3P AC-RANSAC rounds.  The device-side state machine turns surplus rounds into no-ops, so a fixed
// number is enqueued without synchronising.
int ctx_resection_enqueue(Ctx *c, bool first_call) {
  int rc = SFMLOC_OK;
  if (first_call) {
    rc = launch_p3p_init(c);
    if (rc) return rc;
  }
  const K5QueryPlan P = plan_k5_query(k5_in(c), knobs());  // forms.h
  if (first_call) c->p3p_small = P.small;  // (ctx_resection_wait corrects it if the set turns out larger)
  const int rounds = first_call ? P.first_rounds : P.later_rounds;
  for (int r = 0; r < rounds && rc == SFMLOC_OK; ++r)
    rc = launch_p3p_round(c, (first_call && r == 0) ? kP3pFirstBatch : kP3pLaterBatch);
  if (rc == SFMLOC_OK) rc = launch_p3p_finish(c);  // pose + inlier pairs once the state says "done"; a no-op before
  return rc;
}

}  // namespace

// Grows the P3P workspace of a context to hold `n` correspondences (a query has at most one per feature).  Rare: only a
// query with more than kP3pMaxN features gets here.  On failure the context keeps its old arrays and capacity and the
// caller gets SFMLOC_ENOMEM (ctx_p3p_workspace).  A context that is recording for a gang session never gets here with
// work recorded -- the reserve is the first thing a query's stage does -- but if it does, reading c->stream issues
// what was recorded first (gang.h), so stream order is still call order.
int ctx_p3p_reserve(Ctx *c, uint32_t n) {
  c->p3p_query_n = n;
  if (n <= c->p3p_cap) return SFMLOC_OK;
  uint32_t cap = c->p3p_cap;
  while (cap < n) cap <<= 1;
  const int k = g_test_fail_alloc.exchange(-1, std::memory_order_relaxed);
  if (k >= 0) g_fail_countdown = k;  // (the P3P hook; unarmed, the thread's own countdown stands)
  const int rc = ctx_p3p_workspace(c, cap);
  if (k >= 0) g_fail_countdown = -1;
  return rc;
}

namespace {

// The host copy of the result record is written by k_p3p_finish itself (p3p_publish), which every call of
// ctx_resection_enqueue ends with; a copy is only needed when the chain stops before K5 (measurements).
int ctx_fetch_result(Ctx *c, bool no_p3p = false) {
  if (!no_p3p) return SFMLOC_OK;
  HostResult *h = c->h_result;
  SFM_RC(c->d_result.download(h, sizeof(HostResult), c->stream));
  return SFMLOC_OK;
}

int ctx_resection_wait(Ctx *c) {
  HostResult *h = c->h_result;
  for (int guard = 0; guard < 64; ++guard) {
    SFM_HIP(hipStreamSynchronize(c->stream));
    c->stream.dirty = false;
    if (h->state.done) {
      SFM_CHECK((h->pose.status & 8) == 0, SFMLOC_EHIP, "six-point resection: a round found no prepared model (internal)");
      c->map->credits.note_p3p_set(h->state.n);  // what the next queries' rounds look like
      return SFMLOC_OK;
    }
    if (k5_small_refuted(h->state.n)) c->p3p_small = false;
    int rc;
    {
      EventScope ev(c, SFMLOC_K_P3P);
      rc = ctx_resection_enqueue(c, false);
    }
    if (rc) return rc;
    rc = ctx_fetch_result(c);
    if (rc) return rc;
  }
  set_error("P3P AC-RANSAC did not finish (iteration %d of %d)", h->state.iter, h->state.n_iter);
  return SFMLOC_EHIP;
}

static int ctx_localize_begin_impl(Ctx *c, Query *q, QueryPass &pass, const ViewSel &sel);

int ctx_localize_begin(Ctx *c, Query *q, QueryPass &pass, const ViewSel &sel) {
  SFM_CHECK(c->in_flight == nullptr, SFMLOC_EINVAL, "sfmloc_localize_begin: context already has a query in flight");
  ctx_mark_busy(c);
  const int rc = ctx_localize_begin_impl(c, q, pass, sel);
  if (rc) ctx_mark_idle(c);
  return rc;
}

// SFMLOC_DIAG_STOP_AFTER = 1 (putative matches) / 2 (geometric filter) / 3 (2D-3D set): measurements only -- the chain
// ends there and sfmloc_localize_end returns an empty pose (bench.py marks such a line as not the metric)
static int diag_stop_after() {
  static const int v = env_int("SFMLOC_DIAG_STOP_AFTER", 0);
  return v;
}

static int ctx_localize_begin_impl(Ctx *c, Query *q, QueryPass &pass, const ViewSel &sel) {
  c->t_begin = now_s();
  int rc = ctx_set_query_camera(c, q, "sfmloc_localize");
  if (rc) return rc;
  rc = ctx_p3p_reserve(c, q->n);
  if (rc) return rc;
  const int stop = diag_stop_after();
  rc = ctx_match_and_filter(c, q, pass, sel, "sfmloc_localize", stop != 1);
  if (rc) return rc;
  if (stop == 0 || stop > 2) {
    rc = ctx_match_set(c, q, pass);
    if (rc) return rc;
  }
  if (stop == 0) {
    EventScope ev(c, SFMLOC_K_P3P);
    rc = ctx_resection_enqueue(c, true);
  }
  if (rc) return rc;
  rc = ctx_fetch_result(c, stop != 0);
  if (rc) return rc;
  c->in_flight = q;
  return SFMLOC_OK;
}

int ctx_localize_end(Ctx *c, sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark, uint32_t cap) {
  SFM_CHECK(c->in_flight != nullptr, SFMLOC_EINVAL, "sfmloc_localize_end: no query in flight on this context");
  c->in_flight = nullptr;
  ctx_mark_idle(c);
  if (diag_stop_after()) {  // truncated chain (measurements): nothing to wait for but the stream
    SFM_HIP(hipStreamSynchronize(c->stream));
    memset(out, 0, sizeof(*out));
    return SFMLOC_OK;
  }
  int rc = ctx_resection_wait(c);
  if (rc) return rc;
  HostResult *h = c->h_result;
  *out = h->pose;
  out->status |= h->status;
  out->n_putative_views = (int32_t)h->view_stats[0];
  out->n_geometric_views = (int32_t)h->view_stats[1];
  c->map->credits.note_k3_largest_view(h->view_stats[2]);  // the form of the next queries' K3
  // (none of these can be reached with data the reference accepts: a view's matches beyond 65 536, an internal
  // inconsistency of the candidate part, more correspondences than the query has features)
  SFM_CHECK((out->status & 1) == 0, SFMLOC_ECAP, "a view has more than 65536 putative matches");
  SFM_CHECK((out->status & 2) == 0, SFMLOC_ECAP, "more than %u 2D-3D candidates (match-set workspace)", c->cand_cap);
  SFM_CHECK((out->status & 4) == 0, SFMLOC_ECAP, "more than %u 2D-3D correspondences (P3P workspace)", c->p3p_cap);
  if (out->ok && out->n_inliers > 0 && (pair_qfeat || pair_landmark)) {
    const uint32_t k = (uint32_t)out->n_inliers;
    SFM_CHECK(cap >= k, SFMLOC_ECAP, "pair buffers hold %u entries, %u inliers", cap, k);
    if (c->p3p_cap > (uint32_t)kP3pMaxN) {  // the pair lists live outside the HostResult record
      const hipStream_t cs = c->stream;
      if (pair_qfeat) SFM_RC(dev_read(pair_qfeat, c->d_pair_qfeat, k, cs));
      if (pair_landmark) SFM_RC(dev_read(pair_landmark, c->d_pair_landmark, k, cs));
    } else {
      if (pair_qfeat) memcpy(pair_qfeat, h->pair_qfeat, k * sizeof(uint32_t));
      if (pair_landmark) memcpy(pair_landmark, h->pair_landmark, k * sizeof(uint32_t));
    }
  }
  // the reference's `times` (LocalizeEngine.cc:643-658): with params.profile = 1 every stage of this query was
  // bracketed by HIP events on its stream -- selectBow = K8, putMatch = K1 + K2, geoMatch = K3, PnP = 2D-3D set + P3P
  // (the reference's PnP bucket runs from the end of geometricMatch to the end of Localize), others = the rest of the
  // wall time begin -> end.  Without profiling only the total is known and it goes to `others`.
  for (int i = 0; i < 7; ++i) out->stage_seconds[i] = 0.0;
  const double wall = now_s() - c->t_begin;
  if (c->map->params.profile == 1) {
    double per[SFMLOC_K_COUNT] = {0};
    rc = drain_events(c, per);
    if (rc) return rc;
    out->stage_seconds[1] = per[SFMLOC_K_BOW] * 1e-3;
    out->stage_seconds[3] = (per[SFMLOC_K_HAMMING] + per[SFMLOC_K_COMPACT]) * 1e-3;
    out->stage_seconds[4] = per[SFMLOC_K_FMATRIX] * 1e-3;
    out->stage_seconds[5] = (per[SFMLOC_K_MATCHSET] + per[SFMLOC_K_P3P]) * 1e-3;
    double sum = 0.0;
    for (int i = 0; i < 6; ++i) sum += out->stage_seconds[i];
    out->stage_seconds[6] = wall > sum ? wall - sum : 0.0;
  } else {
    out->stage_seconds[6] = wall;
  }
  return SFMLOC_OK;
}

}  // namespace

int ctx_resection_begin(Ctx *c) { return ctx_resection_enqueue(c, true); }
int ctx_resection_wait_done(Ctx *c) { return ctx_resection_wait(c); }

// gang.h: issue what the members of a gang session have recorded -- the heads of their lists that are the same kernel
// on the same grid as ONE launch, a head without a partner as a plain launch
int gang_flush(GangState *g) {
  int rc = SFMLOC_OK;
  bool oom = false;
  for (GangMember *m : g->members) oom |= m->gang_oom;
  if (oom) {  // a chain with a launch missing must not run at all: drop the session's records
    for (GangMember *m : g->members) {
      m->gang_recs.clear();
      m->gang_head = 0;
      m->gang_oom = false;
    }
    set_error("gang session: out of host memory while recording launches; the launches still recorded were dropped");
    return SFMLOC_ENOMEM;
  }
  for (;;) {
    // the members advance in step: always the earliest position any member still has to issue, and there every member
    // whose record is the same kernel on the same grid in ONE launch (dynamic LDS: the largest request serves all)
    size_t pos = SIZE_MAX;
    for (GangMember *m : g->members)
      if (m->gang_head < m->gang_recs.size() && m->gang_head < pos) pos = m->gang_head;
    if (pos == SIZE_MAX) break;
    GangRec *grp[kGangMembers];
    int n = 0;
    GangRec *lead = nullptr;
    uint32_t shmem = 0;
    for (GangMember *m : g->members) {
      if (m->gang_head != pos || pos >= m->gang_recs.size()) continue;
      GangRec *r = &m->gang_recs[pos];
      if (lead && !(r->key == lead->key && r->grid.x == lead->grid.x && r->grid.y == lead->grid.y &&
                    r->grid.z == lead->grid.z && r->block.x == lead->block.x && r->block.y == lead->block.y &&
                    r->block.z == lead->block.z))
        continue;
      if (!lead) lead = r;
      grp[n++] = r;
      shmem = r->shmem > shmem ? r->shmem : shmem;
      ++m->gang_head;
      if (n == lead->cap) break;
    }
    const bool together = n > 1 && lead->grid.z == 1;
    int lrc = SFMLOC_OK;  // (a launch that fails leaves its text; the rest of the chain is still issued, as before)
    const LaunchStream on(g->stream, LaunchSite{__FILE__, __LINE__}, g->members[0]->device);
    if (together) {
      lead->shmem = shmem;
      lrc = lead->launch_many(grp, n, on);
    } else {
      for (int i = 0; i < n; ++i) {
        const int one = grp[i]->launch_one(*grp[i], on);
        lrc = lrc ? lrc : one;
      }
    }
    g->launches += together ? 1 : n;
    g->gang_launches += together ? 1 : 0;
    rc = lrc ? lrc : rc;
  }
  for (GangMember *m : g->members) {
    m->gang_recs.clear();
    m->gang_head = 0;
  }
  return rc;
}

int gang_open(GangMember *const *members, int n) {
  GangMember *lead = members[0];
  if (!lead->gang_owned) {
    lead->gang_owned.reset(new (std::nothrow) GangState());
    SFM_CHECK(lead->gang_owned, SFMLOC_ENOMEM, "out of host memory");
  }
  GangState *g = lead->gang_owned.get();
  SFM_RC(g->done.ensure(kOrderingEvent));
  SFM_CHECK(lead->stream.own, SFMLOC_EINVAL, "gang session: the leading member has no stream");
  g->stream = lead->stream.own;
  g->members.clear();
  for (int i = 0; i < n; ++i) {
    GangMember *c = members[i];
    c->ever_ganged = true;
    // (own == nullptr: a member that has no stream of its own yet -- an extractor that only ever worked in sessions)
    if (i > 0 && c->stream.own && c->stream.dirty && c->stream.own != g->stream) {  // the member's own earlier work comes first
      SFM_RC(c->gang_ev.ensure(kOrderingEvent));
      SFM_HIP(hipEventRecord(c->gang_ev, c->stream.own));
      SFM_HIP(hipStreamWaitEvent(g->stream, c->gang_ev, 0));
      c->stream.dirty = false;
    }
    g->members.push_back(c);
  }
  for (GangMember *c : g->members) c->stream.gang = g;
  return SFMLOC_OK;
}

int gang_close(GangMember *lead) {
  GangState *g = lead->stream.gang;
  if (!g) return SFMLOC_OK;
  const int rc = gang_flush(g);
  for (GangMember *c : g->members) c->stream.gang = nullptr;
  lead->stream.dirty = true;
  // the members' own streams continue after the gang's work
  bool any_own = false;
  for (size_t i = 1; i < g->members.size(); ++i)
    any_own |= g->members[i]->stream.own && g->members[i]->stream.own != g->stream;
  if (any_own) {
    SFM_HIP(hipEventRecord(g->done, g->stream));
    for (size_t i = 1; i < g->members.size(); ++i)
      if (g->members[i]->stream.own && g->members[i]->stream.own != g->stream) {
        SFM_HIP(hipStreamWaitEvent(g->members[i]->stream.own, g->done, 0));
        // the member's stream now carries a dependency on the session's work: a later session under ANOTHER leader
        // must order itself after it (gang_open records and waits only for dirty members) -- ADVICE r02
        g->members[i]->stream.dirty = true;
      }
  }
  return rc;  // (gang_flush has set the message)
}

int match_putative_on(Ctx *c, Query *q, const uint32_t *view_sel, uint32_t n_sel) {
  QueryPass pass;
  return ctx_match_putative(c, q, pass, ViewSel::host(view_sel, n_sel));
}
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

const char *sfmloc_last_error(void) { return g_err; }
int sfmloc_abi_version(void) { return SFMLOC_ABI_VERSION; }

int sfmloc_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void sfmloc_default_params(sfmloc_params *p) {
  if (!p) return;
  memset(p, 0, sizeof(*p));
  p->dist_ratio = 0.6f;         // localization.cpp:70
  p->ransac_round = 200;        // localization.cpp:71
  p->geom_precision = 4.0;      // localization.cpp:81
  p->bow_knn = 0;               // localization.cpp:73
  p->min_putative = 16;         // localization.cpp:56
  p->min_resection_points = 8;  // localization.cpp:57
  p->min_inliers = 10;          // localization.cpp:58
  p->p3p_max_iteration = 4096;  // OpenMVG Image_Localizer_Match_Data default
  p->seed = 0x5f3759df12345678ull;
  p->refine_pose = 0;
  p->device = 0;
  p->profile = 0;
  p->exact_rows = 0;
  p->k1_mfma = 1;
  p->guided_matching = 0;       // -gm: false (localization.cpp:82, computeFeaturesAndMatches.cpp:63)
}

// what sfmloc_map_create accepts (nothing here touches a device)
static int map_desc_check(const sfmloc_map_desc *d) {
  SFM_CHECK(d->n_views > 0 && d->view_id && d->view_off, SFMLOC_EINVAL, "sfmloc_map_create: no views");
  SFM_CHECK(d->view_off[0] == 0 && d->view_off[d->n_views] == d->n_rows, SFMLOC_EINVAL,
            "sfmloc_map_create: view_off must start at 0 and end at n_rows");
  SFM_CHECK(d->n_rows < (1ull << 32) - 64, SFMLOC_EINVAL, "sfmloc_map_create: more than 2^32 rows per shard");
  SFM_CHECK(d->n_rows == 0 || d->desc, SFMLOC_EINVAL, "sfmloc_map_create: desc is null");
  for (uint32_t v = 0; v < d->n_views; ++v) {
    SFM_CHECK(d->view_off[v] <= d->view_off[v + 1], SFMLOC_EINVAL, "sfmloc_map_create: view_off not monotone at %u", v);
    SFM_CHECK(v == 0 || d->view_id[v - 1] < d->view_id[v], SFMLOC_EINVAL,
              "sfmloc_map_create: view_id must be strictly ascending at %u", v);
    SFM_CHECK(d->view_id[v] < (1u << 24), SFMLOC_EINVAL, "sfmloc_map_create: view id %u >= 2^24", d->view_id[v]);
  }
  if (d->row_landmark) {
    SFM_CHECK(d->n_landmarks == 0 || (d->landmark_id && d->landmark_X), SFMLOC_EINVAL,
              "sfmloc_map_create: landmark arrays missing");
    for (uint64_t r = 0; r < d->n_rows; ++r)
      SFM_CHECK(d->row_landmark[r] >= -1 && d->row_landmark[r] < (int64_t)d->n_landmarks, SFMLOC_EINVAL,
                "sfmloc_map_create: row_landmark[%llu] out of range", (unsigned long long)r);
  }
  return SFMLOC_OK;
}

// a new map's tables and its own context, on the current device (p.device); on an error the map is deleted as it stands
static int map_fill(Map *m, const sfmloc_map_desc *d, const sfmloc_params &p) {
  m->device = p.device;
  m->params = p;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, p.device) == hipSuccess) m->n_cu = prop.multiProcessorCount;
  Stream s;  // upload stream (a local: gone before the map's buffers are, on every way out)
  SFM_RC(s.create());
  m->n_rows = d->n_rows;
  m->n_blocks = (uint32_t)((d->n_rows + kBlockRows - 1) / kBlockRows);
  m->max_view_blocks = 0;
  for (uint32_t v = 0; v < d->n_views; ++v) {
    const uint32_t r0 = d->view_off[v], r1 = d->view_off[v + 1];
    if (r1 > r0) m->max_view_blocks = std::max(m->max_view_blocks, (r1 - 1) / kBlockRows - r0 / kBlockRows + 1);
    m->max_view_rows = std::max(m->max_view_rows, r1 - r0);
  }
  m->n_views = d->n_views;
  m->n_landmarks = d->row_landmark ? d->n_landmarks : 0;
  m->h_view_id.assign(d->view_id, d->view_id + d->n_views);
  m->h_view_off.assign(d->view_off, d->view_off + d->n_views + 1);
  if (d->view_wh) m->h_view_wh.assign(d->view_wh, d->view_wh + 2 * (size_t)d->n_views);
  m->focal = d->focal;
  m->ppx = d->ppx;
  m->ppy = d->ppy;
  m->k1 = d->k1;
  m->k2 = d->k2;
  m->k3 = d->k3;
  SFM_CHECK(d->intrinsic_type == 0 || d->intrinsic_type == 3, SFMLOC_EINVAL,
            "sfmloc_map_create: intrinsic_type %u (0 = pinhole, 3 = pinhole_radial_k3)", d->intrinsic_type);
  m->intrinsic_type = d->intrinsic_type;
  uint64_t *acct = &m->hbm_bytes;

  // bank: upload row-major chunks and re-tile on the device
  const uint64_t n_pad = (uint64_t)m->n_blocks * kBlockRows;
  SFM_RC(dev_alloc(acct, m->d_bank, (size_t)n_pad * 4));
  if (n_pad) {
    SFM_RC(m->d_bank.zero(s));
    const uint64_t chunk = 16ull << 20;  // rows per staging chunk (1 GiB)
    DevBuf<uint4> d_stage;
    const uint64_t stage_rows = std::min<uint64_t>(chunk, d->n_rows);
    SFM_RC(d_stage.alloc(nullptr, stage_rows * 4));
    for (uint64_t r0 = 0; r0 < d->n_rows; r0 += chunk) {
      const uint64_t n = std::min<uint64_t>(chunk, d->n_rows - r0);
      SFM_RC(d_stage.upload(d->desc + r0 * 64, n * 4, s)  /* (64-byte rows as four uint4) */);
      SFM_RC(launch_tile_bank(d_stage, r0, n, m->d_bank, s));
      SFM_HIP(hipStreamSynchronize(s));
    }
  }

  {  // view tables + the phantom (empty) view at index n_views (sfmloc_internal.h)
    std::vector<uint32_t> off(d->view_off, d->view_off + d->n_views + 1), id(d->view_id, d->view_id + d->n_views);
    off.push_back((uint32_t)d->n_rows);
    id.push_back(0xFFFFFFu);
    SFM_RC(dev_upload(acct, m->d_view_off, off.data(), off.size(), s));
    SFM_RC(dev_upload(acct, m->d_view_id, id.data(), id.size(), s));
    if (d->view_wh) {
      std::vector<uint32_t> wh(d->view_wh, d->view_wh + 2 * (size_t)d->n_views);
      wh.push_back(1);
      wh.push_back(1);
      SFM_RC(dev_upload(acct, m->d_view_wh, wh.data(), wh.size(), s));
    }
    SFM_HIP(hipStreamSynchronize(s));  // the staging vectors go out of scope
  }
  if (d->kpt_xy)
    SFM_RC(dev_upload(acct, m->d_kpt, reinterpret_cast<const float2 *>(d->kpt_xy), (size_t)d->n_rows, s));
  if (d->row_landmark) {
    SFM_RC(dev_upload(acct, m->d_row_landmark, d->row_landmark, (size_t)d->n_rows, s));
    SFM_RC(dev_upload(acct, m->d_landmark_id, d->landmark_id, (size_t)d->n_landmarks, s));
    SFM_RC(dev_upload(acct, m->d_landmark_X, d->landmark_X, (size_t)d->n_landmarks * 3, s));
  }
  if (d->bow && d->bow_dim) {
    m->bow_dim = d->bow_dim;
    SFM_RC(dev_upload(acct, m->d_bow, d->bow, (size_t)d->n_views * d->bow_dim, s));
  }
  m->have_geometry = d->view_wh && d->kpt_xy && d->row_landmark && d->focal > 0.0;
  SFM_RC(dev_alloc(acct, m->d_L10, (size_t)65538));
  SFM_RC(launch_fill_log10(m->d_L10, 65538, s));
  {
    uint16_t tab[513];
    build_ratio_table(p.dist_ratio, tab);
    SFM_RC(dev_alloc(acct, m->d_ratio_cnt, (size_t)513));
    SFM_RC(m->d_ratio_cnt.upload(tab, 513, s));
    SFM_HIP(hipStreamSynchronize(s));  // tab lives on the stack
    m->ratio_cnt_for = p.dist_ratio;
  }
  SFM_HIP(hipStreamSynchronize(s));
  s.reset();  // (before the context's stream comes into being)
  return make_ctx(m, &m->ctx0);
}

int sfmloc_map_create(const sfmloc_map_desc *d, const sfmloc_params *params, sfmloc_map **out) {
  SFM_CHECK(d && out, SFMLOC_EINVAL, "sfmloc_map_create: null argument");
  *out = nullptr;
  SFM_RC(map_desc_check(d));
  const sfmloc_params p = options_or(params, sfmloc_default_params);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV,
            "no HIP device visible (%s); this library has no CPU fallback",
            e == hipSuccess ? "device count 0" : hipGetErrorString(e));
  SFM_CHECK(p.device >= 0 && p.device < ndev, SFMLOC_EINVAL, "device %d out of range (0..%d)", p.device, ndev - 1);
  SFM_HIP(hipSetDevice(p.device));
  // (the map has no context yet when filling it fails, so deleting it lets everything go)
  return make_handle<Map>("sfmloc_map_create", out, [&](Map *m) { return map_fill(m, d, p); });
}

void sfmloc_map_destroy(sfmloc_map *map) { free_map(reinterpret_cast<Map *>(map)); }

int sfmloc_map_get_info(const sfmloc_map *map, sfmloc_map_info *info) {
  SFM_CHECK(map && info, SFMLOC_EINVAL, "sfmloc_map_get_info: null argument");
  const Map *m = reinterpret_cast<const Map *>(map);
  info->n_rows = m->n_rows;
  info->n_views = m->n_views;
  info->n_landmarks = m->n_landmarks;
  info->hbm_bytes = map_hbm_bytes(m);
  info->device = m->device;
  return SFMLOC_OK;
}

int sfmloc_context_create(sfmloc_map *map, sfmloc_context **out) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_context_create: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  Ctx *c = nullptr;
  int rc = make_ctx(m, &c);
  if (rc) return rc;
  m->pool.push_back(c);
  *out = reinterpret_cast<sfmloc_context *>(c);
  return SFMLOC_OK;
}

int sfmloc_context_create_sharing(sfmloc_map *map, sfmloc_context *lender, sfmloc_context **out) {
  SFM_CHECK(map && lender && out, SFMLOC_EINVAL, "sfmloc_context_create_sharing: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *l = reinterpret_cast<Ctx *>(lender);
  SFM_CHECK(l->map == m, SFMLOC_EINVAL, "sfmloc_context_create_sharing: the lender belongs to another map");
  SFM_HIP(hipSetDevice(m->device));
  Ctx *c = nullptr;
  int rc = make_ctx(m, &c, l);
  if (rc) return rc;
  m->pool.push_back(c);
  *out = reinterpret_cast<sfmloc_context *>(c);
  return SFMLOC_OK;
}

int sfmloc_context_create_merge(sfmloc_map *map, sfmloc_context *lender, sfmloc_context **out) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_context_create_merge: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *l = reinterpret_cast<Ctx *>(lender);
  SFM_CHECK(!l || l->map == m, SFMLOC_EINVAL, "sfmloc_context_create_merge: the lender belongs to another map");
  SFM_HIP(hipSetDevice(m->device));
  Ctx *c = nullptr;
  int rc = make_ctx(m, &c, l, /*merge_only=*/true);
  if (rc) return rc;
  m->pool.push_back(c);
  *out = reinterpret_cast<sfmloc_context *>(c);
  return SFMLOC_OK;
}

void sfmloc_context_destroy(sfmloc_context *ctx) {
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  if (!c) return;
  Map *m = c->map;
  hipSetDevice(m->device);
  ctx_mark_idle(c);
  auto it = std::find(m->pool.begin(), m->pool.end(), c);
  if (it != m->pool.end()) m->pool.erase(it);
  auto ib = std::find(m->batch_ctx.begin(), m->batch_ctx.end(), c);
  if (ib != m->batch_ctx.end()) m->batch_ctx.erase(ib);
  free_ctx(c);
}

int sfmloc_query_create(sfmloc_map *map, const uint8_t *desc, const float *kpt_xy, uint32_t n, uint32_t width,
                        uint32_t height, sfmloc_query **out) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_query_create: null argument");
  *out = nullptr;
  SFM_CHECK(n == 0 || desc, SFMLOC_EINVAL, "sfmloc_query_create: desc is null");
  SFM_CHECK(n <= SFMLOC_MAX_QUERY_ROWS, SFMLOC_EINVAL, "sfmloc_query_create: %u query descriptors > %u", n,
            SFMLOC_MAX_QUERY_ROWS);
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  return make_handle<Query>("sfmloc_query_create", out, [&](Query *q) -> int {
    q->map = m;
    q->n = n;
    q->width = width;
    q->height = height;
    const size_t n_pad = ((size_t)n + 63) / 64 * 64;
    if (!n_pad) return SFMLOC_OK;
    hipStream_t s = m->ctx0->stream;
    SFM_RC(q->d_desc.alloc(nullptr, n_pad * 4));
    SFM_RC(q->d_desc.zero(s));
    SFM_RC(q->d_desc.upload(desc, (size_t)n * 4, s));
    std::vector<float> k6;
    if (kpt_xy) {
      q->h_kpt.assign(kpt_xy, kpt_xy + 2 * (size_t)n);
      // The reference writes the query's keypoints to <tmp>/<base>.feat with `ostream << float`
      // (6 significant digits, AKAZEOpenCV.cpp:80-81) and the F-matrix filter reads them back through
      // Regions::Load (:106-111); pt2D keeps the unrounded values (:77-79).  Reproduce the round trip.
      k6.resize(2 * (size_t)n);
      sfmloc_feat_round_trip(kpt_xy, 2 * (uint64_t)n, k6.data());
      SFM_RC(q->d_kpt.alloc(nullptr, n));
      SFM_RC(q->d_kpt6.alloc(nullptr, n));
      SFM_RC(q->d_kpt.upload(kpt_xy, n, s));
      SFM_RC(q->d_kpt6.upload(k6.data(), n, s));
    }
    SFM_HIP(hipStreamSynchronize(s));
    return SFMLOC_OK;
  });
}

void sfmloc_feat_round_trip(const float *kpt_xy, uint64_t n_values, float *out) {
  char buf[64];
  for (uint64_t i = 0; i < n_values; ++i) {
    snprintf(buf, sizeof(buf), "%.6g", (double)kpt_xy[i]);
    out[i] = strtof(buf, nullptr);
  }
}

int sfmloc_query_create_view(sfmloc_map *map, const void *desc_dev, const void *kpt_dev, const void *kpt6_dev,
                             const void *bow_dev, uint32_t n, uint32_t width, uint32_t height, sfmloc_query **out) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_query_create_view: null argument");
  *out = nullptr;
  SFM_CHECK(n == 0 || (desc_dev && kpt_dev && kpt6_dev), SFMLOC_EINVAL, "sfmloc_query_create_view: null device pointer");
  SFM_CHECK(n <= SFMLOC_MAX_QUERY_ROWS, SFMLOC_EINVAL, "sfmloc_query_create_view: %u query descriptors > %u", n,
            SFMLOC_MAX_QUERY_ROWS);
  SFM_CHECK(((uintptr_t)desc_dev & 15) == 0 && ((uintptr_t)kpt_dev & 7) == 0 && ((uintptr_t)kpt6_dev & 7) == 0 &&
                ((uintptr_t)bow_dev & 3) == 0,
            SFMLOC_EINVAL, "sfmloc_query_create_view: misaligned device pointer (descriptors 16, keypoints 8, bow 4 bytes)");
  Query *q = new (std::nothrow) Query();
  SFM_CHECK(q, SFMLOC_ENOMEM, "out of host memory");
  q->map = reinterpret_cast<Map *>(map);
  q->n = n;
  q->width = width;
  q->height = height;
  q->is_view = true;
  q->d_desc.borrow(desc_dev);  // (the caller's arrays: never freed here)
  q->d_kpt.borrow(kpt_dev);
  q->d_kpt6.borrow(kpt6_dev);
  q->d_bow.borrow(bow_dev);
  *out = reinterpret_cast<sfmloc_query *>(q);
  return SFMLOC_OK;
}

void sfmloc_query_destroy(sfmloc_query *query) {
  Query *q = reinterpret_cast<Query *>(query);
  if (!q) return;
  if (q->map) {
    hipSetDevice(q->map->device);
    // only the contexts that worked on THIS query can still be reading it: the others keep running (a server destroys a
    // query per request while other users' queries are in flight)
    std::vector<Ctx *> all = q->map->pool;
    if (q->map->ctx0) all.push_back(q->map->ctx0);
    for (Ctx *c : all)
      if (c->last_query == q || c->in_flight == q) {
        hipStreamSynchronize(c->stream);
        if (c->last_query == q) c->last_query = nullptr;
      }
  }
  delete q;  // (frees the arrays it owns; a view's are borrowed)
}

int sfmloc_query_set_bow(sfmloc_query *query, const float *query_bow) {
  SFM_CHECK(query && query_bow, SFMLOC_EINVAL, "sfmloc_query_set_bow: null argument");
  Query *q = reinterpret_cast<Query *>(query);
  Map *m = q->map;
  SFM_CHECK(m && m->bow_dim > 0, SFMLOC_EINVAL, "sfmloc_query_set_bow: the map has no .bow vectors");
  SFM_CHECK(!q->is_view, SFMLOC_EINVAL, "sfmloc_query_set_bow: a view's BoW vector is given to sfmloc_query_create_view");
  SFM_HIP(hipSetDevice(m->device));
  if (!q->d_bow) SFM_HIP(query_array(q->d_bow, m->bow_dim));
  SFM_RC(q->d_bow.upload(query_bow, m->bow_dim, nullptr));
  return SFMLOC_OK;
}

int sfmloc_query_set_uncalibrated(sfmloc_query *query, int on) {
  SFM_CHECK(query, SFMLOC_EINVAL, "sfmloc_query_set_uncalibrated: null argument");
  Query *q = reinterpret_cast<Query *>(query);
  q->uncalibrated = on != 0;
  return SFMLOC_OK;
}

// ----- stage-level API on the map's own context -------------------------------------------------------

int sfmloc_match_putative(sfmloc_map *map, sfmloc_query *query, const uint32_t *view_sel, uint32_t n_sel) {
  SFM_CHECK(map && query, SFMLOC_EINVAL, "sfmloc_match_putative: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Query *q = reinterpret_cast<Query *>(query);
  SFM_CHECK(q->map == m, SFMLOC_EINVAL, "sfmloc_match_putative: query belongs to another map");
  SFM_HIP(hipSetDevice(m->device));
  QueryPass pass;
  return ctx_match_putative(m->ctx0, q, pass, ViewSel::host(view_sel, n_sel));
}

int sfmloc_putative_read(sfmloc_map *map, uint32_t *view_count, uint32_t *match_i, uint32_t *match_j,
                         uint32_t *match_d, uint64_t cap) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_putative_read: null map");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  std::vector<uint32_t> cnt(m->n_views);
  SFM_RC(c->d_view_count.read(cnt.data(), cnt.size(), cs));
  if (view_count) memcpy(view_count, cnt.data(), cnt.size() * sizeof(uint32_t));
  if (match_i || match_j || match_d) {
    SFM_CHECK(cap >= m->n_rows, SFMLOC_ECAP, "sfmloc_putative_read: cap %llu < n_rows %llu", (unsigned long long)cap,
              (unsigned long long)m->n_rows);
    std::vector<uint32_t> hi(m->n_rows), hk(m->n_rows);
    SFM_RC(c->d_match_i.read(hi.data(), hi.size(), cs));
    SFM_RC(c->d_match_key.read(hk.data(), hk.size(), cs));
    for (uint32_t v = 0; v < m->n_views; ++v) {
      const uint32_t off = m->h_view_off[v];
      for (uint32_t k = 0; k < cnt[v]; ++k) {
        if (match_i) match_i[off + k] = hi[off + k];
        if (match_j) match_j[off + k] = hk[off + k] & 0xFFFFu;
        if (match_d) match_d[off + k] = hk[off + k] >> 16;
      }
    }
  }
  return SFMLOC_OK;
}

int sfmloc_putative_read_rows(sfmloc_map *map, uint32_t *best0, uint32_t *best1) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_putative_read_rows: null map");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  SFM_HIP(hipStreamSynchronize(cs));
  for (uint64_t r = 0; r < m->n_rows; ++r) {
    if (best0) best0[r] = SFMLOC_NOMATCH;
    if (best1) best1[r] = SFMLOC_NOMATCH;
  }
  if (c->last_nq == 0 || c->last_n_sel == 0 || c->last_split == 0 || c->last_n_work_blocks == 0) return SFMLOC_OK;
  const uint64_t nwb = c->last_n_work_blocks;
  std::vector<uint2> part((size_t)c->last_split * nwb * 64);
  SFM_RC(c->d_part.read(part.data(), part.size(), cs));
  std::vector<unsigned long long> mask;
  if (c->last_screened) {  // only the rows the screening scan could not reject have a pair; the others stay NOMATCH
    mask.resize(nwb);
    SFM_RC(c->d_flagmask.read(mask.data(), nwb, cs));
  }
  auto push = [](uint32_t &b0, uint32_t &b1, uint32_t k) {
    if (k < b0) {
      b1 = b0;
      b0 = k;
    } else if (k < b1) {
      b1 = k;
    }
  };
  if (c->last_blocks_on_device) {  // the list was built on the device (BoW shortlist); padding names no block
    c->last_blocks.resize(nwb);
    SFM_RC(c->d_block_list.read(c->last_blocks.data(), nwb, cs));
    c->last_blocks_on_device = false;
  }
  for (uint64_t w = 0; w < nwb; ++w) {
    const uint32_t blk = c->last_all_views ? (uint32_t)w : c->last_blocks[w];
    if (blk == 0xFFFFFFFFu) continue;
    for (uint32_t l = 0; l < kBlockRows; ++l) {
      const uint64_t r = (uint64_t)blk * kBlockRows + l;
      if (r >= m->n_rows) break;
      if (c->last_screened && !((mask[w] >> l) & 1ull)) continue;
      uint32_t b0 = SFMLOC_NOMATCH, b1 = SFMLOC_NOMATCH;
      for (uint32_t s = 0; s < c->last_split; ++s) {
        const uint2 p = part[((size_t)s * nwb + w) * 64 + l];
        push(b0, b1, p.x);
        push(b0, b1, p.y);
      }
      if (best0) best0[r] = b0;
      if (best1) best1[r] = b1;
    }
  }
  return SFMLOC_OK;
}

int sfmloc_geometric_filter(sfmloc_map *map, sfmloc_query *query) {
  SFM_CHECK(map && query, SFMLOC_EINVAL, "sfmloc_geometric_filter: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Query *q = reinterpret_cast<Query *>(query);
  int rc = check_stage(m->ctx0, q, "sfmloc_geometric_filter");
  if (rc) return rc;
  SFM_HIP(hipSetDevice(m->device));
  QueryPass pass;
  return ctx_geometric_filter(m->ctx0, q, pass);
}

int sfmloc_geometric_read(sfmloc_map *map, uint32_t *geo_count, uint32_t *geo_idx, uint64_t cap) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_geometric_read: null map");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  std::vector<uint32_t> cnt(m->n_views);
  SFM_RC(c->d_geo_count.read(cnt.data(), cnt.size(), cs));
  if (geo_count) memcpy(geo_count, cnt.data(), cnt.size() * sizeof(uint32_t));
  if (geo_idx) {
    SFM_CHECK(!c->geo_is_pairs, SFMLOC_EINVAL,
              "sfmloc_geometric_read: guided matches are not indices into the putative lists; use sfmloc_geometric_read_pairs");
    SFM_CHECK(cap >= m->n_rows, SFMLOC_ECAP, "sfmloc_geometric_read: cap too small");
    std::vector<uint32_t> gi(m->n_rows);
    SFM_RC(c->d_geo_idx.read(gi.data(), gi.size(), cs));
    for (uint32_t v = 0; v < m->n_views; ++v)
      for (uint32_t k = 0; k < cnt[v]; ++k) geo_idx[m->h_view_off[v] + k] = gi[m->h_view_off[v] + k];
  }
  int st = 0;
  SFM_RC(dev_read(&st, c->d_status, 1, cs));
  SFM_CHECK((st & 1) == 0, SFMLOC_ECAP, "a view has more than 65536 putative matches");
  return SFMLOC_OK;
}

int sfmloc_geometric_read_pairs(sfmloc_map *map, uint32_t *geo_count, uint32_t *geo_i, uint32_t *geo_j, uint64_t cap) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_geometric_read_pairs: null map");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  std::vector<uint32_t> cnt(m->n_views);
  SFM_RC(c->d_geo_count.read(cnt.data(), cnt.size(), cs));
  if (geo_count) memcpy(geo_count, cnt.data(), cnt.size() * sizeof(uint32_t));
  if (geo_i || geo_j) {
    SFM_CHECK(cap >= m->n_rows, SFMLOC_ECAP, "sfmloc_geometric_read_pairs: cap too small");
    std::vector<uint32_t> gi(m->n_rows), gj;
    SFM_RC(c->d_geo_idx.read(gi.data(), gi.size(), cs));
    std::vector<uint32_t> pi, pk;
    if (c->geo_is_pairs) {
      gj.resize(m->n_rows);
      SFM_RC(c->d_geo_j.read(gj.data(), gj.size(), cs));
    } else {  // indices into the putative lists: resolve them
      pi.resize(m->n_rows);
      pk.resize(m->n_rows);
      SFM_RC(c->d_match_i.read(pi.data(), pi.size(), cs));
      SFM_RC(c->d_match_key.read(pk.data(), pk.size(), cs));
    }
    for (uint32_t v = 0; v < m->n_views; ++v) {
      const uint32_t off = m->h_view_off[v];
      for (uint32_t k = 0; k < cnt[v]; ++k) {
        const uint32_t g = gi[off + k];
        if (geo_i) geo_i[off + k] = c->geo_is_pairs ? g : pi[off + g];
        if (geo_j) geo_j[off + k] = c->geo_is_pairs ? gj[off + k] : (pk[off + g] & 0xFFFFu);
      }
    }
  }
  return SFMLOC_OK;
}

int sfmloc_match_set(sfmloc_map *map, sfmloc_query *query) {
  SFM_CHECK(map && query, SFMLOC_EINVAL, "sfmloc_match_set: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Query *q = reinterpret_cast<Query *>(query);
  int rc = check_stage(m->ctx0, q, "sfmloc_match_set");
  if (rc) return rc;
  SFM_HIP(hipSetDevice(m->device));
  rc = ctx_set_query_camera(m->ctx0, q, "sfmloc_match_set");
  if (rc) return rc;
  rc = ctx_p3p_reserve(m->ctx0, q->n);  // K5's start runs at the end of this stage (k_match_set_finish)
  if (rc) return rc;
  return ctx_match_set(m->ctx0, q, QueryPass{});
}

int sfmloc_match_set_read(sfmloc_map *map, uint32_t *n, uint32_t *qfeat, uint32_t *landmark_id, double *pt2d,
                          double *pt3d, uint32_t cap) {
  SFM_CHECK(map && n, SFMLOC_EINVAL, "sfmloc_match_set_read: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  uint32_t k = 0;
  SFM_RC(c->d_ms_n.read(&k, 1, cs));
  *n = k;
  int st = 0;
  SFM_RC(dev_read(&st, c->d_status, 1, cs));
  SFM_CHECK((st & 2) == 0, SFMLOC_ECAP, "more than %u 2D-3D candidates (match-set workspace)", c->cand_cap);
  if (k == 0) return SFMLOC_OK;
  SFM_CHECK(cap >= k, SFMLOC_ECAP, "sfmloc_match_set_read: cap %u < %u", cap, k);
  if (qfeat) SFM_RC(c->d_ms_qfeat.read(qfeat, k, cs));
  if (landmark_id) SFM_RC(c->d_ms_landmark.read(landmark_id, k, cs));
  if (pt2d) SFM_RC(c->d_pt2d.read(pt2d, (size_t)k * 2, cs));
  if (pt3d) SFM_RC(c->d_pt3d.read(pt3d, (size_t)k * 3, cs));
  return SFMLOC_OK;
}

int sfmloc_resection(sfmloc_map *map, sfmloc_query *query) {
  SFM_CHECK(map && query, SFMLOC_EINVAL, "sfmloc_resection: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Query *q = reinterpret_cast<Query *>(query);
  Ctx *c = m->ctx0;
  int rc = check_stage(c, q, "sfmloc_resection");
  if (rc) return rc;
  SFM_HIP(hipSetDevice(m->device));
  rc = ctx_set_query_camera(c, q, "sfmloc_resection");
  if (rc) return rc;
  rc = ctx_p3p_reserve(c, q->n);
  if (rc) return rc;
  {
    EventScope ev(c, SFMLOC_K_P3P);
    rc = ctx_resection_enqueue(c, true);
  }
  if (rc) return rc;
  rc = ctx_fetch_result(c);
  if (rc) return rc;
  return ctx_resection_wait(c);
}

int sfmloc_pose_read(sfmloc_map *map, sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark,
                     uint32_t *inlier_idx, uint32_t cap) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_pose_read: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_HIP(hipSetDevice(m->device));
  const hipStream_t cs = c->stream;
  SFM_RC(dev_read(out, c->d_pose, 1, cs));
  SFM_CHECK((out->status & 4) == 0, SFMLOC_ECAP, "more than %u 2D-3D correspondences (P3P workspace)", c->p3p_cap);
  if (out->ok && out->n_inliers > 0) {
    const uint32_t k = (uint32_t)out->n_inliers;
    if (pair_qfeat || pair_landmark || inlier_idx)
      SFM_CHECK(cap >= k, SFMLOC_ECAP, "sfmloc_pose_read: cap %u < %u inliers", cap, k);
    if (pair_qfeat) SFM_RC(dev_read(pair_qfeat, c->d_pair_qfeat, k, cs));
    if (pair_landmark)
      SFM_RC(dev_read(pair_landmark, c->d_pair_landmark, k, cs));
    if (inlier_idx) SFM_RC(c->d_inlier_idx.read(inlier_idx, k, cs));
  }
  return SFMLOC_OK;
}

// ----- whole queries --------------------------------------------------------------------------------

int sfmloc_localize_begin(sfmloc_context *ctx, sfmloc_query *query, const uint32_t *view_sel, uint32_t n_sel) {
  SFM_CHECK(ctx && query, SFMLOC_EINVAL, "sfmloc_localize_begin: null argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  SFM_CHECK(q->map == c->map, SFMLOC_EINVAL, "sfmloc_localize_begin: query belongs to another map");
  SFM_HIP(hipSetDevice(c->map->device));
  QueryPass pass;
  return ctx_localize_begin(c, q, pass, ViewSel::host(view_sel, n_sel));
}

int sfmloc_localize_bow_begin(sfmloc_context *ctx, sfmloc_query *query, const float *query_bow, uint32_t knn,
                              const uint32_t *cand_views, uint32_t n_cand) {
  SFM_CHECK(ctx && query, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: null argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  Map *m = c->map;
  SFM_CHECK(query_bow || q->d_bow, SFMLOC_EINVAL,
            "sfmloc_localize_bow_begin: no BoW vector (pass one, or make it resident with sfmloc_query_set_bow)");
  SFM_CHECK(q->map == m, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: query belongs to another map");
  SFM_CHECK(m->bow_dim > 0 && m->d_bow, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: the map has no .bow vectors");
  SFM_CHECK(c->in_flight == nullptr, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: context already has a query in flight");
  SFM_CHECK(!c->merge_only, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: this context was created for sfmloc_merge_begin only");
  if (!cand_views) n_cand = m->n_views;
  SFM_CHECK(n_cand <= m->n_views, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: n_cand > n_views");
  SFM_HIP(hipSetDevice(m->device));
  // "if (knnbow > 0 && viewList.size() > knnbow)" (localization.cpp:346, LocalizeEngine.cc:342): otherwise every
  // candidate is matched
  QueryPass pass;
  if (knn == 0 || n_cand <= knn) return ctx_localize_begin(c, q, pass, ViewSel::host(cand_views, n_cand));
  if (cand_views) {
    for (uint32_t i = 0; i < n_cand; ++i) {
      SFM_CHECK(cand_views[i] < m->n_views, SFMLOC_EINVAL, "sfmloc_localize_bow_begin: view index out of range");
      SFM_CHECK(i == 0 || cand_views[i - 1] < cand_views[i], SFMLOC_EINVAL,
                "sfmloc_localize_bow_begin: candidate views must be strictly ascending");
    }
    SFM_RC(c->d_bow_cand.upload(cand_views, n_cand, c->stream));
  }
  if (query_bow)
    SFM_RC(c->d_bow_query.upload(query_bow, m->bow_dim, c->stream));
  int rc;
  {
    EventScope ev(c, SFMLOC_K_BOW);
    // the workgroup that finishes the shortlist also clears the query's counters and builds the block list
    const ChainArgs chain = make_chain_args(c, q, c->d_bow_sel, knn);
    rc = launch_bow_select(c, query_bow ? c->d_bow_query : q->d_bow, cand_views ? c->d_bow_cand : nullptr,
                           n_cand, knn, c->d_bow_dist, c->d_bow_sel, &chain);
  }
  if (rc) return rc;
  // K8 leaves the knn views in ascending order in d_bow_sel; everything downstream reads the selection on the device
  pass.chain_done = true;
  return ctx_localize_begin(c, q, pass, ViewSel::device(c->d_bow_sel, knn));
}

int sfmloc_localize_end(sfmloc_context *ctx, sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark,
                        uint32_t cap) {
  SFM_CHECK(ctx && out, SFMLOC_EINVAL, "sfmloc_localize_end: null argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  return ctx_localize_end(c, out, pair_qfeat, pair_landmark, cap);
}

// ----- sharded maps: one process per GPU, bank sharded by view ------------------------------

uint64_t sfmloc_part_bytes(uint32_t cap) { return (uint64_t)kPartHeaderBytes + (uint64_t)cap * sizeof(Candidate); }

int sfmloc_shard_begin(sfmloc_context *ctx, sfmloc_query *query, const uint32_t *view_sel, uint32_t n_sel) {
  SFM_CHECK(ctx && query, SFMLOC_EINVAL, "sfmloc_shard_begin: null argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  int rc = check_sharded(c, q, "sfmloc_shard_begin");
  if (rc) return rc;
  SFM_HIP(hipSetDevice(c->map->device));
  ctx_mark_busy(c);  // until sfmloc_context_sync
  QueryPass pass;
  rc = ctx_match_and_filter(c, q, pass, ViewSel::host(view_sel, n_sel), "sfmloc_shard_begin");
  if (rc) return rc;
  EventScope ev(c, SFMLOC_K_MATCHSET);
  return launch_emit_candidates(c, q, pass, c->last_n_sel, c->last_all_views);
}

int sfmloc_shard_export(sfmloc_context *ctx, void *dst_dev, uint32_t cap) {
  SFM_CHECK(ctx && dst_dev && cap > 0, SFMLOC_EINVAL, "sfmloc_shard_export: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  // header (with the true count: the merging side flags count > cap) + the candidates that exist, at most cap
  return launch_export_part(c, dst_dev, cap < c->cand_cap ? cap : c->cand_cap);
}

int sfmloc_shard_bow_keys(sfmloc_context *ctx, sfmloc_query *query, const float *query_bow, uint32_t knn,
                          void *keys_dev) {
  SFM_CHECK(ctx && query && keys_dev && knn > 0, SFMLOC_EINVAL, "sfmloc_shard_bow_keys: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  Map *m = c->map;
  int rc = check_sharded(c, q, "sfmloc_shard_bow_keys", /*in_flight=*/false);
  if (rc) return rc;
  SFM_CHECK(m->bow_dim > 0 && m->d_bow, SFMLOC_EINVAL, "sfmloc_shard_bow_keys: the map has no .bow vectors");
  SFM_CHECK(query_bow || q->d_bow, SFMLOC_EINVAL, "sfmloc_shard_bow_keys: no BoW vector");
  SFM_CHECK(c->in_flight == nullptr, SFMLOC_EINVAL, "sfmloc_shard_bow_keys: context has a query in flight");
  SFM_CHECK(knn <= 1024, SFMLOC_EINVAL, "sfmloc_shard_bow_keys: knn %u > 1024", knn);
  SFM_HIP(hipSetDevice(m->device));
  ctx_mark_busy(c);
  if (query_bow)
    SFM_RC(c->d_bow_query.upload(query_bow, m->bow_dim, c->stream));
  EventScope ev(c, SFMLOC_K_BOW);
  return launch_bow_keys(c, query_bow ? c->d_bow_query : q->d_bow, knn, c->d_bow_dist, c->d_bow_cand,
                         reinterpret_cast<unsigned long long *>(keys_dev));
}

int sfmloc_shard_begin_bow(sfmloc_context *ctx, sfmloc_query *query, const void *keys_dev, uint32_t n_parts,
                           uint64_t part_stride_keys, uint32_t knn) {
  SFM_CHECK(ctx && query && keys_dev && n_parts > 0 && knn > 0, SFMLOC_EINVAL, "sfmloc_shard_begin_bow: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  Map *m = c->map;
  int rc = check_sharded(c, q, "sfmloc_shard_begin_bow");
  if (rc) return rc;
  SFM_CHECK(!c->merge_only, SFMLOC_EINVAL, "sfmloc_shard_begin_bow: this context was created for sfmloc_merge_begin only");
  if (part_stride_keys == 0) part_stride_keys = knn;
  SFM_CHECK(part_stride_keys >= knn, SFMLOC_EINVAL, "sfmloc_shard_begin_bow: part_stride_keys < knn");
  SFM_CHECK(m->bow_dim > 0 && c->d_bow_sel, SFMLOC_EINVAL, "sfmloc_shard_begin_bow: the map has no BoW vectors");
  SFM_HIP(hipSetDevice(m->device));
  ctx_mark_busy(c);  // until sfmloc_context_sync
  // this shard's part of the global knn best: ascending local view indices, padded with the phantom view up to
  // n_pad = min(knn, n_views) entries -- the launch sizes below depend on n_pad only, never on the outcome
  const uint32_t n_pad = knn < m->n_views ? knn : m->n_views;
  {
    EventScope ev(c, SFMLOC_K_BOW);
    // the workgroup that merges the key lists also clears the query's counters and builds the block list
    const ChainArgs chain = make_chain_args(c, q, c->d_bow_sel, n_pad);
    rc = launch_bow_merge_select(c, reinterpret_cast<const unsigned long long *>(keys_dev), n_parts,
                                 part_stride_keys, knn, n_pad, c->d_bow_sel, n_pad ? &chain : nullptr);
  }
  if (rc) return rc;
  QueryPass pass;
  pass.chain_done = n_pad != 0;
  rc = ctx_match_and_filter(c, q, pass, ViewSel::device(c->d_bow_sel, n_pad), "sfmloc_shard_begin_bow");
  if (rc) return rc;
  EventScope ev(c, SFMLOC_K_MATCHSET);
  return launch_emit_candidates(c, q, pass, c->last_n_sel, c->last_all_views);
}

int sfmloc_context_signal(sfmloc_context *ctx, void *hip_stream) {
  SFM_CHECK(ctx, SFMLOC_EINVAL, "sfmloc_context_signal: null context");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  SFM_HIP(hipEventRecord(c->xev_out, c->stream));
  SFM_HIP(hipStreamWaitEvent(reinterpret_cast<hipStream_t>(hip_stream), c->xev_out, 0));
  return SFMLOC_OK;
}

int sfmloc_context_wait(sfmloc_context *ctx, void *hip_stream) {
  SFM_CHECK(ctx, SFMLOC_EINVAL, "sfmloc_context_wait: null context");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  SFM_HIP(hipEventRecord(c->xev_in, reinterpret_cast<hipStream_t>(hip_stream)));
  SFM_HIP(hipStreamWaitEvent(c->stream, c->xev_in, 0));
  return SFMLOC_OK;
}

int sfmloc_gang_begin(sfmloc_context *const *ctxs, uint32_t n) {
  SFM_CHECK(ctxs && n >= 1 && n <= (uint32_t)kGangMembers, SFMLOC_EINVAL, "sfmloc_gang_begin: 1..%d contexts", kGangMembers);
  Ctx *lead = reinterpret_cast<Ctx *>(ctxs[0]);
  SFM_CHECK(lead, SFMLOC_EINVAL, "sfmloc_gang_begin: null context");
  for (uint32_t i = 0; i < n; ++i) {
    Ctx *c = reinterpret_cast<Ctx *>(ctxs[i]);
    SFM_CHECK(c && c->map == lead->map, SFMLOC_EINVAL, "sfmloc_gang_begin: the contexts belong to different maps");
    SFM_CHECK(c->stream.gang == nullptr, SFMLOC_EINVAL, "sfmloc_gang_begin: context %u is already in a gang session", i);
    for (uint32_t j = 0; j < i; ++j) SFM_CHECK(ctxs[j] != ctxs[i], SFMLOC_EINVAL, "sfmloc_gang_begin: context listed twice");
  }
  // (stage brackets are events on the stream around every launch: with profiling on, the session records nothing and the
  // members simply run one after the other)
  if (n == 1 || lead->map->params.profile != 0) return SFMLOC_OK;
  SFM_HIP(hipSetDevice(lead->map->device));
  GangMember *ms[kGangMembers];
  for (uint32_t i = 0; i < n; ++i) ms[i] = reinterpret_cast<Ctx *>(ctxs[i]);
  return gang_open(ms, (int)n);
}

int sfmloc_gang_end(sfmloc_context *const *ctxs, uint32_t n) {
  SFM_CHECK(ctxs && n >= 1 && n <= (uint32_t)kGangMembers && ctxs[0], SFMLOC_EINVAL, "sfmloc_gang_end: 1..%d contexts", kGangMembers);
  Ctx *lead = reinterpret_cast<Ctx *>(ctxs[0]);
  GangState *g = lead->stream.gang;
  if (!g) return SFMLOC_OK;  // the session recorded nothing (one member, or profiling)
  SFM_CHECK(g == lead->gang_owned.get() && g->members.size() == n, SFMLOC_EINVAL, "sfmloc_gang_end: not the contexts of the session");
  SFM_HIP(hipSetDevice(lead->map->device));
  return gang_close(lead);
}

int sfmloc_gang_counters(sfmloc_context *lead_ctx, uint64_t *launches, uint64_t *gang_launches) {
  SFM_CHECK(lead_ctx, SFMLOC_EINVAL, "sfmloc_gang_counters: null context");
  Ctx *c = reinterpret_cast<Ctx *>(lead_ctx);
  if (launches) *launches = c->gang_owned ? c->gang_owned->launches : 0;
  if (gang_launches) *gang_launches = c->gang_owned ? c->gang_owned->gang_launches : 0;
  return SFMLOC_OK;
}

int sfmloc_context_sync(sfmloc_context *ctx) {
  SFM_CHECK(ctx, SFMLOC_EINVAL, "sfmloc_context_sync: null context");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  SFM_HIP(hipStreamSynchronize(c->stream));
  c->stream.dirty = false;
  if (c->in_flight == nullptr) ctx_mark_idle(c);
  return SFMLOC_OK;
}

uint64_t sfmloc_packed_bytes(uint32_t n_queries, uint32_t budget) { return packed_part_bytes(n_queries, budget); }

int sfmloc_shard_export_packed(sfmloc_context *ctx, void *packed_dev, uint32_t n_queries, uint32_t budget,
                               uint32_t query_index) {
  SFM_CHECK(ctx && packed_dev && n_queries > 0 && query_index < n_queries, SFMLOC_EINVAL,
            "sfmloc_shard_export_packed: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_HIP(hipSetDevice(c->map->device));
  return launch_export_packed(c, packed_dev, n_queries, budget, query_index);
}

static int merge_begin_impl(sfmloc_context *ctx, sfmloc_query *query, const void *parts_dev, uint32_t n_parts,
                            uint32_t cap, uint64_t part_stride, uint32_t packed_b, uint32_t packed_qi) {
  SFM_CHECK(ctx && query && parts_dev && n_parts > 0 && cap > 0, SFMLOC_EINVAL, "sfmloc_merge_begin: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  Query *q = reinterpret_cast<Query *>(query);
  Map *m = c->map;
  int rc = check_sharded(c, q, "sfmloc_merge_begin");
  if (rc) return rc;
  SFM_CHECK(m->focal > 0.0, SFMLOC_EINVAL, "sfmloc_merge_begin: the map has no intrinsic");
  SFM_CHECK(q->n == 0 || q->d_kpt, SFMLOC_EINVAL, "sfmloc_merge_begin: the query was created without keypoints");
  if (part_stride == 0) part_stride = sfmloc_part_bytes(cap);
  SFM_CHECK(packed_b || part_stride >= sfmloc_part_bytes(cap), SFMLOC_EINVAL, "sfmloc_merge_begin: part_stride too small");
  SFM_HIP(hipSetDevice(m->device));
  c->t_begin = now_s();
  // (counted like a begun localisation: with other contexts' work queued -- the next batch's stage 1, always, in the
  // pipeline of dist.py -- K5 takes its shared-GPU round sizes; sfmloc_localize_end uncounts)
  ctx_mark_busy(c);
  {
    c->p3p_uncal = false;  // (refused above; the context may have served an uncalibrated query before)
    const int rcr = ctx_p3p_reserve(c, q->n);
    if (rcr) {
      ctx_mark_idle(c);
      return rcr;
    }
  }
  {
    EventScope ev(c, SFMLOC_K_MATCHSET);
    rc = launch_select_candidates(c, q, QueryPass{}, reinterpret_cast<const unsigned char *>(parts_dev), n_parts, part_stride,
                                  cap, packed_b, packed_qi, /*reset_status=*/true);
  }
  if (!rc) {
    EventScope ev(c, SFMLOC_K_P3P);
    rc = ctx_resection_enqueue(c, true);
  }
  if (!rc) rc = ctx_fetch_result(c);
  if (rc) {
    ctx_mark_idle(c);
    return rc;
  }
  c->in_flight = q;
  return SFMLOC_OK;
}

int sfmloc_merge_begin(sfmloc_context *ctx, sfmloc_query *query, const void *parts_dev, uint32_t n_parts,
                       uint32_t cap, uint64_t part_stride) {
  return merge_begin_impl(ctx, query, parts_dev, n_parts, cap, part_stride, 0, 0);
}

int sfmloc_merge_begin_packed(sfmloc_context *ctx, sfmloc_query *query, const void *packed_dev, uint32_t n_parts,
                              uint64_t part_stride, uint32_t n_queries, uint32_t budget, uint32_t query_index) {
  SFM_CHECK(n_queries > 0 && query_index < n_queries && budget > 0, SFMLOC_EINVAL,
            "sfmloc_merge_begin_packed: bad argument");
  if (part_stride == 0) part_stride = packed_part_bytes(n_queries, budget);
  SFM_CHECK(part_stride >= packed_part_bytes(n_queries, budget), SFMLOC_EINVAL,
            "sfmloc_merge_begin_packed: part_stride too small");
  SFM_CHECK((uint64_t)n_parts * budget < (1ull << 32), SFMLOC_EINVAL, "sfmloc_merge_begin_packed: n_parts * budget >= 2^32");
  return merge_begin_impl(ctx, query, packed_dev, n_parts, budget, part_stride, n_queries, query_index);
}

int sfmloc_localize(sfmloc_map *map, sfmloc_query *query, const uint32_t *view_sel, uint32_t n_sel,
                    sfmloc_pose *out, uint32_t *pair_qfeat, uint32_t *pair_landmark, uint32_t cap) {
  SFM_CHECK(map && query && out, SFMLOC_EINVAL, "sfmloc_localize: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Query *q = reinterpret_cast<Query *>(query);
  SFM_CHECK(q->map == m, SFMLOC_EINVAL, "sfmloc_localize: query belongs to another map");
  SFM_HIP(hipSetDevice(m->device));
  QueryPass pass;
  int rc = ctx_localize_begin(m->ctx0, q, pass, ViewSel::host(view_sel, n_sel));
  if (rc) {
    m->ctx0->in_flight = nullptr;
    return rc;
  }
  return ctx_localize_end(m->ctx0, out, pair_qfeat, pair_landmark, cap);
}

int sfmloc_localize_bow(sfmloc_map *map, sfmloc_query *query, const float *query_bow, uint32_t knn,
                        const uint32_t *cand_views, uint32_t n_cand, sfmloc_pose *out, uint32_t *pair_qfeat,
                        uint32_t *pair_landmark, uint32_t cap) {
  SFM_CHECK(map && query && out, SFMLOC_EINVAL, "sfmloc_localize_bow: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  int rc = sfmloc_localize_bow_begin(reinterpret_cast<sfmloc_context *>(m->ctx0), query, query_bow, knn, cand_views, n_cand);
  if (rc) {
    m->ctx0->in_flight = nullptr;
    return rc;
  }
  return ctx_localize_end(m->ctx0, out, pair_qfeat, pair_landmark, cap);
}

int sfmloc_localize_batch(sfmloc_map *map, sfmloc_query *const *queries, uint32_t n, uint32_t n_contexts,
                          sfmloc_pose *poses, uint32_t *pair_qfeat, uint32_t *pair_landmark, uint32_t pair_stride) {
  SFM_CHECK(map && (n == 0 || (queries && poses)), SFMLOC_EINVAL, "sfmloc_localize_batch: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  if (n_contexts == 0) n_contexts = 4;
  if (n_contexts > n) n_contexts = n ? n : 1;
  while (m->batch_ctx.size() < n_contexts) {
    Ctx *c = nullptr;
    int rc = make_ctx(m, &c);
    if (rc) return rc;
    m->pool.push_back(c);
    m->batch_ctx.push_back(c);
  }
  int first_err = SFMLOC_OK;
  auto finish = [&](uint32_t i) {
    Ctx *c = m->batch_ctx[i % n_contexts];
    int rc = ctx_localize_end(c, &poses[i], pair_qfeat ? pair_qfeat + (size_t)i * pair_stride : nullptr,
                              pair_landmark ? pair_landmark + (size_t)i * pair_stride : nullptr, pair_stride);
    if (rc && !first_err) first_err = rc;
  };
  for (uint32_t i = 0; i < n; ++i) {
    if (i >= n_contexts) finish(i - n_contexts);
    Ctx *c = m->batch_ctx[i % n_contexts];
    Query *q = reinterpret_cast<Query *>(queries[i]);
    QueryPass pass;
    int rc = (q && q->map == m) ? ctx_localize_begin(c, q, pass, ViewSel{}) : SFMLOC_EINVAL;
    if (rc) {
      if (!first_err) {
        first_err = rc;
        if (!(q && q->map == m)) set_error("sfmloc_localize_batch: query %u is null or belongs to another map", i);
      }
      // drain what is in flight and stop
      for (uint32_t k = (i >= n_contexts ? i - n_contexts + 1 : 0); k < i; ++k) finish(k);
      return first_err;
    }
  }
  for (uint32_t k = (n >= n_contexts ? n - n_contexts : 0); k < n; ++k) finish(k);
  return first_err;
}

// ----- BoW shortlist ---------------------------------------------------------------------------------------

int sfmloc_bow_select(sfmloc_map *map, const float *query_bow, const uint32_t *cand_views, uint32_t n_cand,
                      uint32_t k, uint32_t *out_sel, uint32_t *n_out) {
  SFM_CHECK(map && query_bow && out_sel && n_out, SFMLOC_EINVAL, "sfmloc_bow_select: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_CHECK(m->bow_dim > 0 && m->d_bow, SFMLOC_EINVAL, "sfmloc_bow_select: the map has no .bow vectors");
  if (!cand_views) n_cand = m->n_views;
  SFM_CHECK(n_cand <= m->n_views, SFMLOC_EINVAL, "sfmloc_bow_select: n_cand > n_views");
  // CV_Assert(knn < viewList.size()) (BoFUtils.cpp:30)
  SFM_CHECK(k < n_cand, SFMLOC_EINVAL, "sfmloc_bow_select: knn %u must be smaller than the %u candidate views", k,
            n_cand);
  SFM_HIP(hipSetDevice(m->device));
  if (cand_views) {
    for (uint32_t i = 0; i < n_cand; ++i) {
      SFM_CHECK(cand_views[i] < m->n_views, SFMLOC_EINVAL, "sfmloc_bow_select: view index out of range");
      SFM_CHECK(i == 0 || cand_views[i - 1] < cand_views[i], SFMLOC_EINVAL,
                "sfmloc_bow_select: candidate views must be strictly ascending");
    }
    SFM_RC(c->d_bow_cand.upload(cand_views, n_cand, c->stream));
  }
  SFM_RC(c->d_bow_query.upload(query_bow, m->bow_dim, c->stream));
  int rc;
  {
    EventScope ev(c, SFMLOC_K_BOW);
    rc = launch_bow_select(c, c->d_bow_query, cand_views ? c->d_bow_cand : nullptr, n_cand, k,
                           c->d_bow_dist, c->d_bow_sel);
  }
  if (rc) return rc;
  SFM_RC(c->d_bow_sel.download(out_sel, k, c->stream));
  SFM_HIP(hipStreamSynchronize(c->stream));
  *n_out = k;
  return SFMLOC_OK;
}

int sfmloc_bow_distances(sfmloc_map *map, const float *query_bow, float *out_dist) {
  SFM_CHECK(map && query_bow && out_dist, SFMLOC_EINVAL, "sfmloc_bow_distances: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_CHECK(m->bow_dim > 0 && m->d_bow, SFMLOC_EINVAL, "sfmloc_bow_distances: the map has no .bow vectors");
  SFM_HIP(hipSetDevice(m->device));
  if (m->n_views == 0) return SFMLOC_OK;
  SFM_RC(c->d_bow_query.upload(query_bow, m->bow_dim, c->stream));
  int rc;
  {
    EventScope ev(c, SFMLOC_K_BOW);
    rc = launch_bow_select(c, c->d_bow_query, nullptr, m->n_views, 1, c->d_bow_dist, c->d_bow_sel);
  }
  if (rc) return rc;
  // the kernel stores the float32 distance's bit pattern (non-negative floats order like their bits)
  SFM_RC(c->d_bow_dist.download(out_dist, m->n_views, c->stream));
  SFM_HIP(hipStreamSynchronize(c->stream));
  return SFMLOC_OK;
}

int sfmloc_bof_create(const sfmloc_bof_desc *d, int device, sfmloc_bof **out) {
  SFM_CHECK(d && out, SFMLOC_EINVAL, "sfmloc_bof_create: null argument");
  *out = nullptr;
  SFM_CHECK(d->K > 0 && d->centers && d->in_dim > 0 && d->in_dim <= 128, SFMLOC_EINVAL,
            "sfmloc_bof_create: bad model (K %d, in_dim %d)", d->K, d->in_dim);
  SFM_CHECK(d->pyramid_level >= 1 && d->pyramid_level <= 3, SFMLOC_EINVAL, "PYRAMID_LEVEL must be 1..3");
  SFM_CHECK(d->n_pca == 0 || (d->pca_mean && d->pca_eigvec && d->pca_eigval && d->n_pca <= 128), SFMLOC_EINVAL,
            "sfmloc_bof_create: PCA arrays missing");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV, "no HIP device visible; this library has no CPU fallback");
  SFM_HIP(hipSetDevice(device));
  return make_handle<BofModel>("sfmloc_bof_create", out, [&](BofModel *b) -> int {
    b->device = device;
    b->K = d->K;
    b->in_dim = d->in_dim;
    b->n_pca = d->n_pca;
    b->cdim = d->n_pca > 0 ? d->n_pca : d->in_dim;
    b->resized = d->resized_image_size;
    b->levels = d->use_spatial_pyramid ? d->pyramid_level : 1;
    b->norm_type = d->norm_type;
    b->cells = 0;
    for (int l = 0; l < b->levels; ++l) b->cells += (l == 0) ? 1 : (l == 2 ? 3 : (l + 1) * (l + 1));
    // (the model's own stream is created by the first sfmloc_bof_compute: a model inside a sfmloc_imgbow works on that
    // object's stream and needs none -- an idle stream still shares a hardware queue with streams that work; the uploads
    // here name no stream, so each has completed when it returns: devmem.h "Transfers")
    SFM_RC(dev_upload(nullptr, b->d_centers, d->centers, (size_t)d->K * b->cdim, nullptr));
    if (d->n_pca > 0) {
      SFM_RC(dev_upload(nullptr, b->d_pca_mean, d->pca_mean, (size_t)d->in_dim, nullptr));
      SFM_RC(dev_upload(nullptr, b->d_pca_evec, d->pca_eigvec, (size_t)d->n_pca * d->in_dim, nullptr));
      SFM_RC(dev_upload(nullptr, b->d_pca_eval, d->pca_eigval, (size_t)d->n_pca, nullptr));
    }
    SFM_RC(b->d_counts.alloc(nullptr, (size_t)b->K * b->cells));
    return b->d_out.alloc(nullptr, (size_t)b->K * b->cells);
  });
}

void sfmloc_bof_destroy(sfmloc_bof *bof) {
  BofModel *b = reinterpret_cast<BofModel *>(bof);
  if (!b) return;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  delete b;  // (devmem.h, order of destruction: its buffers, then its stream)
}

int sfmloc_bof_dim(const sfmloc_bof *bof) {
  const BofModel *b = reinterpret_cast<const BofModel *>(bof);
  return b ? b->K * b->cells : 0;
}

int sfmloc_bof_compute(sfmloc_bof *bof, const float *desc, const float *kpt_xy, uint32_t n, double *out_bow) {
  SFM_CHECK(bof && out_bow && (n == 0 || (desc && kpt_xy)), SFMLOC_EINVAL, "sfmloc_bof_compute: null argument");
  BofModel *b = reinterpret_cast<BofModel *>(bof);
  SFM_HIP(hipSetDevice(b->device));
  if ((size_t)n * 2 * sizeof(float) > b->d_kxy.bytes()) {  // (the pair grows together or not at all)
    DevGroup g(nullptr);
    g.add(b->d_desc, (size_t)n * b->in_dim);
    g.add(b->d_kxy, (size_t)n * 2);
    if (!g.ok()) return g.rc();
    g.commit();
  }
  SFM_RC(b->stream.ensure());
  if (n) {
    SFM_RC(b->d_desc.upload(desc, (size_t)n * b->in_dim, b->stream));
    SFM_RC(b->d_kxy.upload(kpt_xy, (size_t)n * 2, b->stream));
  }
  int rc = launch_bof(b, b->stream, b->d_desc, b->d_kxy, (int)n, b->d_counts, b->d_out, nullptr);  // (stream: created above)
  if (rc) return rc;
  SFM_RC(b->d_out.download(out_bow, (size_t)b->K * b->cells, b->stream));
  SFM_HIP(hipStreamSynchronize(b->stream));
  return SFMLOC_OK;
}

// ----- a rank's whole batch per call --------------------------------------------
// dist.py drove a batch with one ctypes call per query and stage (~2 ms of a 17 ms batch at N = 8); these take the
// batch's arrays and run the same per-query calls in gang sessions of `gang` contexts: query i goes to context
// i mod n_ctx, the contexts [g, g + gang) of every n_ctx consecutive queries form one session (the first of them leads),
// the sessions take turns so that their streams stay equally loaded -- exactly the order dist.HipShardCompute._rounds
// queued them in, so the results are the same bits.
}  // extern "C"
namespace {
template <class PerQuery>
int shard_batch_rounds(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, uint32_t n_queries, const char *who,
                       PerQuery per_query) {
  SFM_CHECK(ctxs && n_ctx > 0, SFMLOC_EINVAL, "%s: no contexts", who);
  if (gang == 0) gang = 1;
  if (gang > (uint32_t)kGangMembers) gang = kGangMembers;
  for (uint32_t base = 0; base < n_queries; base += n_ctx)
    for (uint32_t g0 = 0; g0 < n_ctx; g0 += gang) {
      uint32_t m = 0;
      for (uint32_t k = g0; k < n_ctx && k < g0 + gang && base + k < n_queries; ++k) ++m;
      if (m == 0) continue;
      int rc = m > 1 ? sfmloc_gang_begin(ctxs + g0, m) : SFMLOC_OK;
      for (uint32_t k = 0; k < m && rc == SFMLOC_OK; ++k) rc = per_query(ctxs[g0 + k], base + g0 + k);
      const int rc_end = m > 1 ? sfmloc_gang_end(ctxs + g0, m) : SFMLOC_OK;
      if (rc == SFMLOC_OK) rc = rc_end;
      if (rc) return rc;
    }
  return SFMLOC_OK;
}
}  // namespace
extern "C" {

int sfmloc_shard_batch_bow_keys(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                                uint32_t n_queries, uint32_t knn, void *keys_dev) {
  SFM_CHECK(queries && keys_dev && knn > 0, SFMLOC_EINVAL, "sfmloc_shard_batch_bow_keys: bad argument");
  return shard_batch_rounds(ctxs, n_ctx, gang, n_queries, "sfmloc_shard_batch_bow_keys", [&](sfmloc_context *c, uint32_t i) {
    return sfmloc_shard_bow_keys(c, queries[i], nullptr, knn, static_cast<unsigned char *>(keys_dev) + (size_t)i * knn * 8);
  });
}

int sfmloc_shard_batch_begin_bow(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                                 uint32_t n_queries, const void *keys_all_dev, uint32_t n_parts, uint32_t knn,
                                 void *packed_dev, uint32_t budget) {
  SFM_CHECK(queries && keys_all_dev && packed_dev && knn > 0 && n_parts > 0, SFMLOC_EINVAL,
            "sfmloc_shard_batch_begin_bow: bad argument");
  // keys_all [n_parts][n_queries][knn]: query i's lists start at i * knn keys, one part every n_queries * knn keys
  return shard_batch_rounds(ctxs, n_ctx, gang, n_queries, "sfmloc_shard_batch_begin_bow", [&](sfmloc_context *c, uint32_t i) {
    int rc = sfmloc_shard_begin_bow(c, queries[i], static_cast<const unsigned char *>(keys_all_dev) + (size_t)i * knn * 8,
                                    n_parts, (uint64_t)n_queries * knn, knn);
    if (!rc) rc = sfmloc_shard_export_packed(c, packed_dev, n_queries, budget, i);
    return rc;
  });
}

int sfmloc_shard_batch_begin(sfmloc_context *const *ctxs, uint32_t n_ctx, uint32_t gang, sfmloc_query *const *queries,
                             uint32_t n_queries, void *packed_dev, uint32_t budget) {
  SFM_CHECK(queries && packed_dev, SFMLOC_EINVAL, "sfmloc_shard_batch_begin: bad argument");
  return shard_batch_rounds(ctxs, n_ctx, gang, n_queries, "sfmloc_shard_batch_begin", [&](sfmloc_context *c, uint32_t i) {
    int rc = sfmloc_shard_begin(c, queries[i], nullptr, 0);
    if (!rc) rc = sfmloc_shard_export_packed(c, packed_dev, n_queries, budget, i);
    return rc;
  });
}

// stage 2 of up to kGangMembers queries in ONE session: context k takes query query_index[k] of the batch
int sfmloc_merge_batch_begin(sfmloc_context *const *ctxs, uint32_t n, sfmloc_query *const *queries, const uint32_t *query_index,
                             const void *packed_all_dev, uint32_t n_parts, uint64_t part_stride, uint32_t n_queries,
                             uint32_t budget) {
  SFM_CHECK(ctxs && queries && query_index && packed_all_dev && n > 0 && n <= (uint32_t)kGangMembers, SFMLOC_EINVAL,
            "sfmloc_merge_batch_begin: 1..%d contexts", kGangMembers);
  int rc = n > 1 ? sfmloc_gang_begin(ctxs, n) : SFMLOC_OK;
  for (uint32_t k = 0; k < n && rc == SFMLOC_OK; ++k)
    rc = sfmloc_merge_begin_packed(ctxs[k], queries[k], packed_all_dev, n_parts, part_stride, n_queries, budget, query_index[k]);
  const int rc_end = n > 1 ? sfmloc_gang_end(ctxs, n) : SFMLOC_OK;
  return rc ? rc : rc_end;
}

int sfmloc_debug_resect6(sfmloc_map *map, const double *pt2d, const double *pt3d, uint32_t n, uint32_t width,
                         uint32_t height, sfmloc_pose *out, uint32_t *inlier_idx, uint32_t cap) {
  SFM_CHECK(map && pt2d && pt3d && out && n > 0 && width > 0 && height > 0, SFMLOC_EINVAL, "sfmloc_debug_resect6: bad argument");
  SFM_CHECK(n <= 65536u, SFMLOC_EINVAL, "sfmloc_debug_resect6: more than 65536 correspondences");
  Map *m = reinterpret_cast<Map *>(map);
  Ctx *c = m->ctx0;
  SFM_CHECK(c->in_flight == nullptr && !c->stream.gang, SFMLOC_EINVAL, "sfmloc_debug_resect6: the map's context is busy");
  SFM_HIP(hipSetDevice(m->device));
  int rc = ctx_p3p_reserve(c, n);
  if (rc) return rc;
  std::vector<uint32_t> iota(n);
  for (uint32_t i = 0; i < n; ++i) iota[i] = i;
  const hipStream_t cs = c->stream;
  SFM_RC(c->d_pt2d.upload(pt2d, (size_t)n * 2, cs));
  SFM_RC(c->d_pt3d.upload(pt3d, (size_t)n * 3, cs));
  SFM_RC(c->d_ms_qfeat.upload(iota.data(), n, cs));
  SFM_RC(c->d_ms_landmark.upload(iota.data(), n, cs));
  SFM_RC(c->d_ms_n.upload(&n, 1, cs));
  SFM_HIP(hipStreamSynchronize(cs));  // (the caller's arrays, iota and n are pageable host memory)
  ctx_set_uncalibrated_camera(c, width, height);
  c->p3p_init_fused = false;  // K5's init reads the count written above
  rc = ctx_resection_begin(c);
  if (!rc) rc = ctx_resection_wait_done(c);
  c->p3p_uncal = false;
  if (rc) return rc;
  const HostResult *h = c->h_result;
  *out = h->pose;
  SFM_CHECK((out->status & 4) == 0, SFMLOC_ECAP, "more than %u 2D-3D correspondences (P3P workspace)", c->p3p_cap);
  if (inlier_idx && out->ok && out->n_inliers > 0) {
    SFM_CHECK(cap >= (uint32_t)out->n_inliers, SFMLOC_ECAP, "sfmloc_debug_resect6: cap %u < %d inliers", cap, out->n_inliers);
    SFM_RC(c->d_inlier_idx.read(inlier_idx, out->n_inliers, cs));
  }
  return SFMLOC_OK;
}

void sfmloc_debug_fail_p3p_alloc(int k) { sfmloc::g_test_fail_alloc.store(k, std::memory_order_relaxed); }
void sfmloc_debug_fail_next_alloc(int k) { sfmloc::g_fail_countdown = k; }

int sfmloc_debug_context_views(sfmloc_context *ctx, uint32_t *views, uint32_t cap, uint32_t *n) {
  SFM_CHECK(ctx && n && (views || cap == 0), SFMLOC_EINVAL, "sfmloc_debug_context_views: bad argument");
  Ctx *c = reinterpret_cast<Ctx *>(ctx);
  SFM_CHECK(!c->stream.gang, SFMLOC_EINVAL, "sfmloc_debug_context_views: the context is recording a gang session");
  SFM_HIP(hipSetDevice(c->map->device));
  const hipStream_t cs = c->stream;
  SFM_HIP(hipStreamSynchronize(cs));
  *n = c->last_n_sel;
  SFM_CHECK(cap >= c->last_n_sel, SFMLOC_ECAP, "sfmloc_debug_context_views: cap %u < %u views", cap, c->last_n_sel);
  if (c->last_all_views) {  // (no list on the device: every view, in order)
    for (uint32_t v = 0; v < c->last_n_sel; ++v) views[v] = v;
  } else if (c->last_n_sel) {
    SFM_RC(c->d_view_sel.read(views, c->last_n_sel, cs));
  }
  return SFMLOC_OK;
}

int sfmloc_debug_math(int device, int op, const double *in, int n, int in_stride, double *out, int out_stride) {
  SFM_CHECK(in && out && n > 0 && in_stride > 0 && out_stride > 0, SFMLOC_EINVAL, "sfmloc_debug_math: bad argument");
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV, "no HIP device visible; this library has no CPU fallback");
  SFM_HIP(hipSetDevice(device));
  DevBuf<double> d_in, d_out;
  int rc = d_in.alloc(nullptr, (size_t)n * in_stride);
  if (!rc) rc = d_out.alloc(nullptr, (size_t)n * out_stride);
  if (rc) return rc;
  rc = d_in.upload(in, (size_t)n * in_stride, nullptr);  // (a one-shot call without a stream: all of it on the null stream)
  if (!rc) rc = d_out.zero(nullptr);
  if (!rc) rc = launch_debug_math(op, d_in, n, in_stride, d_out, out_stride, nullptr);
  if (!rc) rc = d_out.read(out, (size_t)n * out_stride, nullptr);
  return rc;
}

int sfmloc_sync(sfmloc_map *map) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_sync: null map");
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  SFM_HIP(hipStreamSynchronize(m->ctx0->stream));
  for (Ctx *c : m->pool) SFM_HIP(hipStreamSynchronize(c->stream));
  return SFMLOC_OK;
}

int sfmloc_stats_read(sfmloc_map *map, sfmloc_kernel_stats *out) {
  SFM_CHECK(map && out, SFMLOC_EINVAL, "sfmloc_stats_read: null argument");
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  memset(out, 0, sizeof(*out));
  std::vector<Ctx *> all = m->pool;
  all.push_back(m->ctx0);
  for (Ctx *c : all) {
    const hipStream_t cs = c->stream;
    SFM_HIP(hipStreamSynchronize(cs));
    int rc = drain_events(c);
    if (rc) return rc;
    for (int k = 0; k < SFMLOC_K_COUNT; ++k) {
      out->total_ms[k] += c->stats.total_ms[k];
      out->launches[k] += c->stats.launches[k];
    }
    out->hamming_pairs += c->stats.hamming_pairs;
    out->hamming_alg_bytes += c->stats.hamming_alg_bytes;
    unsigned long long k1s[kSelPairsSlot + 1], k1c[2] = {0, 0};
    SFM_RC(c->d_k1_counters.read(k1s, kSelPairsSlot + 1, cs));
    for (int q = 0; q < kK1CounterSlots; ++q) {
      k1c[0] += k1s[2 * q];
      k1c[1] += k1s[2 * q + 1];
    }
    out->hamming_lane_ops += c->stats.hamming_lane_ops + 64ull * k1c[0] * (uint64_t)c->k1_finish_ops;
    out->hamming_pairs_finished += 64ull * k1c[0];
    out->hamming_rows_flagged += k1c[1];
    out->hamming_pairs += k1s[kSelPairsSlot];
  }
  return SFMLOC_OK;
}

int sfmloc_set_profile(sfmloc_map *map, int level) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_set_profile: null map");
  SFM_CHECK(level >= 0 && level <= 2, SFMLOC_EINVAL, "sfmloc_set_profile: level %d (0 off, 1 every stage, 2 K1 only)", level);
  reinterpret_cast<Map *>(map)->params.profile = level;
  return SFMLOC_OK;
}

int sfmloc_stats_reset(sfmloc_map *map) {
  SFM_CHECK(map, SFMLOC_EINVAL, "sfmloc_stats_reset: null map");
  Map *m = reinterpret_cast<Map *>(map);
  SFM_HIP(hipSetDevice(m->device));
  std::vector<Ctx *> all = m->pool;
  all.push_back(m->ctx0);
  for (Ctx *c : all) {
    const hipStream_t cs = c->stream;
    SFM_HIP(hipStreamSynchronize(cs));
    int rc = drain_events(c);
    if (rc) return rc;
    memset(&c->stats, 0, sizeof(c->stats));
    SFM_RC(c->d_k1_counters.zero(cs));  // (on the context's stream: a scan queued next is ordered behind the clear)
  }
  return SFMLOC_OK;
}

}  // extern "C"
