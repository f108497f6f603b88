// sfmloc_sfm_color_plan: the greedy view cover of OpenMVG's ColorizeTracks (openMVG_main_ComputeSfM_DataColor) on a
// device-resident sfm_data.  The semantics are stated in include/sfmloc.h ("colouring plan").
//
// The reference recounts every view over the remaining landmarks in each iteration.  Here the counts are decremental:
// card[v] starts as the length of view v's list (adjust.hip's transpose) and colouring a landmark subtracts one from
// the count of every view that sees it, so an observation is read once when its landmark is coloured and once more
// for every time its view is chosen before that.  An iteration is two launches on the handle's stream:
//
//   k_color_argmax   one workgroup: the view of the largest card, lowest index among equals, as one integer maximum of
//                    (card << 32 | 0xFFFFFFFF - view).  It is the only writer of the plan's state (iteration number,
//                    chosen view, order[]), which stays in device memory.
//   k_color_update   grid-stride over the chosen view's list: an uncoloured landmark records (iteration, observation)
//                    and walks its CSR row with atomicSub on card[] (uint32: the same result in any order).  The
//                    remaining-landmark count goes down by one atomicSub per workgroup.
//
// Stream order alone carries the dependency between the two and between iterations; no workgroup waits for another.
// The host enqueues SFMLOC_COLOR_CHUNK iterations, then reads the remaining count; once it is 0 the kernels still in
// the queue return at once.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfm_data.h"

namespace sfmloc {
namespace {

constexpr uint32_t kUncoloured = 0xFFFFFFFFu;
constexpr int kArgmaxThreads = 1024;
constexpr int kUpdateThreads = 256;
constexpr uint32_t kUpdateMaxBlocks = 256;

thread_local double g_color_last_ms = 0.0;

struct ColorState {
  uint32_t remaining;  // uncoloured landmarks that have an observation (k_color_update subtracts)
  uint32_t n_order;    // iterations chosen so far
  uint32_t view;       // the chosen view of the iteration in flight
  uint32_t active;     // 1 = k_color_argmax chose a view: k_color_update has work
};

// card[v] = length of view v's list; lm_iter = uncoloured; remaining = landmarks with a non-empty CSR row
__global__ __launch_bounds__(256) void k_color_init(uint32_t n_views, const uint32_t *__restrict__ view_off,
                                                    uint32_t *__restrict__ card, uint32_t n_lm,
                                                    const uint64_t *__restrict__ obs_off, uint32_t *__restrict__ lm_iter,
                                                    unsigned long long *__restrict__ lm_obs, ColorState *st) {
  __shared__ uint32_t cnt;
  if (threadIdx.x == 0) cnt = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_views) card[i] = view_off[i + 1] - view_off[i];
  bool has = false;
  if (i < n_lm) {
    lm_iter[i] = kUncoloured;
    lm_obs[i] = 0;
    has = obs_off[i + 1] > obs_off[i];
  }
  const unsigned long long b = __ballot(has);
  if ((threadIdx.x & 63) == 0 && b) atomicAdd(&cnt, (uint32_t)__popcll(b));
  __syncthreads();
  if (threadIdx.x == 0 && cnt) atomicAdd(&st->remaining, cnt);
}

__global__ __launch_bounds__(kArgmaxThreads) void k_color_argmax(uint32_t n_views, const uint32_t *__restrict__ card,
                                                                 ColorState *st, uint32_t *__restrict__ order) {
  __shared__ unsigned long long wbest[kArgmaxThreads / 64];
  const uint32_t remaining = st->remaining;
  if (remaining == 0) {  // (uniform: every thread read the same word, nobody has written it in this launch)
    if (threadIdx.x == 0) st->active = 0;
    return;
  }
  unsigned long long best = 0;
  for (uint32_t v = threadIdx.x; v < n_views; v += kArgmaxThreads) {
    const unsigned long long key = ((unsigned long long)card[v] << 32) | (unsigned long long)(0xFFFFFFFFu - v);
    best = key > best ? key : best;
  }
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(best, off, 64);
    best = o > best ? o : best;
  }
  if ((threadIdx.x & 63) == 0) wbest[threadIdx.x >> 6] = best;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < kArgmaxThreads / 64; ++w) best = wbest[w] > best ? wbest[w] : best;
    const uint32_t c = (uint32_t)(best >> 32), v = 0xFFFFFFFFu - (uint32_t)best;
    if (c == 0 || st->n_order >= n_views) {  // (cannot happen while landmarks remain; ends the loop if it did)
      st->remaining = 0;
      st->active = 0;
    } else {
      order[st->n_order] = v;
      st->n_order += 1;
      st->view = v;
      st->active = 1;
    }
  }
}

__global__ __launch_bounds__(kUpdateThreads) void k_color_update(
    const uint32_t *__restrict__ view_off, const uint32_t *__restrict__ vlist, const uint32_t *__restrict__ obs_lm,
    const uint64_t *__restrict__ obs_off, const uint32_t *__restrict__ obs_view, uint32_t *card, uint32_t *lm_iter,
    unsigned long long *lm_obs, ColorState *st) {
  __shared__ uint32_t coloured;
  if (!st->active) return;  // (written by k_color_argmax only: the same for every workgroup of this launch)
  if (threadIdx.x == 0) coloured = 0;
  __syncthreads();
  const uint32_t v = st->view, k = st->n_order - 1;
  const uint32_t b = view_off[v], e = view_off[v + 1];
  uint32_t mine = 0;
  for (uint32_t p = b + blockIdx.x * kUpdateThreads + threadIdx.x; p < e; p += gridDim.x * kUpdateThreads) {
    const uint32_t o = vlist[p], l = obs_lm[o];
    // a landmark that names the view twice sits in adjacent places of the list (its row is contiguous and the sort
    // is stable): its first place alone acts, so no two lanes claim one landmark
    if (p > b && obs_lm[vlist[p - 1]] == l) continue;
    if (lm_iter[l] != kUncoloured) continue;
    lm_iter[l] = k;
    lm_obs[l] = o;
    ++mine;
    for (uint64_t j = obs_off[l]; j < obs_off[l + 1]; ++j) atomicSub(&card[obs_view[j]], 1u);
  }
  if (mine) atomicAdd(&coloured, mine);
  __syncthreads();
  if (threadIdx.x == 0 && coloured) atomicSub(&st->remaining, coloured);
}

int color_plan_impl(const Sfm &h, uint32_t *order, uint32_t *n_order, uint32_t *lm_iter, uint64_t *lm_obs) {
  CallScope d;  // (on the handle's stream; before the buffers: destroyed after them)
  const SfmDev V = sfm_dev(h);
  uint32_t max_view_obs = 0;  // the longest per-view list
  for (uint32_t v = 0; v < h.n_views; ++v) max_view_obs = std::max(max_view_obs, h.h_view_off[v + 1] - h.h_view_off[v]);
  DevBuf<uint32_t> d_card, d_order, d_iter;
  DevBuf<unsigned long long> d_obs;
  DevBuf<ColorState> d_st;
  int rc;
  if ((rc = d_card.alloc(nullptr, V.n_views)) || (rc = d_order.alloc(nullptr, V.n_views)) ||
      (rc = d_iter.alloc(nullptr, V.n_lm ? V.n_lm : 1)) || (rc = d_obs.alloc(nullptr, V.n_lm ? V.n_lm : 1)) ||
      (rc = d_st.alloc(nullptr, 1)))
    return rc;
  if ((rc = d.open(true, &g_color_last_ms, h.s))) return rc;
  SFM_RC(d_st.zero(d.s));
  SFM_RC(d_order.zero(V.n_views, d.s));
  if ((rc = d.time_begin())) return rc;
  const uint32_t n_init = V.n_views > V.n_lm ? V.n_views : V.n_lm;
  SFM_RC(dev_launch(k_color_init, dim3((n_init + 255) / 256), dim3(256), 0, d.s, V.n_views, V.view_off, d_card, V.n_lm,
                    V.obs_off, d_iter, d_obs, d_st));
  uint32_t blocks = (max_view_obs + kUpdateThreads - 1) / kUpdateThreads;
  blocks = blocks < 1 ? 1 : (blocks > kUpdateMaxBlocks ? kUpdateMaxBlocks : blocks);
  ColorState st;
  for (;;) {
    SFM_RC(d_st.download(&st, 1, d.s));
    SFM_HIP(hipStreamSynchronize(d.s));
    if (st.remaining == 0) break;
    for (uint32_t i = 0; i < SFMLOC_COLOR_CHUNK; ++i) {
      SFM_RC(dev_launch(k_color_argmax, dim3(1), dim3(kArgmaxThreads), 0, d.s, V.n_views, d_card, d_st, d_order));
      SFM_RC(dev_launch(k_color_update, dim3(blocks), dim3(kUpdateThreads), 0, d.s, V.view_off, V.vlist, V.obs_lm,
                        V.obs_off, V.obs_view, d_card, d_iter, d_obs, d_st));
    }
  }
  if ((rc = d.time_end())) return rc;
  SFM_RC(d_order.download(order, st.n_order, d.s));
  if (V.n_lm) {
    SFM_RC(d_iter.download(lm_iter, V.n_lm, d.s));
    SFM_RC(d_obs.download(lm_obs, V.n_lm, d.s));
  }
  SFM_HIP(hipStreamSynchronize(d.s));
  *n_order = st.n_order;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

double sfmloc_sfm_color_last_ms(void) { return g_color_last_ms; }

int sfmloc_sfm_color_plan(sfmloc_sfm *hh, uint32_t *order, uint32_t *n_order, uint32_t *lm_iter, uint64_t *lm_obs) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_color_plan: null handle");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  SFM_CHECK(order && n_order && (h->n_lm == 0 || (lm_iter && lm_obs)), SFMLOC_EINVAL,
            "sfmloc_sfm_color_plan: null argument");
  g_color_last_ms = 0.0;
  SFM_HIP(hipSetDevice(h->device));
  return color_plan_impl(*h, order, n_order, lm_iter, lm_obs);
}

}  // extern "C"
