// sfmloc_sfm_register: the growth step of incremental SfM on a resident sfm_data whose keep masks exist -- views
// without a pose are resected with K5 on their correspondences to the kept landmarks, the kept landmarks gain the
// observations of the new views that fit, and the landmarks the new views make triangulable are triangulated; round
// after round until a round registers nothing.  The semantics are stated in include/sfmloc.h ("sfmloc_sfm_register");
// tests/register_np.py restates every operation.  f64, unfused (the library's -ffp-contract=off), no float atomics.
//
//   lists       k_reg_compact: one workgroup per unposed view, all of them in one launch.  The view's slice of the
//               transpose (adjust.hip's vlist: ascending landmark id) is compacted to the observations of kept landmarks
//               in tiles of 256: a wave64 ballot gives the rank inside the wave, the four waves' counts meet in LDS, the
//               running count carries over the tiles.  No atomic decides a position (radix_sort.h's scatter is the
//               model).  The compacted list of view v starts where its slice starts, view_off[v]; cnt[v] is its length.
//   resection   sfm_data.h's sfm_resect_gang on the compacted lists with their counts, the pixel undistorted: the driver
//               adjust.hip's re-resection runs on.  What is this file's: which views are tried, the acceptance rule
//               and the round bookkeeping.
//   extend      k_reg_extend: one thread per entry of a new view's compacted list; "inliers" of sfmloc.h on the
//               projection triangulate.hip's tri_inlier and adjust.hip's k_adj_residual use (geom::project_pixel).
//   select      k_reg_select: the landmarks the selective triangulation (triangulate.hip, TriArgs::select) runs on.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "sfm_data.h"

namespace sfmloc {
namespace {

constexpr int kRegBlock = 256;              // a tile of the compaction: four waves

// sfmloc.h "list": cnt[v] and the kept-landmark observations of every unposed view, order preserved
__global__ __launch_bounds__(kRegBlock) void k_reg_compact(const uint32_t *__restrict__ unposed,
                                                           const uint32_t *__restrict__ vlist,
                                                           const uint32_t *__restrict__ view_off,
                                                           const uint32_t *__restrict__ obs_lm,
                                                           const uint8_t *__restrict__ lm_stage,
                                                           uint32_t *__restrict__ clist, uint32_t *__restrict__ cnt) {
  constexpr int kWaves = kRegBlock / 64;
  __shared__ uint32_t wsum[kWaves];
  const uint32_t v = unposed[blockIdx.x];
  const uint32_t b = view_off[v], n = view_off[v + 1] - b;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  uint32_t run = 0;  // kept entries of the earlier tiles (the same in every thread)
  for (uint32_t base = 0; base < n; base += kRegBlock) {
    const uint32_t i = base + threadIdx.x;
    uint32_t o = 0;
    bool keep = false;
    if (i < n) {
      o = vlist[b + i];
      keep = lm_stage[obs_lm[o]] == 3;
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) wsum[w] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0, total = 0;
#pragma unroll
    for (int ww = 0; ww < kWaves; ++ww) {
      const uint32_t x = wsum[ww];
      before += ww < w ? x : 0u;
      total += x;
    }
    if (keep) clist[b + run + before + (uint32_t)__popcll(m & below)] = o;  // (at most the slice's n entries)
    run += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) cnt[v] = run;
}

// sfmloc.h "count" alone, for every view: one workgroup per view over its slice of the transpose; nothing is written
// but c[v] (sfmloc_sfm_register_counts)
__global__ __launch_bounds__(kRegBlock) void k_reg_counts(uint32_t n_views, const uint32_t *__restrict__ vlist,
                                                          const uint32_t *__restrict__ view_off,
                                                          const uint32_t *__restrict__ obs_lm,
                                                          const uint8_t *__restrict__ lm_stage, uint32_t *__restrict__ c) {
  __shared__ uint32_t s_cnt;
  const uint32_t v = blockIdx.x;
  if (v >= n_views) return;
  const uint32_t b = view_off[v], n = view_off[v + 1] - b;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  uint32_t mine = 0;
  for (uint32_t i = threadIdx.x; i < n; i += kRegBlock) mine += lm_stage[obs_lm[vlist[b + i]]] == 3 ? 1u : 0u;
  if (mine) atomicAdd(&s_cnt, mine);  // (an integer count: order-free)
  __syncthreads();
  if (threadIdx.x == 0) c[v] = s_cnt;
}

// the resident arrays (SfmDev; obs_keep is written) and the round's lists
struct RegExtendArgs : SfmDev {
  const uint32_t *unposed, *clist, *cnt;
  const uint8_t *view_new;
  double thr;
  unsigned long long *extended;
};

// sfmloc.h "extend": blockIdx.y = a view that was unposed when the round began (nothing to do unless it registered),
// one thread per entry of its compacted list; X does not move
__global__ __launch_bounds__(kRegBlock) void k_reg_extend(RegExtendArgs A) {
  __shared__ unsigned int s_cnt;
  const uint32_t v = A.unposed[blockIdx.y];
  if (!A.view_new[v]) return;  // (the same for the whole workgroup)
  const uint32_t n = A.cnt[v];
  if (blockIdx.x * (uint32_t)kRegBlock >= n) return;
  if (threadIdx.x == 0) s_cnt = 0;
  __syncthreads();
  const uint32_t k = blockIdx.x * (uint32_t)kRegBlock + threadIdx.x;
  bool in = false;
  if (k < n) {
    const uint32_t o = A.clist[A.view_off[v] + k], l = A.obs_lm[o];
    const uint32_t ii = A.view_intr[v], pi = A.view_pose[v];
    const double *R = A.pose_R + 9 * (size_t)pi, *C = A.pose_C + 3 * (size_t)pi, *K = A.intr + 6 * (size_t)ii;
    const double *X = A.lm_X + 3 * (size_t)l;
    double X2, px, py;
    geom::project_pixel(R, C, K, A.intr_type[ii] == 3, X, &X2, &px, &py);
    const double ex = A.obs_x[2 * (size_t)o] - px, ey = A.obs_x[2 * (size_t)o + 1] - py;
    in = !A.obs_keep[o] && X2 > 0.0 && sqrt(ex * ex + ey * ey) <= A.thr;  // (a NaN residual is not <= thr)
    if (in) A.obs_keep[o] = 1;
  }
  const unsigned long long m = __ballot(in);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&s_cnt, (unsigned int)__popcll(m));  // (integer counts: order-free)
  __syncthreads();
  if (threadIdx.x == 0 && s_cnt) atomicAdd(A.extended, (unsigned long long)s_cnt);
}

// sfmloc.h "new landmarks": not kept, an observation in a view registered this round, at least 2 posed observations
__global__ __launch_bounds__(256) void k_reg_select(uint32_t n_lm, const uint64_t *__restrict__ obs_off,
                                                    const uint32_t *__restrict__ obs_view,
                                                    const uint32_t *__restrict__ view_pose,
                                                    const uint8_t *__restrict__ pose_valid,
                                                    const uint8_t *__restrict__ view_new,
                                                    const uint8_t *__restrict__ lm_stage, uint8_t *__restrict__ select) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lm) return;
  uint32_t posed = 0, touched = 0;
  if (lm_stage[l] != 3)
    for (uint64_t o = obs_off[l]; o < obs_off[l + 1]; ++o) {
      const uint32_t v = obs_view[o];
      posed += pose_valid[view_pose[v]] ? 1u : 0u;
      touched |= view_new[v];
    }
  select[l] = (touched && posed >= 2) ? 1 : 0;
}

int reg_run(Sfm &h, const sfmloc_register_options &opt, sfmloc_register_report *rep) {
  SfmRegState &S = h.reg;
  const uint32_t n_views = h.n_views, n_lm = h.n_lm;
  hipStream_t s = h.s;
  const size_t obs1 = h.n_obs ? h.n_obs : 1, lm1 = n_lm ? n_lm : 1;
  int rc;
  if (S.res.size() != n_views) {  // the first call on this handle
    if ((rc = S.d_clist.alloc(nullptr, obs1)) || (rc = S.d_cnt.alloc(nullptr, n_views)) ||
        (rc = S.d_unposed.alloc(nullptr, n_views)) || (rc = S.d_view_new.alloc(nullptr, n_views)) ||
        (rc = S.d_select.alloc(nullptr, lm1)) || (rc = S.d_extended.alloc(nullptr, 1)))
      return rc;
    S.round.assign(n_views, -1);
    S.last_cnt.assign(n_views, 0);
    S.inliers.assign(n_views, std::vector<uint32_t>());
    S.res.assign(n_views, sfmloc_sfm_view_result{});  // (last: a failed allocation leaves the state unmade)
  }
  Event e0, e1;
  SFM_RC(e0.create(kTimingEvent));
  SFM_RC(e1.create(kTimingEvent));
  SFM_HIP(hipEventRecord(e0, s));
  SFM_RC(S.d_extended.zero(1, s));
  sfmloc_register_report R;
  memset(&R, 0, sizeof R);
  for (uint32_t v = 0; v < n_views; ++v) R.views_unposed_in += h.h_pose_valid[h.h_view_pose[v]] ? 0u : 1u;
  std::vector<uint32_t> unposed, cnt(n_views), todo, todo_n;
  std::vector<uint8_t> is_new(n_views);
  unsigned long long ext_before = 0;
  // (rounds are numbered over the handle's life: a second call goes on where the first stopped)
  for (uint32_t i = 0; opt.max_rounds == 0 || i < opt.max_rounds; ++i) {
    const uint32_t round = S.rounds_done;
    // count + list: the views without a pose as the round begins, one launch
    unposed.clear();
    for (uint32_t v = 0; v < n_views; ++v)
      if (!h.h_pose_valid[h.h_view_pose[v]]) unposed.push_back(v);
    if (unposed.empty()) break;
    SFM_RC(S.d_unposed.upload(unposed.data(), unposed.size(), s));
    const SfmDev D = sfm_dev(h);
    SFM_RC(dev_launch(k_reg_compact, dim3((unsigned)unposed.size()), dim3(kRegBlock), 0, s, S.d_unposed, D.vlist,
                      D.view_off, D.obs_lm, D.lm_stage, S.d_clist, S.d_cnt));
    SFM_RC(S.d_cnt.download(cnt.data(), n_views, s));
    SFM_HIP(hipStreamSynchronize(s));
    // candidates
    todo.clear();
    todo_n.clear();
    uint32_t longest = 0;
    for (uint32_t v : unposed) {
      const uint32_t c = cnt[v];
      longest = std::max(longest, c);
      if (c > opt.min_points && (S.round[v] < 0 || c > S.last_cnt[v])) {
        SFM_CHECK(c <= kSfmMaxViewObs, SFMLOC_ECAP, "view %u has %u correspondences (at most %u per view)",
                  h.h_view_id[v], c, kSfmMaxViewObs);
        todo.push_back(v);
        todo_n.push_back(c);
      }
    }
    if (todo.empty()) break;
    for (uint32_t v : todo) S.last_cnt[v] = cnt[v];
    // resection + accept: an accepted pose goes into the host's pose table (the last view in ascending id wins a shared
    // id_pose) and is_new[view] = 1
    std::fill(is_new.begin(), is_new.end(), (uint8_t)0);
    uint32_t n_ok = 0;
    rc = sfm_resect_gang<true>(h, todo, todo_n, S.d_clist, S.d_cnt,
                               [&](uint32_t k, const Pose &p) -> std::vector<uint32_t> & {
      // sfmloc.h "resection"
      const bool ok = p.ok && (opt.min_inliers == 0 || p.n_inliers >= (int32_t)opt.min_inliers);
      sfmloc_sfm_view_result &r = S.res[k];
      memset(&r, 0, sizeof r);
      r.ran = 1;
      r.ok = ok ? 1 : 0;
      r.n_obs = (int32_t)cnt[k];
      r.n_inliers = p.n_inliers;
      r.iterations = p.iterations;
      r.error_max = p.error_max;
      r.nfa = p.nfa;
      memcpy(r.P, p.P, sizeof r.P);
      S.round[k] = (int32_t)round;
      if (ok) {
        memcpy(r.R, p.R, sizeof r.R);
        memcpy(r.center, p.center, sizeof r.center);
        const uint32_t pi = h.h_view_pose[k];
        h.h_pose_valid[pi] = 1;
        memcpy(&h.h_pose_R[9 * (size_t)pi], p.R, 9 * sizeof(double));
        memcpy(&h.h_pose_C[3 * (size_t)pi], p.center, 3 * sizeof(double));
        is_new[k] = 1;
        ++n_ok;
      }
      return S.inliers[k];
    });
    if (rc) return rc;
    ++R.rounds;
    ++S.rounds_done;
    R.views_tried += (uint32_t)todo.size();
    R.views_registered += n_ok;
    if (n_ok == 0) break;
    SFM_RC(dev_upload(D.pose_valid, h.h_pose_valid.data(), h.n_poses, s));
    SFM_RC(dev_upload(D.pose_R, h.h_pose_R.data(), 9 * (size_t)h.n_poses, s));
    SFM_RC(dev_upload(D.pose_C, h.h_pose_C.data(), 3 * (size_t)h.n_poses, s));
    SFM_RC(S.d_view_new.upload(is_new.data(), n_views, s));
    // extend
    RegExtendArgs E;
    static_cast<SfmDev &>(E) = D;
    E.unposed = S.d_unposed;
    E.clist = S.d_clist;
    E.cnt = S.d_cnt;
    E.view_new = S.d_view_new;
    E.thr = opt.residual_px;
    E.extended = S.d_extended;
    if (longest)
      SFM_RC(dev_launch(k_reg_extend, dim3((longest + kRegBlock - 1) / kRegBlock, (unsigned)unposed.size()),
                        dim3(kRegBlock), 0, s, E));
    // new landmarks
    if (n_lm)
      SFM_RC(dev_launch(k_reg_select, dim3((n_lm + 255) / 256), dim3(256), 0, s, n_lm, D.obs_off, D.obs_view,
                        D.view_pose, D.pose_valid, S.d_view_new, D.lm_stage, S.d_select));
    SFM_RC(S.d_extended.download(&S.h_extended, 1, s));
    sfmloc_triangulate_options to;
    memset(&to, 0, sizeof to);
    to.mode = SFMLOC_TRI_ROBUST;
    to.min_inliers = opt.tri_min_inliers;
    to.allow_pairs = opt.tri_allow_pairs;
    to.residual_px = opt.residual_px;
    sfmloc_triangulate_report tr;
    rc = triangulate_run(h, to, &tr, S.d_select);  // (ends with the stream drained: `ext` has arrived)
    if (rc) return rc;
    R.obs_extended += S.h_extended - ext_before;
    ext_before = S.h_extended;
    R.landmarks_tried += tr.landmarks_kept + tr.failed_posed + tr.failed_hypothesis + tr.failed_inliers;
    R.landmarks_added += tr.landmarks_kept;
  }
  SFM_HIP(hipEventRecord(e1, s));
  SFM_HIP(hipEventSynchronize(e1));
  float ms = 0.f;
  SFM_HIP(hipEventElapsedTime(&ms, e0, e1));
  R.device_ms = ms;
  if (rep) *rep = R;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_register_default_options(sfmloc_register_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->max_rounds = 16;
  o->min_points = 10;  // MINIMUM_VIEW_NUM_TO_ESTIMATAE_CAMERA_POSE, test ">"
  o->min_inliers = 0;
  o->tri_min_inliers = 3;
  o->tri_allow_pairs = 1;
  o->residual_px = 4.0;
}

int sfmloc_sfm_register(sfmloc_sfm *hh, const sfmloc_register_options *opt, sfmloc_register_report *rep) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_register: null handle");
  sfmloc_register_options o;
  if (opt) o = *opt;
  else sfmloc_register_default_options(&o);
  SFM_CHECK(o.tri_min_inliers >= 2 && o.residual_px >= 0.0, SFMLOC_EINVAL,
            "sfmloc_sfm_register: tri_min_inliers must be at least 2 and residual_px not negative");
  if (rep) memset(rep, 0, sizeof *rep);
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_CHECK(h->cleaned, SFMLOC_EINVAL,
            "sfmloc_sfm_register: the keep masks do not exist yet (after sfmloc_sfm_triangulate or sfmloc_sfm_clean)");
  SFM_HIP(hipSetDevice(h->device));
  try {
    return reg_run(*h, o, rep);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_register: out of host memory");
    return SFMLOC_ENOMEM;
  }
}

int sfmloc_sfm_register_read(const sfmloc_sfm *hh, sfmloc_sfm_view_result *out, int32_t *round) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_register_read: null handle");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  const SfmRegState &S = h->reg;
  for (uint32_t k = 0; k < h->n_views; ++k) {
    const bool have = k < S.res.size();
    if (out) {
      if (have) out[k] = S.res[k];
      else memset(&out[k], 0, sizeof out[k]);
    }
    if (round) round[k] = have ? S.round[k] : -1;
  }
  return SFMLOC_OK;
}

int sfmloc_sfm_register_counts(const sfmloc_sfm *hh, uint32_t *c) {
  SFM_CHECK(hh && c, SFMLOC_EINVAL, "sfmloc_sfm_register_counts: null argument");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  SFM_CHECK(h->cleaned, SFMLOC_EINVAL,
            "sfmloc_sfm_register_counts: the keep masks do not exist yet (after sfmloc_sfm_triangulate or sfmloc_sfm_clean)");
  if (h->n_views == 0) return SFMLOC_OK;
  SFM_HIP(hipSetDevice(h->device));
  DevBuf<uint32_t> d_c;  // (the call's own: the handle keeps nothing of it)
  SFM_RC(d_c.alloc(nullptr, h->n_views));
  const SfmDev D = sfm_dev(*h);
  hipStream_t s = h->s;
  SFM_RC(dev_launch(k_reg_counts, dim3(h->n_views), dim3(kRegBlock), 0, s, h->n_views, D.vlist, D.view_off, D.obs_lm,
                    D.lm_stage, d_c));
  SFM_RC(d_c.download(c, h->n_views, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

int sfmloc_sfm_register_inliers(const sfmloc_sfm *hh, uint32_t k, uint32_t *idx, uint32_t cap, uint32_t *n) {
  SFM_CHECK(hh && n, SFMLOC_EINVAL, "sfmloc_sfm_register_inliers: null argument");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  SFM_CHECK(k < h->n_views, SFMLOC_EINVAL, "sfmloc_sfm_register_inliers: view index %u out of range", k);
  static const std::vector<uint32_t> none;
  const std::vector<uint32_t> &v = k < h->reg.inliers.size() ? h->reg.inliers[k] : none;
  *n = (uint32_t)v.size();
  SFM_CHECK(!idx || cap >= v.size(), SFMLOC_ECAP, "sfmloc_sfm_register_inliers: %u entries, %zu inliers", cap, v.size());
  if (idx && !v.empty()) memcpy(idx, v.data(), v.size() * sizeof(uint32_t));
  return SFMLOC_OK;
}

}  // extern "C"
