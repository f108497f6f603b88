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
//   fill        RegFillBody: the compacted list into a K5 context's 2D-3D buffers, the pixel undistorted.  K5 itself
//               runs unchanged, as adjust.hip's re-resection runs it: 32 views per gang session, stream = id_view.
//   extend      k_reg_extend: one thread per entry of a new view's compacted list; "inliers" of sfmloc.h in the
//               arithmetic of triangulate.hip's tri_inlier / adjust.hip's k_adj_residual.
//   select      k_reg_select: the landmarks the selective triangulation (triangulate.hip, TriArgs::select) runs on.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "geom_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint32_t kRegGang = 32;           // contexts per gang session (kGangMembers)
constexpr uint32_t kRegMaxViewObs = 65536;  // a view's list must fit a context's 2D-3D buffers (make_ctx: 65 536)
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

// sfmloc.h "list": a view's compacted list into a context's 2D-3D buffers, the pixel undistorted for
// pinhole_radial_k3 (ii = the view's intrinsic); the inlier pairs then name positions in the list
struct RegFillBody {
  static constexpr int kGangThreads = kRegBlock;
  static __device__ __forceinline__ void run(const uint32_t *clist, const uint32_t *view_off, const uint32_t *cnt,
                                             uint32_t v, uint32_t ii, const uint32_t *obs_lm, const double *obs_x,
                                             const double *lm_X, const uint32_t *lm_id, const uint32_t *intr_type,
                                             const double *intr, uint32_t *ms_n, uint32_t *ms_qfeat,
                                             uint32_t *ms_landmark, double *pt2d, double *pt3d) {
    const uint32_t b = view_off[v], n = cnt[v];
    const double *K = intr + 6 * (size_t)ii;
    const bool radial = intr_type[ii] == 3;
    for (uint32_t k = threadIdx.x; k < n; k += kRegBlock) {
      const uint32_t o = clist[b + k], l = obs_lm[o];
      const double x = obs_x[2 * (size_t)o], y = obs_x[2 * (size_t)o + 1];
      double ux = x, uy = y;
      if (radial) geom::ud_pixel_k3(K[0], K[1], K[2], K[3], K[4], K[5], x, y, &ux, &uy);
      pt2d[2 * k] = ux;
      pt2d[2 * k + 1] = uy;
      pt3d[3 * k] = lm_X[3 * (size_t)l];
      pt3d[3 * k + 1] = lm_X[3 * (size_t)l + 1];
      pt3d[3 * k + 2] = lm_X[3 * (size_t)l + 2];
      ms_qfeat[k] = k;
      ms_landmark[k] = lm_id[l];
    }
    if (threadIdx.x == 0) *ms_n = n;
  }
};
__global__ __launch_bounds__(kRegBlock) void k_reg_fill(const uint32_t *clist, const uint32_t *view_off,
                                                        const uint32_t *cnt, uint32_t v, uint32_t ii,
                                                        const uint32_t *obs_lm, const double *obs_x, const double *lm_X,
                                                        const uint32_t *lm_id, const uint32_t *intr_type,
                                                        const double *intr, uint32_t *ms_n, uint32_t *ms_qfeat,
                                                        uint32_t *ms_landmark, double *pt2d, double *pt3d) {
  RegFillBody::run(clist, view_off, cnt, v, ii, obs_lm, obs_x, lm_X, lm_id, intr_type, intr, ms_n, ms_qfeat, ms_landmark,
                   pt2d, pt3d);
}

struct RegExtendArgs {
  const uint32_t *unposed, *clist, *view_off, *cnt, *obs_lm, *view_intr, *view_pose, *intr_type;
  const uint8_t *view_new;
  const double *intr, *pose_R, *pose_C, *obs_x, *lm_X;
  double thr;
  uint8_t *obs_keep;
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
    const double f = K[0], ppx = K[1], ppy = K[2];
    const double d0 = X[0] - C[0], d1 = X[1] - C[1], d2 = X[2] - C[2];
    const double X0 = (R[0] * d0 + R[1] * d1) + R[2] * d2;
    const double X1 = (R[3] * d0 + R[4] * d1) + R[5] * d2;
    const double X2 = (R[6] * d0 + R[7] * d1) + R[8] * d2;
    double p0 = X0 / X2, p1 = X1 / X2;
    if (A.intr_type[ii] == 3) {
      const double r2 = p0 * p0 + p1 * p1;
      const double r4 = r2 * r2, r6 = r4 * r2;
      const double rc = ((1.0 + K[3] * r2) + K[4] * r4) + K[5] * r6;
      p0 = p0 * rc;
      p1 = p1 * rc;
    }
    const double ex = A.obs_x[2 * (size_t)o] - (f * p0 + ppx), ey = A.obs_x[2 * (size_t)o + 1] - (f * p1 + ppy);
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

struct Round {
  uint32_t tried = 0, registered = 0;
  uint64_t extended = 0, lm_tried = 0, lm_added = 0;
};

// K5 on the candidates `todo` (view indices), 32 per gang session, as adjust.hip's sfm_resect_impl runs it; an accepted
// pose goes into the host's pose table (the last view in ascending id wins a shared id_pose) and is_new[view] = 1
int reg_resect(const SfmRegView &V, const std::vector<uint32_t> &todo, const std::vector<uint32_t> &cnt, int32_t round,
               uint32_t min_inliers, std::vector<uint8_t> &is_new, uint32_t *n_ok) {
  SfmRegState &S = *V.state;
  sfmloc_context **ctx = nullptr;
  int rc = sfm_reg_contexts(V.handle, std::min<uint32_t>(kRegGang, (uint32_t)todo.size()), &ctx);
  if (rc) return rc;
  for (size_t g0 = 0; g0 < todo.size(); g0 += kRegGang) {
    const uint32_t m = (uint32_t)std::min<size_t>(kRegGang, todo.size() - g0);
    for (uint32_t i = 0; i < m; ++i) {  // (a regrowth synchronises: before the session records anything)
      Ctx *c = reinterpret_cast<Ctx *>(ctx[i]);
      const uint32_t k = todo[g0 + i];
      rc = ctx_p3p_reserve(c, cnt[k]);
      if (rc) return rc;
      const double *K = V.h_intr + 6 * (size_t)V.h_view_intr[k];
      c->p3p_stream = V.h_view_id[k];  // the view's own sampling stream: independent of the batch and of the round
      c->p3p_own_K = true;
      c->p3p_K[0] = K[0];
      c->p3p_K[1] = K[1];
      c->p3p_K[2] = K[2];
    }
    rc = sfmloc_gang_begin(ctx, m);
    if (rc) return rc;
    for (uint32_t i = 0; i < m && rc == SFMLOC_OK; ++i) {
      Ctx *c = reinterpret_cast<Ctx *>(ctx[i]);
      const uint32_t k = todo[g0 + i];
      sfm_launch<RegFillBody>(c, k_reg_fill, dim3(1), dim3(kRegBlock), 0, (const uint32_t *)S.d_clist, V.d_view_off,
                              (const uint32_t *)S.d_cnt, k, V.h_view_intr[k], V.d_obs_lm, V.tri.d_obs_x,
                              (const double *)V.tri.d_lm_X, V.tri.d_lm_id, V.tri.d_intr_type, V.tri.d_intr, c->d_ms_n,
                              c->d_ms_qfeat, c->d_ms_landmark, c->d_pt2d, c->d_pt3d);
      c->p3p_init_fused = false;  // K5's init reads the count k_reg_fill wrote
      rc = ctx_resection_begin(c);
    }
    const int rc_end = sfmloc_gang_end(ctx, m);
    if (rc) return rc;
    if (rc_end) return rc_end;
    std::vector<uint32_t> failed;  // members whose view failed with a non-empty inlier set
    for (uint32_t i = 0; i < m; ++i) {
      Ctx *c = reinterpret_cast<Ctx *>(ctx[i]);
      const uint32_t k = todo[g0 + i];
      rc = ctx_resection_wait_done(c);
      if (rc) return rc;
      const HostResult *hr = reinterpret_cast<const HostResult *>(c->h_result);
      const Pose &p = hr->pose;
      SFM_CHECK((p.status & 4) == 0, SFMLOC_ECAP, "view %u: more correspondences than the P3P workspace holds",
                V.h_view_id[k]);
      const bool ok = p.ok && (min_inliers == 0 || p.n_inliers >= (int32_t)min_inliers);  // sfmloc.h "resection"
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
      if (ok) {
        memcpy(r.R, p.R, sizeof r.R);
        memcpy(r.center, p.center, sizeof r.center);
      }
      S.round[k] = round;
      const uint32_t ni = p.n_inliers > 0 ? (uint32_t)p.n_inliers : 0u;
      std::vector<uint32_t> &inl = S.inliers[k];
      inl.resize(ni);
      if (!p.ok) {  // K5 publishes no pair list for a failed query: its best model's list, read below
        if (ni) failed.push_back(i);
        continue;
      }
      if (c->p3p_cap > (uint32_t)kP3pMaxN)  // (a regrown workspace keeps its pair lists outside the result record)
        SFM_HIP(hipMemcpy(inl.data(), c->d_pair_qfeat, ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
      else
        memcpy(inl.data(), hr->pair_qfeat, ni * sizeof(uint32_t));
      if (!ok) continue;
      const uint32_t pi = V.h_view_pose[k];
      V.h_pose_valid[pi] = 1;
      memcpy(V.h_pose_R + 9 * (size_t)pi, p.R, 9 * sizeof(double));
      memcpy(V.h_pose_C + 3 * (size_t)pi, p.center, 3 * sizeof(double));
      is_new[k] = 1;
      ++*n_ok;
    }
    for (uint32_t i : failed) {
      Ctx *c = reinterpret_cast<Ctx *>(ctx[i]);
      std::vector<uint32_t> &inl = S.inliers[todo[g0 + i]];
      SFM_HIP(hipMemcpyAsync(inl.data(), c->d_best_inl, inl.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, V.tri.s));
    }
    if (!failed.empty()) SFM_HIP(hipStreamSynchronize(V.tri.s));  // (after the contexts' work: the waits above saw it end)
  }
  for (uint32_t i = 0; i < std::min<uint32_t>(kRegGang, (uint32_t)todo.size()); ++i)
    reinterpret_cast<Ctx *>(ctx[i])->p3p_own_K = false;
  return SFMLOC_OK;
}

int reg_run(SfmRegView &V, const sfmloc_register_options &opt, sfmloc_register_report *rep) {
  SfmRegState &S = *V.state;
  const uint32_t n_views = V.tri.n_views, n_lm = V.tri.n_lm;
  hipStream_t s = V.tri.s;
  const size_t obs1 = V.tri.n_obs ? V.tri.n_obs : 1, lm1 = n_lm ? n_lm : 1;
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
  hipEvent_t e0 = nullptr, e1 = nullptr;
  SFM_HIP(hipEventCreate(&e0));
  SFM_HIP(hipEventCreate(&e1));
  struct Events {
    hipEvent_t &a, &b;
    ~Events() {
      hipEventDestroy(a);
      hipEventDestroy(b);
    }
  } events{e0, e1};
  SFM_HIP(hipEventRecord(e0, s));
  SFM_HIP(hipMemsetAsync(S.d_extended, 0, sizeof(unsigned long long), s));
  sfmloc_register_report R;
  memset(&R, 0, sizeof R);
  for (uint32_t v = 0; v < n_views; ++v) R.views_unposed_in += V.h_pose_valid[V.h_view_pose[v]] ? 0u : 1u;
  std::vector<uint32_t> unposed, cnt(n_views), todo;
  std::vector<uint8_t> is_new(n_views);
  unsigned long long ext_before = 0;
  // (rounds are numbered over the handle's life: a second call goes on where the first stopped)
  for (uint32_t i = 0; opt.max_rounds == 0 || i < opt.max_rounds; ++i) {
    const uint32_t round = S.rounds_done;
    // count + list: the views without a pose as the round begins, one launch
    unposed.clear();
    for (uint32_t v = 0; v < n_views; ++v)
      if (!V.h_pose_valid[V.h_view_pose[v]]) unposed.push_back(v);
    if (unposed.empty()) break;
    SFM_HIP(hipMemcpyAsync(S.d_unposed, unposed.data(), unposed.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_reg_compact, dim3((unsigned)unposed.size()), dim3(kRegBlock), 0, s,
                       (const uint32_t *)S.d_unposed, V.d_vlist, V.d_view_off, V.d_obs_lm,
                       (const uint8_t *)V.tri.d_lm_stage, S.d_clist.get(), S.d_cnt.get());
    SFM_HIP(hipGetLastError());
    SFM_HIP(hipMemcpyAsync(cnt.data(), S.d_cnt, n_views * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    SFM_HIP(hipStreamSynchronize(s));
    // candidates
    todo.clear();
    uint32_t longest = 0;
    for (uint32_t v : unposed) {
      const uint32_t c = cnt[v];
      longest = std::max(longest, c);
      if (c > opt.min_points && (S.round[v] < 0 || c > S.last_cnt[v])) {
        SFM_CHECK(c <= kRegMaxViewObs, SFMLOC_ECAP, "view %u has %u correspondences (at most %u per view)",
                  V.h_view_id[v], c, kRegMaxViewObs);
        todo.push_back(v);
      }
    }
    if (todo.empty()) break;
    for (uint32_t v : todo) S.last_cnt[v] = cnt[v];
    // resection + accept
    std::fill(is_new.begin(), is_new.end(), (uint8_t)0);
    uint32_t n_ok = 0;
    rc = reg_resect(V, todo, cnt, (int32_t)round, opt.min_inliers, is_new, &n_ok);
    if (rc) return rc;
    ++R.rounds;
    ++S.rounds_done;
    R.views_tried += (uint32_t)todo.size();
    R.views_registered += n_ok;
    if (n_ok == 0) break;
    SFM_HIP(hipMemcpyAsync(V.d_pose_valid, V.h_pose_valid, V.n_poses, hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemcpyAsync(V.d_pose_R, V.h_pose_R, 9 * (size_t)V.n_poses * sizeof(double), hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemcpyAsync(V.d_pose_C, V.h_pose_C, 3 * (size_t)V.n_poses * sizeof(double), hipMemcpyHostToDevice, s));
    SFM_HIP(hipMemcpyAsync(S.d_view_new, is_new.data(), n_views, hipMemcpyHostToDevice, s));
    // extend
    RegExtendArgs E;
    E.unposed = S.d_unposed;
    E.clist = S.d_clist;
    E.view_off = V.d_view_off;
    E.cnt = S.d_cnt;
    E.obs_lm = V.d_obs_lm;
    E.view_intr = V.tri.d_view_intr;
    E.view_pose = V.tri.d_view_pose;
    E.intr_type = V.tri.d_intr_type;
    E.view_new = S.d_view_new;
    E.intr = V.tri.d_intr;
    E.pose_R = V.d_pose_R;
    E.pose_C = V.d_pose_C;
    E.obs_x = V.tri.d_obs_x;
    E.lm_X = V.tri.d_lm_X;
    E.thr = opt.residual_px;
    E.obs_keep = V.tri.d_obs_keep;
    E.extended = S.d_extended;
    if (longest)
      hipLaunchKernelGGL(k_reg_extend, dim3((longest + kRegBlock - 1) / kRegBlock, (unsigned)unposed.size()),
                         dim3(kRegBlock), 0, s, E);
    SFM_HIP(hipGetLastError());
    // new landmarks
    if (n_lm)
      hipLaunchKernelGGL(k_reg_select, dim3((n_lm + 255) / 256), dim3(256), 0, s, n_lm, V.tri.d_obs_off,
                         V.tri.d_obs_view, V.tri.d_view_pose, (const uint8_t *)V.d_pose_valid,
                         (const uint8_t *)S.d_view_new, (const uint8_t *)V.tri.d_lm_stage, S.d_select.get());
    SFM_HIP(hipGetLastError());
    SFM_HIP(hipMemcpyAsync(&S.h_extended, S.d_extended, sizeof S.h_extended, hipMemcpyDeviceToHost, s));
    SfmTriView T = V.tri;
    T.d_select = S.d_select;
    sfmloc_triangulate_options to;
    memset(&to, 0, sizeof to);
    to.mode = SFMLOC_TRI_ROBUST;
    to.min_inliers = opt.tri_min_inliers;
    to.allow_pairs = opt.tri_allow_pairs;
    to.residual_px = opt.residual_px;
    sfmloc_triangulate_report tr;
    rc = triangulate_run(T, to, &tr);  // (ends with the stream drained: `ext` has arrived)
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

int sfmloc_sfm_register(sfmloc_sfm *h, const sfmloc_register_options *opt, sfmloc_register_report *rep) {
  SFM_CHECK(h, SFMLOC_EINVAL, "sfmloc_sfm_register: null handle");
  sfmloc_register_options o;
  if (opt) o = *opt;
  else sfmloc_register_default_options(&o);
  SFM_CHECK(o.tri_min_inliers >= 2 && o.residual_px >= 0.0, SFMLOC_EINVAL,
            "sfmloc_sfm_register: tri_min_inliers must be at least 2 and residual_px not negative");
  if (rep) memset(rep, 0, sizeof *rep);
  SfmRegView V;
  sfm_reg_view(h, &V);
  SFM_CHECK(V.masks, SFMLOC_EINVAL,
            "sfmloc_sfm_register: the keep masks do not exist yet (after sfmloc_sfm_triangulate or sfmloc_sfm_clean)");
  SFM_HIP(hipSetDevice(V.device));
  try {
    return reg_run(V, o, rep);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_register: out of host memory");
    return SFMLOC_ENOMEM;
  }
}

int sfmloc_sfm_register_read(const sfmloc_sfm *h, sfmloc_sfm_view_result *out, int32_t *round) {
  SFM_CHECK(h, SFMLOC_EINVAL, "sfmloc_sfm_register_read: null handle");
  SfmRegView V;
  sfm_reg_view(const_cast<sfmloc_sfm *>(h), &V);
  const SfmRegState &S = *V.state;
  for (uint32_t k = 0; k < V.tri.n_views; ++k) {
    const bool have = k < S.res.size();
    if (out) {
      if (have) out[k] = S.res[k];
      else memset(&out[k], 0, sizeof out[k]);
    }
    if (round) round[k] = have ? S.round[k] : -1;
  }
  return SFMLOC_OK;
}

int sfmloc_sfm_register_inliers(const sfmloc_sfm *h, uint32_t k, uint32_t *idx, uint32_t cap, uint32_t *n) {
  SFM_CHECK(h && n, SFMLOC_EINVAL, "sfmloc_sfm_register_inliers: null argument");
  SfmRegView V;
  sfm_reg_view(const_cast<sfmloc_sfm *>(h), &V);
  SFM_CHECK(k < V.tri.n_views, SFMLOC_EINVAL, "sfmloc_sfm_register_inliers: view index %u out of range", k);
  static const std::vector<uint32_t> none;
  const std::vector<uint32_t> &v = k < V.state->inliers.size() ? V.state->inliers[k] : none;
  *n = (uint32_t)v.size();
  SFM_CHECK(!idx || cap >= v.size(), SFMLOC_ECAP, "sfmloc_sfm_register_inliers: %u entries, %zu inliers", cap, v.size());
  if (idx && !v.empty()) memcpy(idx, v.data(), v.size() * sizeof(uint32_t));
  return SFMLOC_OK;
}

}  // extern "C"
