// The device-resident sfm_data behind the opaque sfmloc_sfm handle, for the six files that work on it: adjust.hip (the
// handle's life, the transpose, the re-resection, the cleanup, the readers), ba_separable.hip, ba_joint.hip,
// triangulate.hip, register.hip and colorize.hip.  One declaration of the resident arrays (Sfm owns them, SfmDev is
// what kernels see of them) and one gang resection driver (sfm_resect_gang: adjust.hip's re-resection, register.hip's
// growth step).
#pragma once

#include <string.h>

#include <algorithm>
#include <vector>

#include "geom_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {

constexpr uint32_t kSfmGang = kGangMembers;  // views per gang session of a resection
constexpr uint32_t kSfmMaxViewObs = 65536;   // a view's list must fit a context's 2D-3D buffers (make_ctx: 65 536)

// what sfmloc_sfm_register (register.hip) keeps between rounds and calls
struct SfmRegState {
  std::vector<sfmloc_sfm_view_result> res;     // per view: the last round that tried it
  std::vector<int32_t> round;                  // that round, or -1
  std::vector<uint32_t> last_cnt;              // its correspondence count then
  std::vector<std::vector<uint32_t>> inliers;
  uint32_t rounds_done = 0;
  unsigned long long h_extended = 0;
  DevBuf<uint32_t> d_clist, d_cnt, d_unposed;  // compacted lists [n_obs], their lengths [n_views], the unposed views
  DevBuf<uint8_t> d_view_new, d_select;        // [n_views] registered this round, [n_lm] to be triangulated
  DevBuf<unsigned long long> d_extended;
};

struct Sfm {
  int device = 0;
  sfmloc_params params{};
  Stream s;  // (before the buffers: devmem.h, order of destruction)
  uint32_t n_views = 0, n_intr = 0, n_poses = 0, n_lm = 0;
  uint64_t n_obs = 0;
  // host copies of what the host-side rules need (the pose check of the cleanup, the per-view launches)
  std::vector<uint32_t> h_view_id, h_view_intr, h_view_pose, h_intr_type;
  std::vector<double> h_intr;
  std::vector<uint8_t> h_pose_valid;
  std::vector<double> h_pose_R, h_pose_C;
  std::vector<uint64_t> h_obs_off;
  std::vector<uint32_t> h_obs_view;
  std::vector<uint32_t> h_view_off;  // per-view list offsets (read back after the device transpose)
  std::vector<sfmloc_sfm_view_result> res;
  std::vector<std::vector<uint32_t>> inliers;
  bool resected = false, cleaned = false;
  // device
  DevBuf<uint32_t> d_view_id, d_view_intr, d_view_pose, d_intr_type;
  DevBuf<double> d_intr;
  DevBuf<uint8_t> d_pose_valid;
  DevBuf<double> d_pose_R, d_pose_C;
  DevBuf<uint32_t> d_lm_id;
  DevBuf<double> d_lm_X;
  DevBuf<uint64_t> d_obs_off;
  DevBuf<uint32_t> d_obs_view, d_obs_lm;
  DevBuf<double> d_obs_x;
  DevBuf<uint32_t> d_vlist, d_vkey, d_view_off, d_hist;
  DevBuf<uint32_t> d_tmp_k, d_tmp_v;
  DevBuf<double> d_res, d_ray, d_mincos;  // (d_ray, 4 doubles per observation, is also triangulate.hip's pixel scratch)
  DevBuf<uint8_t> d_obs_keep, d_lm_stage;
  DevBuf<uint32_t> d_pose_cnt, d_passes;
  // the adjustments: t = -R C per pose, every pose's views (CSR by pose, ascending view index), a block's costs and
  // outcome; host copies of the keep masks for the pose check of a call after a cleanup
  DevBuf<double> d_pose_t, d_blk_cost;
  DevBuf<uint32_t> d_pose_view_off, d_pose_views, d_blk_info;
  std::vector<uint8_t> h_obs_keep, h_lm_stage;
  // K5's contexts hang off a map without descriptors: its log10 table, parameters and launch heuristics
  sfmloc_map *map = nullptr;
  std::vector<sfmloc_context *> ctx;
  SfmRegState reg;
  // the stream is drained, then K5's contexts and their map go; the buffers and the stream follow as members
  ~Sfm() {
    hipSetDevice(device);
    if (s) hipStreamSynchronize(s);
    for (sfmloc_context *c : ctx) sfmloc_context_destroy(c);
    sfmloc_map_destroy(map);  // (null: nothing)
  }
};

// The resident arrays as kernels take them, by value.  vlist = observation indices sorted by view, ascending landmark
// inside a view, view_off [n_views + 1] (the transpose); obs_lm = an observation's landmark; pose_view_off /
// pose_views = every pose's views in ascending view index; pose_t [n_poses * 3], blk_cost [2 * n_blocks] (a block's
// cost before and after) and blk_info [n_blocks] (steps tried | entered << 29 | moved << 30 | at the cap << 31) are
// scratch.
// obs_keep / lm_stage (3 = kept) are null while the masks do not exist: every observation enters.
struct SfmDev {
  uint32_t n_views, n_intr, n_poses, n_lm;
  uint64_t n_obs;
  const uint32_t *view_id, *view_intr, *view_pose, *intr_type;
  double *intr;
  uint8_t *pose_valid;
  double *pose_R, *pose_C, *pose_t;
  const uint32_t *lm_id;
  double *lm_X;
  const uint64_t *obs_off;
  const uint32_t *obs_view, *obs_lm, *vlist, *view_off;
  const double *obs_x;
  uint8_t *obs_keep, *lm_stage;
  const uint32_t *pose_view_off, *pose_views;
  double *blk_cost;
  uint32_t *blk_info;
};

// adjust.hip.  sfm_dev: built from the handle's buffers at every use and never kept -- the transpose's sort swaps
// d_vlist with its scratch -- and the one place that decides whether the masks are null; make_masks: the caller writes them
// (triangulate.hip).  sfm_check_poses: GetPoseOrDie over what is still in the structure ("... cannot be <what>").
// sfm_fetch_poses: the host's pose table follows the device's.  sfm_ensure_contexts: at least n K5 contexts in h.ctx.
SfmDev sfm_dev(const Sfm &h, bool make_masks = false);
int sfm_check_poses(Sfm &h, const char *what);
int sfm_fetch_poses(Sfm &h);
int sfm_ensure_contexts(Sfm &h, uint32_t n);
// ba_separable.hip: t = -R C of every pose into pose_t, the first launch of either adjustment
int ba_pose_t(const SfmDev &v, hipStream_t s);
// triangulate.hip: sfmloc_sfm_triangulate's body; d_select [n_lm] or null (all): a landmark with 0 is not touched
int triangulate_run(Sfm &h, const sfmloc_triangulate_options &opt, sfmloc_triangulate_report *rep,
                    const uint8_t *d_select = nullptr);

namespace {

// A view's correspondence list into a context's 2D-3D buffers (it stands where k_match_set_finish stands on the query
// path): entries list[view_off[v] ..] of view v, cnt[v] of them, or the view's whole slice without a count array.  The
// pixel as it is (sfmloc.h "raw pixels") or, kUndistort, undistorted for pinhole_radial_k3 (ii = the view's intrinsic).
// The inlier pairs then name positions in the list.
template <bool kUndistort>
struct SfmFillBody {
  static constexpr int kGangThreads = 256;
  static __device__ __forceinline__ void run(const uint32_t *list, const uint32_t *view_off, const uint32_t *cnt,
                                             uint32_t v, uint32_t ii, const uint32_t *obs_lm, const double *obs_x,
                                             const double *lm_X, const uint32_t *lm_id, const uint32_t *intr_type,
                                             const double *intr, uint32_t *ms_n, uint32_t *ms_qfeat,
                                             uint32_t *ms_landmark, double *pt2d, double *pt3d) {
    const uint32_t b = view_off[v], n = cnt ? cnt[v] : view_off[v + 1] - b;
    const double *K = nullptr;
    bool radial = false;
    if constexpr (kUndistort) {
      K = intr + 6 * (size_t)ii;
      radial = intr_type[ii] == 3;
    }
    for (uint32_t k = threadIdx.x; k < n; k += 256) {
      const uint32_t o = list[b + k], l = obs_lm[o];
      const double x = obs_x[2 * (size_t)o], y = obs_x[2 * (size_t)o + 1];
      double ux = x, uy = y;
      if constexpr (kUndistort)
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
template <bool kUndistort>
__global__ __launch_bounds__(256) void k_sfm_fill(const uint32_t *list, const uint32_t *view_off, const uint32_t *cnt,
                                                  uint32_t v, uint32_t ii, const uint32_t *obs_lm, const double *obs_x,
                                                  const double *lm_X, const uint32_t *lm_id, const uint32_t *intr_type,
                                                  const double *intr, uint32_t *ms_n, uint32_t *ms_qfeat,
                                                  uint32_t *ms_landmark, double *pt2d, double *pt3d) {
  SfmFillBody<kUndistort>::run(list, view_off, cnt, v, ii, obs_lm, obs_x, lm_X, lm_id, intr_type, intr, ms_n, ms_qfeat,
                               ms_landmark, pt2d, pt3d);
}

// K5 on the views todo[i] (view indices) with todo_n[i] correspondences each, kSfmGang per gang session, every view on
// its own sampling stream (its id_view: independent of the batch) and with its own intrinsic.  A member's buffers are
// filled from d_list / d_cnt (SfmFillBody).  done(k, pose) is called once per view, in todo's order, with K5's answer: it
// keeps what the caller wants of it and returns the vector that receives the view's inlier set -- positions in the
// view's list: the pair list of a success, the best model's list (AC-RANSAC order) of a failure.
template <bool kUndistort, class Done>
int sfm_resect_gang(Sfm &h, const std::vector<uint32_t> &todo, const std::vector<uint32_t> &todo_n,
                    const uint32_t *d_list, const uint32_t *d_cnt, Done &&done) {
  int rc = sfm_ensure_contexts(h, std::min<uint32_t>(kSfmGang, (uint32_t)todo.size()));
  if (rc) return rc;
  const SfmDev d = sfm_dev(h);
  auto member = [&](uint32_t i) { return reinterpret_cast<Ctx *>(h.ctx[i]); };
  for (size_t g0 = 0; g0 < todo.size(); g0 += kSfmGang) {
    const uint32_t m = (uint32_t)std::min<size_t>(kSfmGang, todo.size() - g0);
    for (uint32_t i = 0; i < m; ++i) {  // (a regrowth synchronises: before the session records anything)
      Ctx *c = member(i);
      const uint32_t k = todo[g0 + i];
      rc = ctx_p3p_reserve(c, todo_n[g0 + i]);
      if (rc) return rc;
      const double *K = &h.h_intr[6 * (size_t)h.h_view_intr[k]];
      c->p3p_stream = h.h_view_id[k];
      c->p3p_own_K = true;
      c->p3p_K[0] = K[0];
      c->p3p_K[1] = K[1];
      c->p3p_K[2] = K[2];
    }
    rc = sfmloc_gang_begin(h.ctx.data(), m);
    if (rc) return rc;
    for (uint32_t i = 0; i < m && rc == SFMLOC_OK; ++i) {
      Ctx *c = member(i);
      const uint32_t k = todo[g0 + i];
      SFM_RC(sfm_launch<SfmFillBody<kUndistort>>(c, k_sfm_fill<kUndistort>, dim3(1), dim3(256), 0, d_list, d.view_off,
                                                 d_cnt, k, h.h_view_intr[k], d.obs_lm, d.obs_x, d.lm_X, d.lm_id,
                                                 d.intr_type, d.intr, c->d_ms_n, c->d_ms_qfeat, c->d_ms_landmark,
                                                 c->d_pt2d, c->d_pt3d));
      c->p3p_init_fused = false;  // K5's init reads the count the fill wrote
      rc = ctx_resection_begin(c);
    }
    const int rc_end = sfmloc_gang_end(h.ctx.data(), m);
    if (rc) return rc;
    if (rc_end) return rc_end;
    std::vector<std::pair<Ctx *, std::vector<uint32_t> *>> failed;  // views that failed with a non-empty inlier set
    for (uint32_t i = 0; i < m; ++i) {
      Ctx *c = member(i);
      const uint32_t k = todo[g0 + i];
      rc = ctx_resection_wait_done(c);
      if (rc) return rc;
      const HostResult *hr = c->h_result;
      const Pose &p = hr->pose;
      SFM_CHECK((p.status & 4) == 0, SFMLOC_ECAP, "view %u: more correspondences than the P3P workspace holds",
                h.h_view_id[k]);
      std::vector<uint32_t> &inl = done(k, p);
      const uint32_t ni = p.n_inliers > 0 ? (uint32_t)p.n_inliers : 0u;
      inl.resize(ni);
      if (!p.ok) {  // K5 publishes no pair list for a failed query: its best model's list, after the gang's last wait
        if (ni) failed.emplace_back(c, &inl);
      } else if (c->p3p_cap > (uint32_t)kP3pMaxN) {  // (a regrown workspace keeps its pair lists outside the record)
        SFM_RC(dev_read(inl.data(), c->d_pair_qfeat, ni, c->stream));
      } else {
        memcpy(inl.data(), hr->pair_qfeat, ni * sizeof(uint32_t));
      }
    }
    // (h.s is not the contexts' stream: the waits above have seen their work finish.  One wait for all failed views.)
    for (const auto &f : failed)
      SFM_RC(f.first->d_best_inl.download(f.second->data(), f.second->size(), h.s));
    if (!failed.empty()) SFM_HIP(hipStreamSynchronize(h.s));
  }
  for (sfmloc_context *cc : h.ctx) reinterpret_cast<Ctx *>(cc)->p3p_own_K = false;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc
