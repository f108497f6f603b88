// sfmloc_sfm: OpenMVG_BA without -c (OpenMVG_BA/src/adjust_sfm_data.cpp:89-155,245-260) on a device-resident
// sfm_data -- every view re-resected with K5, then the structure cleaned.  The semantics are stated in
// include/sfmloc.h; the kernels below name the paragraph of that statement they implement.
//
//   transpose   the observations (CSR by landmark) become per-view correspondence lists in ascending landmark id: a
//               stable LSD radix sort of the observation indices by view index, 8 bits per pass.  Each pass is a
//               per-block digit histogram, one exclusive scan over (digit, block) and a scatter whose rank inside the
//               block comes from wave ballots -- no atomic decides a position, so two runs give the same lists
//               (radix_sort.h, shared with tracks.hip).
//   resection   the lists go straight into the 2D-3D buffers of K5's contexts and K5 runs unchanged: init, rounds,
//               finish (sfm_data.h's sfm_resect_gang, shared with register.hip); every view that has more than 10
//               observations is tried, and whatever K5 answers is recorded.
//   cleanup     f64, unfused (the library's -ffp-contract=off): residual per observation, the clamped cosine of every
//               pair of a landmark's remaining observations (minimum kept), and the -r fixed point as one workgroup's
//               loop over pose counts (integer atomics: a count does not depend on order).  A later cleanup works on
//               what the earlier ones kept.
//   readers     sfmloc_sfm_read*, and what the other stages share of the handle (sfm_data.h): sfm_dev, the pose check,
//               the gang resection's contexts.
// The stages that work on the handle live beside their kernels and reach it through sfm_data.h: sfmloc_sfm_adjust in
// ba_separable.hip, sfmloc_sfm_adjust_joint in ba_joint.hip, sfmloc_sfm_triangulate in triangulate.hip,
// sfmloc_sfm_register in register.hip, sfmloc_sfm_color_plan in colorize.hip.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "radix_sort.h"
#include "sfm_data.h"
#include "sfm_json.h"

namespace sfmloc {
namespace {

// ---- transpose: observations by landmark -> per-view lists in ascending landmark id (sfmloc.h "views") -------------

__global__ __launch_bounds__(256) void k_adj_obs_landmark(const uint64_t *__restrict__ obs_off, uint32_t n_lm,
                                                          uint32_t *__restrict__ obs_lm, uint32_t *__restrict__ vlist) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lm) return;
  for (uint64_t o = obs_off[l]; o < obs_off[l + 1]; ++o) {
    obs_lm[o] = l;
    vlist[o] = (uint32_t)o;  // the sort's payload starts as the identity (landmark order)
  }
}

// view_off[v] = first position of view v in the sorted keys (lower bound), v = 0..n_views
__global__ __launch_bounds__(256) void k_adj_view_off(const uint32_t *__restrict__ key, uint32_t n, uint32_t n_views,
                                                      uint32_t *__restrict__ view_off) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v > n_views) return;
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (key[mid] < v) lo = mid + 1;
    else hi = mid;
  }
  view_off[v] = lo;
}

// ---- cleanup --------------------------------------------------------------------------------------------------------

// per observation: the residual norm (sfmloc.h "residual") and the world ray with its norm (sfmloc.h "angle")
__global__ __launch_bounds__(256) void k_adj_residual(uint64_t n_obs, const uint32_t *__restrict__ obs_lm,
                                                      const uint32_t *__restrict__ obs_view, const double *__restrict__ obs_x,
                                                      const double *__restrict__ lm_X, const uint32_t *__restrict__ view_intr,
                                                      const uint32_t *__restrict__ view_pose,
                                                      const uint32_t *__restrict__ intr_type, const double *__restrict__ intr,
                                                      const double *__restrict__ pose_R, const double *__restrict__ pose_C,
                                                      double thr, int again, double *__restrict__ res,
                                                      double *__restrict__ ray, uint8_t *__restrict__ keep) {
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_obs) return;
  const uint32_t l = obs_lm[o], v = obs_view[o];
  const uint32_t pi = view_pose[v], ii = view_intr[v];
  const double *R = pose_R + 9 * (size_t)pi;
  const double *C = pose_C + 3 * (size_t)pi;
  const double *K = intr + 6 * (size_t)ii;
  const bool radial = intr_type[ii] == 3;
  const double f = K[0], ppx = K[1], ppy = K[2];
  const double x = obs_x[2 * o], y = obs_x[2 * o + 1];
  // obs.x - cam2ima(add_disto(hnormalized(R (X - C))))
  double depth, px, py;
  geom::project_pixel(R, C, K, radial, lm_X + 3 * (size_t)l, &depth, &px, &py);
  const double ex = x - px, ey = y - py;
  const double nrm = sqrt(ex * ex + ey * ey);
  res[o] = nrm;
  const uint8_t was = again ? keep[o] : 1;  // (a later cleanup: what an earlier one removed stays removed)
  keep[o] = (nrm > thr) ? 0 : was;
  // bearing: get_ud_pixel (radial), K^-1 (x, y, 1), normalised, then R^T
  double ux = x, uy = y;
  if (radial) geom::ud_pixel_k3(f, ppx, ppy, K[3], K[4], K[5], x, y, &ux, &uy);
  const double b0 = (ux - ppx) / f, b1 = (uy - ppy) / f, b2 = 1.0;
  const double bn = sqrt((b0 * b0 + b1 * b1) + b2 * b2);
  const double c0 = b0 / bn, c1 = b1 / bn, c2 = b2 / bn;
  const double r0 = (R[0] * c0 + R[3] * c1) + R[6] * c2;
  const double r1 = (R[1] * c0 + R[4] * c1) + R[7] * c2;
  const double r2 = (R[2] * c0 + R[5] * c1) + R[8] * c2;
  ray[4 * o] = r0;
  ray[4 * o + 1] = r1;
  ray[4 * o + 2] = r2;
  ray[4 * o + 3] = sqrt((r0 * r0 + r1 * r1) + r2 * r2);
}

// per landmark: fewer than 2 observations left -> stage 0 (residual filter); else the minimum clamped cosine over all
// pairs -> stage 1 when acos(c) * 180 / pi < angle_deg (angle filter), else 3 (kept).  A later cleanup (again): a
// landmark an earlier one removed becomes stage 4 (gone before this cleanup began) and is not looked at
__global__ __launch_bounds__(256) void k_adj_landmarks(uint32_t n_lm, const uint64_t *__restrict__ obs_off,
                                                       const uint8_t *__restrict__ keep, const double *__restrict__ ray,
                                                       double angle_deg, int again, double *__restrict__ mincos,
                                                       uint8_t *__restrict__ stage) {
  const uint32_t l = blockIdx.x * 256 + threadIdx.x;
  if (l >= n_lm) return;
  if (again && stage[l] != 3) {
    stage[l] = 4;
    mincos[l] = geom::q_nan();
    return;
  }
  const uint64_t a = obs_off[l], b = obs_off[l + 1];
  uint32_t k = 0;
  for (uint64_t o = a; o < b; ++o) k += keep[o];
  if (k < 2) {
    stage[l] = 0;
    mincos[l] = geom::q_nan();
    return;
  }
  const double lo = -1.0 + 1.e-8, hi = 1.0 - 1.e-8;
  double cmin = hi;
  for (uint64_t i = a; i < b; ++i) {
    if (!keep[i]) continue;
    const double *r1 = ray + 4 * i;
    for (uint64_t j = i + 1; j < b; ++j) {
      if (!keep[j]) continue;
      const double *r2 = ray + 4 * j;
      const double dot = (r1[0] * r2[0] + r1[1] * r2[1]) + r1[2] * r2[2];
      const double mag = r1[3] * r2[3];
      double c = dot / mag;
      const double m = (hi < c) ? hi : c;  // std::max(lo, std::min(c, hi)): a NaN cosine becomes lo (180 degrees)
      c = (lo < m) ? m : lo;
      cmin = c < cmin ? c : cmin;
    }
  }
  mincos[l] = cmin;
  stage[l] = (acos(cmin) * 180.0 / 3.14159265358979323846 < angle_deg) ? 1 : 3;
}

// eraseUnstablePosesAndObservations(6, 2) as one workgroup's fixed-point loop (sfmloc.h "unstable"); stage 2 = a
// landmark this loop removed
__global__ __launch_bounds__(1024) void k_adj_unstable(uint32_t n_lm, const uint64_t *__restrict__ obs_off,
                                                       const uint32_t *__restrict__ obs_view,
                                                       const uint32_t *__restrict__ view_pose, uint32_t n_poses,
                                                       uint8_t *pose_valid, uint32_t *pose_cnt, uint8_t *keep,
                                                       uint8_t *stage, uint32_t min_pose, uint32_t min_lm,
                                                       uint32_t *passes) {
  __shared__ int erased, removed;
  const uint32_t t = threadIdx.x;
  uint32_t pass = 0;
  for (;;) {
    for (uint32_t p = t; p < n_poses; p += 1024) pose_cnt[p] = 0;
    __syncthreads();
    for (uint32_t l = t; l < n_lm; l += 1024) {
      if (stage[l] != 3) continue;
      for (uint64_t o = obs_off[l]; o < obs_off[l + 1]; ++o)
        if (keep[o]) atomicAdd(&pose_cnt[view_pose[obs_view[o]]], 1u);
    }
    if (t == 0) {
      erased = 0;
      removed = 0;
    }
    __syncthreads();
    ++pass;
    for (uint32_t p = t; p < n_poses; p += 1024)
      if (pose_valid[p] && pose_cnt[p] < min_pose) {
        pose_valid[p] = 0;
        atomicOr(&erased, 1);
      }
    __syncthreads();
    if (!erased) break;
    for (uint32_t l = t; l < n_lm; l += 1024) {
      if (stage[l] != 3) continue;
      uint32_t k = 0;
      for (uint64_t o = obs_off[l]; o < obs_off[l + 1]; ++o) {
        if (!keep[o]) continue;
        if (!pose_valid[view_pose[obs_view[o]]]) {
          keep[o] = 0;
          atomicOr(&removed, 1);
        } else {
          ++k;
        }
      }
      if (k < min_lm) stage[l] = 2;
    }
    __syncthreads();
    if (!removed) break;
  }
  if (t == 0) *passes = pass;
}

int sfm_transpose(Sfm *h) {
  const uint32_t n = (uint32_t)h->n_obs;
  hipStream_t s = h->s;
  if (h->n_lm)
    SFM_RC(dev_launch(k_adj_obs_landmark, dim3((h->n_lm + 255) / 256), dim3(256), 0, s, h->d_obs_off, h->n_lm,
                      h->d_obs_lm, h->d_vlist));
  if (n) SFM_RC(h->d_vkey.copy_from(h->d_obs_view, n, s));
  // (an odd number of passes leaves the result in the scratch pair)
  bool swapped = false;
  SFM_RC(radix_sort_pairs(h->d_vkey, h->d_vlist, h->d_tmp_k, h->d_tmp_v, n, radix_key_bits(h->n_views - 1), h->d_hist, s,
                          &swapped));
  if (swapped) {
    std::swap(h->d_vkey, h->d_tmp_k);
    std::swap(h->d_vlist, h->d_tmp_v);
  }
  SFM_RC(dev_launch(k_adj_view_off, dim3((h->n_views + 1 + 255) / 256), dim3(256), 0, s, h->d_vkey, n, h->n_views,
                    h->d_view_off));
  h->h_view_off.assign((size_t)h->n_views + 1, 0);
  SFM_RC(h->d_view_off.download(h->h_view_off.data(), (size_t)h->n_views + 1, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

int sfm_create_impl(const sfmloc_sfm_desc *d, const sfmloc_params *params, Sfm *h) {
  SFM_CHECK(d->n_views > 0 && d->view_id && d->view_intrinsic && d->view_pose, SFMLOC_EINVAL,
            "sfmloc_sfm_create: no views");
  SFM_CHECK(d->n_intrinsics > 0 && d->intrinsic_type && d->intrinsic, SFMLOC_EINVAL, "sfmloc_sfm_create: no intrinsics");
  SFM_CHECK(d->n_poses > 0 && d->pose_valid && d->pose_R && d->pose_C, SFMLOC_EINVAL, "sfmloc_sfm_create: no pose table");
  SFM_CHECK(d->obs_off && (d->n_landmarks == 0 || (d->landmark_id && d->landmark_X)), SFMLOC_EINVAL,
            "sfmloc_sfm_create: landmark arrays missing");
  SFM_CHECK(d->obs_off[0] == 0, SFMLOC_EINVAL, "sfmloc_sfm_create: obs_off[0] must be 0");
  for (uint32_t l = 0; l < d->n_landmarks; ++l) {
    SFM_CHECK(d->obs_off[l] <= d->obs_off[l + 1], SFMLOC_EINVAL, "sfmloc_sfm_create: obs_off not monotone at %u", l);
    SFM_CHECK(l == 0 || d->landmark_id[l - 1] < d->landmark_id[l], SFMLOC_EINVAL,
              "sfmloc_sfm_create: landmark_id must be strictly ascending at %u", l);
  }
  const uint64_t n_obs = d->obs_off[d->n_landmarks];
  SFM_CHECK(n_obs < (1ull << 31), SFMLOC_EINVAL, "sfmloc_sfm_create: more than 2^31 observations");
  SFM_CHECK(n_obs == 0 || (d->obs_view && d->obs_x), SFMLOC_EINVAL, "sfmloc_sfm_create: observation arrays missing");
  for (uint32_t v = 0; v < d->n_views; ++v) {
    SFM_CHECK(v == 0 || d->view_id[v - 1] < d->view_id[v], SFMLOC_EINVAL,
              "sfmloc_sfm_create: view_id must be strictly ascending at %u", v);
    SFM_CHECK(d->view_intrinsic[v] < d->n_intrinsics, SFMLOC_EINVAL,
              "sfmloc_sfm_create: view %u: intrinsic index out of range", d->view_id[v]);
    SFM_CHECK(d->view_pose[v] < d->n_poses, SFMLOC_EINVAL, "sfmloc_sfm_create: view %u: pose index out of range",
              d->view_id[v]);
  }
  for (uint32_t i = 0; i < d->n_intrinsics; ++i)
    SFM_CHECK(d->intrinsic_type[i] == 0 || d->intrinsic_type[i] == 3, SFMLOC_EIO,
              "sfmloc_sfm_create: intrinsic %u (table index): type %u is not supported (0 pinhole, 3 pinhole_radial_k3)", i, d->intrinsic_type[i]);
  for (uint64_t o = 0; o < n_obs; ++o)
    SFM_CHECK(d->obs_view[o] < d->n_views, SFMLOC_EINVAL, "sfmloc_sfm_create: obs_view[%llu] out of range",
              (unsigned long long)o);

  sfmloc_params p;
  if (params) p = *params;
  else sfmloc_sfm_default_params(&p);
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  SFM_CHECK(e == hipSuccess && ndev > 0, SFMLOC_ENODEV, "no HIP device visible; this library has no CPU fallback");
  SFM_CHECK(p.device >= 0 && p.device < ndev, SFMLOC_EINVAL, "device %d out of range (0..%d)", p.device, ndev - 1);
  SFM_HIP(hipSetDevice(p.device));
  h->device = p.device;
  h->params = p;
  h->n_views = d->n_views;
  h->n_intr = d->n_intrinsics;
  h->n_poses = d->n_poses;
  h->n_lm = d->n_landmarks;
  h->n_obs = n_obs;
  h->h_view_id.assign(d->view_id, d->view_id + d->n_views);
  h->h_view_intr.assign(d->view_intrinsic, d->view_intrinsic + d->n_views);
  h->h_view_pose.assign(d->view_pose, d->view_pose + d->n_views);
  h->h_intr_type.assign(d->intrinsic_type, d->intrinsic_type + d->n_intrinsics);
  h->h_intr.assign(d->intrinsic, d->intrinsic + 6 * (size_t)d->n_intrinsics);
  h->h_pose_valid.assign(d->pose_valid, d->pose_valid + d->n_poses);
  for (uint8_t &v : h->h_pose_valid) v = v ? 1 : 0;
  h->h_pose_R.assign(d->pose_R, d->pose_R + 9 * (size_t)d->n_poses);
  h->h_pose_C.assign(d->pose_C, d->pose_C + 3 * (size_t)d->n_poses);
  h->h_obs_off.assign(d->obs_off, d->obs_off + (size_t)d->n_landmarks + 1);
  h->h_obs_view.assign(d->obs_view, d->obs_view + n_obs);
  SFM_RC(h->s.create());
  hipStream_t s = h->s;
  // (views, intrinsics and poses are not empty; the landmark and observation arrays may be, and still get an address)
  const size_t lm1 = d->n_landmarks ? d->n_landmarks : 1, obs1 = n_obs ? n_obs : 1;
  SFM_RC(dev_upload(nullptr, h->d_view_id, d->view_id, d->n_views, s));
  SFM_RC(dev_upload(nullptr, h->d_view_intr, d->view_intrinsic, d->n_views, s));
  SFM_RC(dev_upload(nullptr, h->d_view_pose, d->view_pose, d->n_views, s));
  SFM_RC(dev_upload(nullptr, h->d_intr_type, d->intrinsic_type, d->n_intrinsics, s));
  SFM_RC(dev_upload(nullptr, h->d_intr, d->intrinsic, 6 * (size_t)d->n_intrinsics, s));
  SFM_RC(dev_upload(nullptr, h->d_pose_valid, h->h_pose_valid.data(), d->n_poses, s));
  SFM_RC(dev_upload(nullptr, h->d_pose_R, d->pose_R, 9 * (size_t)d->n_poses, s));
  SFM_RC(dev_upload(nullptr, h->d_pose_C, d->pose_C, 3 * (size_t)d->n_poses, s));
  SFM_RC(dev_upload(nullptr, h->d_lm_id, d->landmark_id, d->n_landmarks, s, 1));
  SFM_RC(dev_upload(nullptr, h->d_lm_X, d->landmark_X, 3 * (size_t)d->n_landmarks, s, 1));
  SFM_RC(dev_upload(nullptr, h->d_obs_off, d->obs_off, (size_t)d->n_landmarks + 1, s));
  SFM_RC(dev_upload(nullptr, h->d_obs_view, d->obs_view, n_obs, s, 1));
  SFM_RC(dev_upload(nullptr, h->d_obs_x, d->obs_x, 2 * n_obs, s, 1));
  SFM_RC(h->d_obs_lm.alloc(nullptr, obs1));
  SFM_RC(h->d_vlist.alloc(nullptr, obs1));
  SFM_RC(h->d_vkey.alloc(nullptr, obs1));
  SFM_RC(h->d_tmp_k.alloc(nullptr, obs1));
  SFM_RC(h->d_tmp_v.alloc(nullptr, obs1));
  SFM_RC(h->d_hist.alloc(nullptr, n_obs ? 256 * ((n_obs + kRadixBlock - 1) / kRadixBlock) : 1));
  SFM_RC(h->d_view_off.alloc(nullptr, (size_t)d->n_views + 1));
  SFM_RC(h->d_res.alloc(nullptr, obs1));
  SFM_RC(h->d_ray.alloc(nullptr, 4 * obs1));
  SFM_RC(h->d_obs_keep.alloc(nullptr, obs1));
  SFM_RC(h->d_mincos.alloc(nullptr, lm1));
  SFM_RC(h->d_lm_stage.alloc(nullptr, lm1));
  SFM_RC(h->d_pose_cnt.alloc(nullptr, d->n_poses));
  SFM_RC(h->d_passes.alloc(nullptr, 1));
  {
    std::vector<uint32_t> pv_off((size_t)d->n_poses + 1, 0), pv(d->n_views);
    for (uint32_t v = 0; v < d->n_views; ++v) ++pv_off[d->view_pose[v] + 1];
    for (uint32_t p = 0; p < d->n_poses; ++p) pv_off[p + 1] += pv_off[p];
    std::vector<uint32_t> at(pv_off.begin(), pv_off.end() - 1);
    for (uint32_t v = 0; v < d->n_views; ++v) pv[at[d->view_pose[v]]++] = v;  // (ascending view index inside a pose)
    SFM_RC(dev_upload(nullptr, h->d_pose_view_off, pv_off.data(), pv_off.size(), s));
    SFM_RC(dev_upload(nullptr, h->d_pose_views, pv.data(), pv.size(), s));
    SFM_HIP(hipStreamSynchronize(s));  // (the vectors leave scope)
  }
  SFM_RC(h->d_pose_t.alloc(nullptr, 3 * (size_t)d->n_poses));
  SFM_RC(h->d_blk_cost.alloc(nullptr, 2 * (size_t)std::max(d->n_poses, d->n_landmarks)));
  SFM_RC(h->d_blk_info.alloc(nullptr, (size_t)std::max(d->n_poses, d->n_landmarks)));
  SFM_RC(sfm_transpose(h));
  const uint32_t vid0 = 0, voff[2] = {0, 0};
  sfmloc_map_desc md;
  memset(&md, 0, sizeof md);
  md.n_views = 1;
  md.view_id = &vid0;
  md.view_off = voff;
  md.focal = 1.0;
  SFM_RC(sfmloc_map_create(&md, &h->params, &h->map));
  h->res.assign(d->n_views, sfmloc_sfm_view_result{});
  h->inliers.assign(d->n_views, std::vector<uint32_t>());
  return SFMLOC_OK;
}

int sfm_resect_impl(Sfm *h, uint32_t *n_ran, uint32_t *n_ok) {
  std::vector<uint32_t> todo, todo_n;
  for (uint32_t k = 0; k < h->n_views; ++k) {
    const uint32_t n = h->h_view_off[k + 1] - h->h_view_off[k];
    sfmloc_sfm_view_result &r = h->res[k];
    memset(&r, 0, sizeof r);
    r.n_obs = (int32_t)n;
    h->inliers[k].clear();
    if (n > 10) {  // MINIMUM_VIEW_NUM_TO_ESTIMATAE_CAMERA_POSE, test ">" (adjust_sfm_data.cpp:118)
      SFM_CHECK(n <= kSfmMaxViewObs, SFMLOC_ECAP, "view %u has %u observations (at most %u per view)", h->h_view_id[k],
                n, kSfmMaxViewObs);
      todo.push_back(k);
      todo_n.push_back(n);
    }
  }
  uint32_t ran = 0, ok = 0;
  // the transpose's lists as they are (no count array, raw pixels)
  const int rc = sfm_resect_gang<false>(*h, todo, todo_n, h->d_vlist, nullptr,
                                        [&](uint32_t k, const Pose &p) -> std::vector<uint32_t> & {
    sfmloc_sfm_view_result &r = h->res[k];
    r.ran = 1;
    r.ok = p.ok;
    r.n_inliers = p.n_inliers;
    r.iterations = p.iterations;
    r.error_max = p.error_max;
    r.nfa = p.nfa;
    memcpy(r.P, p.P, sizeof r.P);
    memcpy(r.R, p.R, sizeof r.R);
    memcpy(r.center, p.center, sizeof r.center);
    ++ran;
    if (p.ok) {  // (sfmloc.h "failure": a failed view keeps its input pose, or stays without one)
      ++ok;
      // Pose3(R, -R^T t) (adjust_sfm_data.cpp:138-142); a pose id without an entry gets one
      const uint32_t pi = h->h_view_pose[k];
      h->h_pose_valid[pi] = 1;
      memcpy(&h->h_pose_R[9 * (size_t)pi], p.R, 9 * sizeof(double));
      memcpy(&h->h_pose_C[3 * (size_t)pi], p.center, 3 * sizeof(double));
    }
    return h->inliers[k];
  });
  if (rc) return rc;
  SFM_RC(h->d_pose_valid.upload(h->h_pose_valid.data(), h->n_poses, h->s));
  SFM_RC(h->d_pose_R.upload(h->h_pose_R.data(), 9 * (size_t)h->n_poses, h->s));
  SFM_RC(h->d_pose_C.upload(h->h_pose_C.data(), 3 * (size_t)h->n_poses, h->s));
  SFM_HIP(hipStreamSynchronize(h->s));
  h->resected = true;
  if (n_ran) *n_ran = ran;
  if (n_ok) *n_ok = ok;
  return SFMLOC_OK;
}

// the keep masks of the last cleanup on the host (what a later cleanup or adjustment checks the poses against)
int sfm_fetch_masks(Sfm *h) {
  if (!h->cleaned) return SFMLOC_OK;
  h->h_obs_keep.resize(h->n_obs);
  h->h_lm_stage.resize(h->n_lm);
  if (h->n_obs) SFM_RC(h->d_obs_keep.download(h->h_obs_keep.data(), h->n_obs, h->s));
  if (h->n_lm) SFM_RC(h->d_lm_stage.download(h->h_lm_stage.data(), h->n_lm, h->s));
  SFM_HIP(hipStreamSynchronize(h->s));
  return SFMLOC_OK;
}

int sfm_clean_impl(Sfm *h, double residual_px, double angle_deg, int rm_unstable, uint64_t *counts) {
  const int rc_pose = sfm_check_poses(*h, "cleaned");
  if (rc_pose) return rc_pose;
  const int again = h->cleaned ? 1 : 0;  // a later cleanup works on what the earlier ones kept
  hipStream_t s = h->s;
  if (h->n_obs)
    SFM_RC(dev_launch(k_adj_residual, dim3((unsigned)((h->n_obs + 255) / 256)), dim3(256), 0, s, h->n_obs, h->d_obs_lm,
                      h->d_obs_view, h->d_obs_x, h->d_lm_X, h->d_view_intr, h->d_view_pose, h->d_intr_type, h->d_intr,
                      h->d_pose_R, h->d_pose_C, residual_px, again, h->d_res, h->d_ray, h->d_obs_keep));
  if (h->n_lm)
    SFM_RC(dev_launch(k_adj_landmarks, dim3((h->n_lm + 255) / 256), dim3(256), 0, s, h->n_lm, h->d_obs_off,
                      h->d_obs_keep, h->d_ray, angle_deg, again, h->d_mincos, h->d_lm_stage));
  if (rm_unstable) {
    SFM_RC(dev_launch(k_adj_unstable, dim3(1), dim3(1024), 0, s, h->n_lm, h->d_obs_off, h->d_obs_view, h->d_view_pose,
                      h->n_poses, h->d_pose_valid, h->d_pose_cnt, h->d_obs_keep, h->d_lm_stage, 6u, 2u, h->d_passes));
  }
  std::vector<uint8_t> stage(h->n_lm);
  if (h->n_lm) SFM_RC(h->d_lm_stage.download(stage.data(), h->n_lm, s));
  SFM_RC(h->d_pose_valid.download(h->h_pose_valid.data(), h->n_poses, s));
  SFM_HIP(hipStreamSynchronize(s));
  if (counts) {
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (uint8_t st : stage) {
      if (st == 4) continue;  // (gone before this cleanup)
      ++counts[0];
      counts[1] += st >= 1;
      counts[2] += st >= 2;
      counts[3] += st == 3;
    }
  }
  h->cleaned = true;
  return SFMLOC_OK;
}

}  // namespace

SfmDev sfm_dev(const Sfm &h, bool make_masks) {
  const bool masks = h.cleaned || make_masks;
  SfmDev d;
  d.n_views = h.n_views;
  d.n_intr = h.n_intr;
  d.n_poses = h.n_poses;
  d.n_lm = h.n_lm;
  d.n_obs = h.n_obs;
  d.view_id = h.d_view_id;
  d.view_intr = h.d_view_intr;
  d.view_pose = h.d_view_pose;
  d.intr_type = h.d_intr_type;
  d.intr = h.d_intr;
  d.pose_valid = h.d_pose_valid;
  d.pose_R = h.d_pose_R;
  d.pose_C = h.d_pose_C;
  d.pose_t = h.d_pose_t;
  d.lm_id = h.d_lm_id;
  d.lm_X = h.d_lm_X;
  d.obs_off = h.d_obs_off;
  d.obs_view = h.d_obs_view;
  d.obs_lm = h.d_obs_lm;
  d.vlist = h.d_vlist;
  d.view_off = h.d_view_off;
  d.obs_x = h.d_obs_x;
  d.obs_keep = masks ? h.d_obs_keep.get() : nullptr;  // (before the first cleanup: every observation enters)
  d.lm_stage = masks ? h.d_lm_stage.get() : nullptr;
  d.pose_view_off = h.d_pose_view_off;
  d.pose_views = h.d_pose_views;
  d.blk_cost = h.d_blk_cost;
  d.blk_info = h.d_blk_info;
  return d;
}

int sfm_ensure_contexts(Sfm &h, uint32_t n) {
  while (h.ctx.size() < n) {  // the first has a stream of its own, the others work on it (gang members)
    sfmloc_context *c = nullptr;
    const int rc = sfmloc_context_create_merge(h.map, h.ctx.empty() ? nullptr : h.ctx[0], &c);
    if (rc) return rc;
    h.ctx.push_back(c);
  }
  return SFMLOC_OK;
}

// GetPoseOrDie: the first observation (landmark order) still in the structure whose view has no pose
int sfm_check_poses(Sfm &h, const char *what) {
  const int rc = sfm_fetch_masks(&h);
  if (rc) return rc;
  for (uint32_t l = 0; l < h.n_lm; ++l) {
    if (h.cleaned && h.h_lm_stage[l] != 3) continue;
    for (uint64_t o = h.h_obs_off[l]; o < h.h_obs_off[l + 1]; ++o) {
      if (h.cleaned && !h.h_obs_keep[o]) continue;
      const uint32_t v = h.h_obs_view[o];
      SFM_CHECK(h.h_pose_valid[h.h_view_pose[v]], SFMLOC_EINVAL,
                "view %u has observations but no pose (GetPoseOrDie): the structure cannot be %s", h.h_view_id[v],
                what);
    }
  }
  return SFMLOC_OK;
}

// the host's copy of the pose table follows the device's (sfmloc_sfm_read reads it)
int sfm_fetch_poses(Sfm &h) {
  SFM_RC(h.d_pose_R.download(h.h_pose_R.data(), 9 * (size_t)h.n_poses, h.s));
  SFM_RC(h.d_pose_C.download(h.h_pose_C.data(), 3 * (size_t)h.n_poses, h.s));
  SFM_HIP(hipStreamSynchronize(h.s));
  return SFMLOC_OK;
}

}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_sfm_default_params(sfmloc_params *p) {
  if (!p) return;
  sfmloc_default_params(p);
  p->min_resection_points = 10;  // MINIMUM_VIEW_NUM_TO_ESTIMATAE_CAMERA_POSE (adjust_sfm_data.cpp:39,118)
  p->min_inliers = 7;            // Localize's own gate: vec_inliers > 2.5 * 3
  p->p3p_max_iteration = 4096;   // Image_Localizer_Match_Data::max_iteration
}

int sfmloc_sfm_create(const sfmloc_sfm_desc *desc, const sfmloc_params *params, sfmloc_sfm **out) {
  SFM_CHECK(desc && out, SFMLOC_EINVAL, "sfmloc_sfm_create: null argument");
  return make_handle<Sfm>("sfmloc_sfm_create", out, [&](Sfm *h) { return sfm_create_impl(desc, params, h); });
}

void sfmloc_sfm_destroy(sfmloc_sfm *h) { delete reinterpret_cast<Sfm *>(h); }

int sfmloc_sfm_resect(sfmloc_sfm *hh, uint32_t *n_ran, uint32_t *n_ok) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_resect: null handle");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_CHECK(!h->resected && !h->cleaned, SFMLOC_EINVAL, "sfmloc_sfm_resect: runs once, before the cleanup");
  SFM_HIP(hipSetDevice(h->device));
  try {
    return sfm_resect_impl(h, n_ran, n_ok);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_resect: out of host memory");
    return SFMLOC_ENOMEM;
  }
}

int sfmloc_sfm_resect_read(const sfmloc_sfm *hh, sfmloc_sfm_view_result *out) {
  SFM_CHECK(hh && out, SFMLOC_EINVAL, "sfmloc_sfm_resect_read: null argument");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  memcpy(out, h->res.data(), h->res.size() * sizeof(sfmloc_sfm_view_result));
  return SFMLOC_OK;
}

int sfmloc_sfm_resect_inliers(const sfmloc_sfm *hh, uint32_t k, uint32_t *idx, uint32_t cap, uint32_t *n) {
  SFM_CHECK(hh && n, SFMLOC_EINVAL, "sfmloc_sfm_resect_inliers: null argument");
  const Sfm *h = reinterpret_cast<const Sfm *>(hh);
  SFM_CHECK(k < h->n_views, SFMLOC_EINVAL, "sfmloc_sfm_resect_inliers: view index %u out of range", k);
  const std::vector<uint32_t> &v = h->inliers[k];
  *n = (uint32_t)v.size();
  SFM_CHECK(!idx || cap >= v.size(), SFMLOC_ECAP, "sfmloc_sfm_resect_inliers: %u entries, %zu inliers", cap, v.size());
  if (idx && !v.empty()) memcpy(idx, v.data(), v.size() * sizeof(uint32_t));
  return SFMLOC_OK;
}

int sfmloc_sfm_clean(sfmloc_sfm *hh, double residual_px, double angle_deg, int rm_unstable, uint64_t *counts) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_clean: null handle");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_HIP(hipSetDevice(h->device));
  return sfm_clean_impl(h, residual_px, angle_deg, rm_unstable, counts);
}

int sfmloc_sfm_read_intrinsics(sfmloc_sfm *hh, double *K) {
  SFM_CHECK(hh && K, SFMLOC_EINVAL, "sfmloc_sfm_read_intrinsics: null argument");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_HIP(hipSetDevice(h->device));
  SFM_RC(h->d_intr.read(K, 6 * (size_t)h->n_intr, h->s));
  return SFMLOC_OK;
}

int sfmloc_sfm_read_structure(sfmloc_sfm *hh, double *X) {
  SFM_CHECK(hh && X, SFMLOC_EINVAL, "sfmloc_sfm_read_structure: null argument");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_HIP(hipSetDevice(h->device));
  if (h->n_lm) SFM_RC(h->d_lm_X.read(X, 3 * (size_t)h->n_lm, h->s));
  return SFMLOC_OK;
}

int sfmloc_sfm_read(sfmloc_sfm *hh, uint8_t *pose_valid, double *pose_R, double *pose_C, uint8_t *obs_keep,
                    uint8_t *landmark_keep) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_read: null handle");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_CHECK(h->cleaned || (!obs_keep && !landmark_keep), SFMLOC_EINVAL,
            "sfmloc_sfm_read: the keep masks exist after the cleanup");
  SFM_HIP(hipSetDevice(h->device));
  if (pose_valid) memcpy(pose_valid, h->h_pose_valid.data(), h->n_poses);
  if (pose_R) memcpy(pose_R, h->h_pose_R.data(), 9 * (size_t)h->n_poses * sizeof(double));
  if (pose_C) memcpy(pose_C, h->h_pose_C.data(), 3 * (size_t)h->n_poses * sizeof(double));
  if (obs_keep && h->n_obs) SFM_RC(h->d_obs_keep.read(obs_keep, h->n_obs, h->s));
  if (landmark_keep && h->n_lm) {
    std::vector<uint8_t> st(h->n_lm);
    SFM_RC(h->d_lm_stage.read(st.data(), h->n_lm, h->s));
    for (uint32_t l = 0; l < h->n_lm; ++l) landmark_keep[l] = st[l] == 3 ? 1 : 0;
  }
  return SFMLOC_OK;
}

int sfmloc_sfm_debug_read(sfmloc_sfm *hh, double *residual, double *min_cos) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_debug_read: null handle");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  SFM_CHECK(h->cleaned, SFMLOC_EINVAL, "sfmloc_sfm_debug_read: after the cleanup only");
  SFM_HIP(hipSetDevice(h->device));
  if (residual && h->n_obs) SFM_RC(h->d_res.read(residual, h->n_obs, h->s));
  if (min_cos && h->n_lm) SFM_RC(h->d_mincos.read(min_cos, h->n_lm, h->s));
  return SFMLOC_OK;
}

int sfmloc_sfm_json_rewrite(const char *in_path, const char *out_path) {
  SFM_CHECK(in_path && out_path, SFMLOC_EINVAL, "sfmloc_sfm_json_rewrite: null argument");
  try {
    std::string text, err, out;
    SFM_CHECK(sfmjson::read_file(in_path, &text), SFMLOC_EIO, "%s: cannot be read", in_path);
    sfmjson::Value v;
    SFM_CHECK(sfmjson::parse(text, &v, &err), SFMLOC_EIO, "%s: %s", in_path, err.c_str());
    sfmjson::dump(v, &out);
    SFM_CHECK(sfmjson::write_file(out_path, out), SFMLOC_EIO, "%s: cannot be written", out_path);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_json_rewrite: out of host memory");
    return SFMLOC_ENOMEM;
  }
  return SFMLOC_OK;
}

}  // extern "C"
