// sfmloc_sfm_triangulate: every landmark of a resident sfm_data triangulated from the views' known poses (the robust
// structure computation of openMVG_main_ComputeStructureFromKnownPoses / GlobalSfM's last stage).  The semantics are
// stated in include/sfmloc.h ("sfmloc_sfm_triangulate"); tests/structure_np.py restates every operation.  f64, only
// + - * / sqrt, unfused (the library's -ffp-contract=off), every sum in a fixed order, no float atomics.
//
//   views       k_tri_views: P = K [R | t] per view, once.
//   pixels      k_tri_pixels: get_ud_pixel per observation, once (the bisection is the expensive part of a row).
//   landmarks   k_tri_landmarks: kTriLanes lanes per landmark.  Lane g runs the rounds g, g + kTriLanes, ...: sample,
//               4 x 4 normal matrix of the two views' rows, Jacobi, and the inlier count over the landmark's list, all
//               inside the lane, so no sum crosses a lane.  The lanes' best rounds meet in a butterfly over a total
//               order (count, sum of squares, round); then every lane of the group repeats the final N-view solve on
//               the winner's inliers (the same bits in each, the lanes would idle otherwise) and lane 0 writes.
//               Tracks are short (2 to 10 observations mostly): one workgroup per track would leave the chip idle and
//               one lane per track would run its 2 n solves back to back; DESIGN.md has the reasoning and the timings.
//               With a select mask (sfmloc_sfm_register's new landmarks) only the landmarks it names are worked on and
//               written; sfmloc_sfm_triangulate passes none.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include "sfm_data.h"

namespace sfmloc {
namespace {

constexpr int kTriLanes = 8;    // lanes per landmark (a power of two, at most 64)
constexpr int kTriBlock = 256;  // 32 landmarks per workgroup

// the resident arrays (SfmDev; the masks are written) and this call's options and workspace
struct TriArgs : SfmDev {
  uint32_t mode, min_inliers, allow_pairs;
  double thr;
  uint64_t seed;  // the sampling key (sfmloc_params.seed of the handle)
  const double *ud, *P;
  const uint8_t *select;         // null: every landmark; else only those with select[l] != 0, the others untouched
  unsigned long long *counters;  // kept, too few posed, no hypothesis, too few inliers, observations kept, rounds
};

// sfmloc.h "projection": P = K [R | t], t_i = -((R_i0 C0 + R_i1 C1) + R_i2 C2)
__global__ __launch_bounds__(256) void k_tri_views(uint32_t n_views, const uint32_t *__restrict__ view_intr,
                                                   const uint32_t *__restrict__ view_pose,
                                                   const double *__restrict__ intr, const double *__restrict__ pose_R,
                                                   const double *__restrict__ pose_C, double *__restrict__ P) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= n_views) return;
  const double *R = pose_R + 9 * (size_t)view_pose[v], *C = pose_C + 3 * (size_t)view_pose[v];
  const double *K = intr + 6 * (size_t)view_intr[v];
  const double f = K[0], ppx = K[1], ppy = K[2];
  double M[12];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    M[4 * i] = R[3 * i];
    M[4 * i + 1] = R[3 * i + 1];
    M[4 * i + 2] = R[3 * i + 2];
    M[4 * i + 3] = -((R[3 * i] * C[0] + R[3 * i + 1] * C[1]) + R[3 * i + 2] * C[2]);
  }
  double *out = P + 12 * (size_t)v;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    out[j] = f * M[j] + ppx * M[8 + j];
    out[4 + j] = f * M[4 + j] + ppy * M[8 + j];
    out[8 + j] = M[8 + j];
  }
}

// sfmloc.h "ray": the undistorted pixel of every observation (its own pixel for a pinhole)
__global__ __launch_bounds__(256) void k_tri_pixels(uint64_t n_obs, const uint32_t *__restrict__ obs_view,
                                                    const double *__restrict__ obs_x,
                                                    const uint32_t *__restrict__ view_intr,
                                                    const uint32_t *__restrict__ intr_type,
                                                    const double *__restrict__ intr, double *__restrict__ ud) {
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (o >= n_obs) return;
  const uint32_t ii = view_intr[obs_view[o]];
  const double *K = intr + 6 * (size_t)ii;
  const double x = obs_x[2 * o], y = obs_x[2 * o + 1];
  double ux = x, uy = y;
  if (intr_type[ii] == 3) geom::ud_pixel_k3(K[0], K[1], K[2], K[3], K[4], K[5], x, y, &ux, &uy);
  ud[2 * o] = ux;
  ud[2 * o + 1] = uy;
}

__device__ __forceinline__ bool tri_posed(const TriArgs &A, uint64_t o) {
  return A.pose_valid[A.view_pose[A.obs_view[o]]] != 0;
}

// sfmloc.h "two-view hypothesis": the rows x P2 - P0 and y P2 - P1 of observation o added to G (upper triangle), the
// first row's products before the second's
__device__ __forceinline__ void tri_add_rows(const TriArgs &A, uint64_t o, double (&G)[4][4]) {
  const double *P = A.P + 12 * (size_t)A.obs_view[o];
  const double ux = A.ud[2 * o], uy = A.ud[2 * o + 1];
  double a[4], b[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    a[j] = ux * P[8 + j] - P[j];
    b[j] = uy * P[8 + j] - P[4 + j];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = i; j < 4; ++j) {
      G[i][j] = G[i][j] + a[i] * a[j];
      G[i][j] = G[i][j] + b[i] * b[j];
    }
}

__device__ __forceinline__ void tri_zero(double (&G)[4][4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) G[i][j] = 0.0;
}

// the eigenvector of G's smallest eigenvalue (the first smallest diagonal entry after the Jacobi sweeps), dehomogenised;
// false for a zero or non-finite w or a non-finite point
__device__ __forceinline__ bool tri_solve(double (&G)[4][4], double *X) {
#pragma unroll
  for (int i = 1; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) G[i][j] = G[j][i];
  double V[4][4];
  geom::jacobi_fixed<4>(G, V);
  double best = G[0][0], x0 = V[0][0], x1 = V[1][0], x2 = V[2][0], w = V[3][0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const bool take = G[i][i] < best;
    best = take ? G[i][i] : best;
    x0 = take ? V[0][i] : x0;
    x1 = take ? V[1][i] : x1;
    x2 = take ? V[2][i] : x2;
    w = take ? V[3][i] : w;
  }
  X[0] = x0 / w;
  X[1] = x1 / w;
  X[2] = x2 / w;
  return w != 0.0 && geom::is_finite(w) && geom::is_finite(X[0]) && geom::is_finite(X[1]) && geom::is_finite(X[2]);
}

// sfmloc.h "inliers": depth and pixel residual of X in observation o, on the projection the cleanup's residual uses
// (geom::project_pixel); *sq = the squared residual
__device__ __forceinline__ bool tri_inlier(const TriArgs &A, uint64_t o, const double *X, bool depth_only, double *sq) {
  const uint32_t v = A.obs_view[o];
  const uint32_t ii = A.view_intr[v];
  const double *R = A.pose_R + 9 * (size_t)A.view_pose[v];
  const double *C = A.pose_C + 3 * (size_t)A.view_pose[v];
  const double *K = A.intr + 6 * (size_t)ii;
  double X2, px, py;
  geom::project_pixel(R, C, K, A.intr_type[ii] == 3, X, &X2, &px, &py);
  const double ex = A.obs_x[2 * o] - px, ey = A.obs_x[2 * o + 1] - py;
  const double s = ex * ex + ey * ey;
  *sq = s;
  return X2 > 0.0 && (depth_only || sqrt(s) <= A.thr);  // (a NaN residual is not <= thr)
}

// the k-th posed observation of the list o0 .. o1 (k < the number of posed ones)
__device__ __forceinline__ uint64_t tri_nth_posed(const TriArgs &A, uint64_t o0, uint64_t o1, int k) {
  uint64_t o = o0;
  for (; o < o1; ++o) {
    if (!tri_posed(A, o)) continue;
    if (k == 0) break;
    --k;
  }
  return o;
}

// one landmark on its kTriLanes lanes (g = the lane's place in the group).  status: 0 kept, 1 too few posed
// observations, 2 no valid hypothesis, 3 too few inliers; every lane of the group returns the same values
__device__ __forceinline__ int tri_landmark(const TriArgs &A, uint32_t l, int g, double *X, uint32_t *n_rounds) {
  const uint64_t o0 = A.obs_off[l], o1 = A.obs_off[l + 1];
  const bool blind = A.mode == SFMLOC_TRI_BLIND;
  uint32_t n = 0;
  for (uint64_t o = o0; o < o1; ++o) n += tri_posed(A, o) ? 1u : 0u;
  *n_rounds = 0;
  X[0] = X[1] = X[2] = 0.0;
  if (n < 2) return 1;
  double G[4][4];
  if (blind) {  // sfmloc.h "blind mode": the N-view solve over every posed observation
    tri_zero(G);
    for (uint64_t o = o0; o < o1; ++o)
      if (tri_posed(A, o)) tri_add_rows(A, o, G);
    if (!tri_solve(G, X)) {
      X[0] = X[1] = X[2] = 0.0;
      return 2;
    }
  } else {
    const uint32_t rounds = n == 2 ? 1u : 2u * n;
    *n_rounds = rounds;
    int best_cnt = -1;  // (-1: no round of this lane had a hypothesis)
    double best_ssq = 0.0, bX0 = 0.0, bX1 = 0.0, bX2 = 0.0;
    uint32_t best_r = 0;
    for (uint32_t r = (uint32_t)g; r < rounds; r += kTriLanes) {
      int32_t smp[2];
      geom::ac_sample<2>(nullptr, (int)n, A.seed, geom::STAGE_TRIANGULATE, A.lm_id[l], r, smp);
      tri_zero(G);
      tri_add_rows(A, tri_nth_posed(A, o0, o1, smp[0]), G);
      tri_add_rows(A, tri_nth_posed(A, o0, o1, smp[1]), G);
      double H[3];
      if (!tri_solve(G, H)) continue;
      int cnt = 0;
      double ssq = 0.0, sq;
      for (uint64_t o = o0; o < o1; ++o)
        if (tri_posed(A, o) && tri_inlier(A, o, H, false, &sq)) {
          ++cnt;
          ssq = ssq + sq;
        }
      if (cnt > best_cnt || (cnt == best_cnt && ssq < best_ssq)) {  // (a later round must be strictly better)
        best_cnt = cnt;
        best_ssq = ssq;
        best_r = r;
        bX0 = H[0];
        bX1 = H[1];
        bX2 = H[2];
      }
    }
    // sfmloc.h "winner": most inliers, then the smaller sum of squares, then the earlier round -- a total order, so the
    // butterfly leaves the same winner in every lane
#pragma unroll
    for (int m = 1; m < kTriLanes; m <<= 1) {
      const int oc = __shfl_xor(best_cnt, m, kTriLanes);
      const double os = __shfl_xor(best_ssq, m, kTriLanes);
      const uint32_t orr = (uint32_t)__shfl_xor((int)best_r, m, kTriLanes);
      const double ox0 = __shfl_xor(bX0, m, kTriLanes), ox1 = __shfl_xor(bX1, m, kTriLanes),
                   ox2 = __shfl_xor(bX2, m, kTriLanes);
      const bool better = oc > best_cnt || (oc == best_cnt && (os < best_ssq || (os == best_ssq && orr < best_r)));
      best_cnt = better ? oc : best_cnt;
      best_ssq = better ? os : best_ssq;
      best_r = better ? orr : best_r;
      bX0 = better ? ox0 : bX0;
      bX1 = better ? ox1 : bX1;
      bX2 = better ? ox2 : bX2;
    }
    if (best_cnt < 0) return 2;
    // sfmloc.h "final point": the N-view solve over the winner's inliers
    const double W[3] = {bX0, bX1, bX2};
    tri_zero(G);
    int cnt = 0;
    double sq;
    for (uint64_t o = o0; o < o1; ++o)
      if (tri_posed(A, o) && tri_inlier(A, o, W, false, &sq)) {
        tri_add_rows(A, o, G);
        ++cnt;
      }
    if (cnt < 2) return 3;
    if (!tri_solve(G, X)) {
      X[0] = X[1] = X[2] = 0.0;
      return 2;
    }
  }
  // sfmloc.h "keep rule": the final inliers, counted once
  uint32_t cnt = 0;
  double sq;
  for (uint64_t o = o0; o < o1; ++o) cnt += (tri_posed(A, o) && tri_inlier(A, o, X, blind, &sq)) ? 1u : 0u;
  const uint32_t need = (n == 2 && A.allow_pairs) ? 2u : A.min_inliers;
  if (cnt >= need) return 0;
  X[0] = X[1] = X[2] = 0.0;
  return 3;
}

__global__ __launch_bounds__(kTriBlock) void k_tri_landmarks(TriArgs A) {
  __shared__ unsigned int s_cnt[6];
  if (threadIdx.x < 6) s_cnt[threadIdx.x] = 0;
  __syncthreads();
  const uint32_t l = (blockIdx.x * (uint32_t)kTriBlock + threadIdx.x) / kTriLanes;
  const int g = threadIdx.x % kTriLanes;
  if (l < A.n_lm && (!A.select || A.select[l])) {  // (the kTriLanes lanes of a landmark agree)
    double X[3];
    uint32_t rounds;
    const int status = tri_landmark(A, l, g, X, &rounds);
    if (g == 0) {
      const bool blind = A.mode == SFMLOC_TRI_BLIND;
      uint32_t kept = 0;
      double sq;
      for (uint64_t o = A.obs_off[l]; o < A.obs_off[l + 1]; ++o) {
        const bool in = status == 0 && tri_posed(A, o) && tri_inlier(A, o, X, blind, &sq);
        A.obs_keep[o] = in ? 1 : 0;
        kept += in ? 1u : 0u;
      }
      A.lm_X[3 * (size_t)l] = X[0];
      A.lm_X[3 * (size_t)l + 1] = X[1];
      A.lm_X[3 * (size_t)l + 2] = X[2];
      A.lm_stage[l] = status == 0 ? 3 : 0;  // (the stages of the cleanup: 3 = kept)
      atomicAdd(&s_cnt[status], 1u);        // (integer counts: the same whatever the order)
      atomicAdd(&s_cnt[4], kept);
      atomicAdd(&s_cnt[5], rounds);
    }
  }
  __syncthreads();
  if (threadIdx.x < 6 && s_cnt[threadIdx.x]) atomicAdd(A.counters + threadIdx.x, (unsigned long long)s_cnt[threadIdx.x]);
}

}  // namespace

int triangulate_run(Sfm &h, const sfmloc_triangulate_options &opt, sfmloc_triangulate_report *rep,
                    const uint8_t *d_select) {
  CallScope d;  // (on the handle's stream; before the buffers: destroyed after them)
  hipStream_t s = h.s;
  DevBuf<double> d_P;
  DevBuf<unsigned long long> d_cnt;
  int rc = d_P.alloc(nullptr, 12 * (size_t)h.n_views);
  if (rc) return rc;
  rc = d_cnt.alloc(nullptr, 6);
  if (rc) return rc;
  double ms = 0.0;
  if ((rc = d.open(true, &ms, s)) || (rc = d.time_begin())) return rc;
  unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};
  SFM_RC(d_cnt.zero(6, s));
  TriArgs A;
  static_cast<SfmDev &>(A) = sfm_dev(h, true);  // (this call makes the masks)
  A.mode = opt.mode;
  A.min_inliers = opt.min_inliers;
  A.allow_pairs = opt.allow_pairs;
  A.thr = opt.residual_px;
  A.seed = h.params.seed;
  A.ud = h.d_ray;  // (the cleanup's ray scratch, 4 doubles per observation: every cleanup rewrites it)
  A.P = d_P;
  A.select = d_select;
  A.counters = d_cnt;
  SFM_RC(dev_launch(k_tri_views, dim3((h.n_views + 255) / 256), dim3(256), 0, s, h.n_views, A.view_intr, A.view_pose,
                    A.intr, A.pose_R, A.pose_C, d_P));
  if (h.n_obs)
    SFM_RC(dev_launch(k_tri_pixels, dim3((unsigned)((h.n_obs + 255) / 256)), dim3(256), 0, s, h.n_obs, A.obs_view,
                      A.obs_x, A.view_intr, A.intr_type, A.intr, h.d_ray));
  if (h.n_lm) {
    const uint64_t lanes = (uint64_t)h.n_lm * kTriLanes;
    SFM_RC(dev_launch(k_tri_landmarks, dim3((unsigned)((lanes + kTriBlock - 1) / kTriBlock)), dim3(kTriBlock), 0, s,
                      A));
  }
  if ((rc = d.time_end())) return rc;
  SFM_RC(d_cnt.download(cnt, 6, s));
  SFM_HIP(hipStreamSynchronize(s));
  if (rep) {
    rep->landmarks_in = h.n_lm;
    rep->landmarks_kept = cnt[0];
    rep->failed_posed = cnt[1];
    rep->failed_hypothesis = cnt[2];
    rep->failed_inliers = cnt[3];
    rep->obs_in = h.n_obs;
    rep->obs_kept = cnt[4];
    rep->rounds = cnt[5];
    rep->device_ms = ms;
  }
  return SFMLOC_OK;
}

}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_triangulate_default_options(sfmloc_triangulate_options *o) {
  if (!o) return;
  memset(o, 0, sizeof *o);
  o->mode = SFMLOC_TRI_ROBUST;
  o->min_inliers = 3;
  o->allow_pairs = 1;
  o->residual_px = 4.0;
}

int sfmloc_sfm_triangulate(sfmloc_sfm *hh, const sfmloc_triangulate_options *opt, sfmloc_triangulate_report *rep) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_triangulate: null handle");
  sfmloc_triangulate_options o;
  if (opt) o = *opt;
  else sfmloc_triangulate_default_options(&o);
  SFM_CHECK(o.mode == SFMLOC_TRI_ROBUST || o.mode == SFMLOC_TRI_BLIND, SFMLOC_EINVAL,
            "sfmloc_sfm_triangulate: mode = %u (0 robust, 1 blind)", o.mode);
  SFM_CHECK(o.min_inliers >= 2 && o.residual_px >= 0.0, SFMLOC_EINVAL,
            "sfmloc_sfm_triangulate: min_inliers must be at least 2 and residual_px not negative");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  if (rep) memset(rep, 0, sizeof *rep);
  SFM_HIP(hipSetDevice(h->device));
  const int rc = triangulate_run(*h, o, rep);
  if (rc) return rc;
  h->cleaned = true;  // the masks exist: a cleanup or an adjustment that follows works on what was kept
  return SFMLOC_OK;
}

}  // extern "C"
