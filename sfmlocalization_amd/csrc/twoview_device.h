// The two-view point of one match on bearings, shared by the cheirality count of the relative poses (relpose.hip), the
// depths of the wedge scales (pairscales.hip) and the starting points of the two-view refinement (relrefine.hip):
// triangulate.hip's hypothesis from [I | 0] and [R | t].  Before it, the scene those three calls share as it sits in
// device memory: PairDev and PairPosesDev, the pointers every kernel of theirs takes (its argument struct derives from
// them), and PairSceneBufs and PairPosesBufs, which own the arrays for the length of a call.  Everything is in the
// anonymous namespace: each translation unit compiles its own copy, no device symbol crosses one.
#pragma once

#include <vector>

#include "geom_device.h"
#include "pair_scene.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

// a PairScene (pair_scene.h) on the device; view_wh is null where the call was given none
struct PairDev {
  uint32_t n_views, n_pairs;
  const uint64_t *view_off, *offsets;
  const float *kpt;
  const uint32_t *view_wh, *view_intr, *intr_type, *pairs, *match_i, *match_j;
  const double *intr;
};

// a PairPoses on the device; use[k] is 0 or 1, all 1 where the caller passed no use_pair
struct PairPosesDev {
  const double *relR, *relt;
  const uint64_t *inl_off;
  const uint32_t *inl_idx;
  const uint8_t *use;
};

struct PairSceneBufs {
  DevBuf<uint64_t> view_off, offsets;
  DevBuf<float> kpt;
  DevBuf<uint32_t> wh, vintr, itype, pairs, mi, mj;
  DevBuf<double> intr;
  PairDev D{};
  int upload(const PairScene &sc, hipStream_t s) {
    const size_t n = sc.n_views, P = sc.n_pairs, total = (size_t)sc.offsets[P];
    SFM_RC(dev_upload(nullptr, view_off, sc.view_off, n + 1, s));
    SFM_RC(dev_upload(nullptr, kpt, sc.kpt_xy, 2 * (size_t)sc.view_off[n], s));
    if (sc.view_wh) SFM_RC(dev_upload(nullptr, wh, sc.view_wh, 2 * n, s));
    SFM_RC(dev_upload(nullptr, vintr, sc.view_intrinsic, n, s));
    SFM_RC(dev_upload(nullptr, intr, sc.intrinsics, 6 * (size_t)sc.n_intrinsics, s));
    SFM_RC(dev_upload(nullptr, itype, sc.intrinsic_type, (size_t)sc.n_intrinsics, s));
    SFM_RC(dev_upload(nullptr, pairs, sc.pairs, 2 * P, s));
    SFM_RC(dev_upload(nullptr, offsets, sc.offsets, P + 1, s));
    SFM_RC(dev_upload(nullptr, mi, sc.match_i, total, s));
    SFM_RC(dev_upload(nullptr, mj, sc.match_j, total, s));
    D = PairDev{sc.n_views, sc.n_pairs, view_off, offsets, kpt, wh, vintr, itype, pairs, mi, mj, intr};
    return SFMLOC_OK;
  }
  const PairDev &dev() const { return D; }
};

struct PairPosesBufs {
  DevBuf<double> relR, relt;
  DevBuf<uint64_t> inl_off;
  DevBuf<uint32_t> inl_idx;
  DevBuf<uint8_t> use;
  PairPosesDev D{};
  int upload(const PairScene &sc, const PairPoses &po, hipStream_t s) {
    const size_t P = sc.n_pairs;
    std::vector<uint8_t> use01(P, 1);
    if (po.use_pair)
      for (size_t k = 0; k < P; ++k) use01[k] = po.use_pair[k] ? 1 : 0;
    SFM_RC(dev_upload(nullptr, relR, po.rel_R, 9 * P, s));
    SFM_RC(dev_upload(nullptr, relt, po.rel_t, 3 * P, s));
    SFM_RC(dev_upload(nullptr, inl_off, po.inlier_off, P + 1, s));
    SFM_RC(dev_upload(nullptr, inl_idx, po.inlier_idx, (size_t)po.inlier_off[P], s));
    SFM_RC(dev_upload(nullptr, use, use01.data(), P, s));
    D = PairPosesDev{relR, relt, inl_off, inl_idx, use};
    return SFMLOC_OK;
  }
  const PairPosesDev &dev() const { return D; }
};

// sfmloc.h "bearings": the pixel (x, y) of a view whose intrinsic is K = f, ppx, ppy, k1, k2, k3 of type 0 or 3
__device__ __forceinline__ void view_bearing(const double *K, uint32_t type, double x, double y, double *bx, double *by) {
  double ux = x, uy = y;
  if (type == 3) geom::ud_pixel_k3(K[0], K[1], K[2], K[3], K[4], K[5], x, y, &ux, &uy);
  *bx = (ux - K[1]) / K[0];
  *by = (uy - K[2]) / K[0];
}

// what every feature of one view of the scene shares: its intrinsic K and that one's type, its first feature row
struct ViewCam {
  const double *K;
  uint32_t type;
  uint64_t row0;
};
__device__ __forceinline__ ViewCam view_cam(const PairDev &D, uint32_t v) {
  const uint32_t ii = D.view_intr[v];
  return ViewCam{D.intr + 6 * (size_t)ii, D.intr_type[ii], D.view_off[v]};
}

// ... of feature f of the view of c; a kernel that walks one view's features keeps c
__device__ __forceinline__ void feature_bearing(const PairDev &D, const ViewCam &c, uint32_t f, double *__restrict__ bx,
                                                double *__restrict__ by) {
  const uint64_t row = c.row0 + f;
  view_bearing(c.K, c.type, (double)D.kpt[2 * row], (double)D.kpt[2 * row + 1], bx, by);
}

// sfmloc.h "cheirality": false when no point exists; else X the point in I's frame, *zi = X_2 and *zj = (R X + t)_2
__device__ __forceinline__ bool two_view_point(const double *R, const double *t, double a, double b, double u, double v,
                                               double X[3], double *zi, double *zj) {
  using namespace geom;
  const double P1[12] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0};
  const double P2[12] = {R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]};
  double G[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) G[i][j] = 0.0;
#pragma unroll
  for (int side = 0; side < 2; ++side) {
    const double *P = side ? P2 : P1;
    const double bx = side ? u : a, by = side ? v : b;
    double ra[4], rb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ra[j] = bx * P[8 + j] - P[j];
      rb[j] = by * P[8 + j] - P[4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = i; j < 4; ++j) {
        G[i][j] = G[i][j] + ra[i] * ra[j];
        G[i][j] = G[i][j] + rb[i] * rb[j];
      }
  }
#pragma unroll
  for (int i = 1; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) G[i][j] = G[j][i];
  double V[4][4];
  jacobi_fixed<4>(G, V);
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
  const double X0 = x0 / w, X1 = x1 / w, X2 = x2 / w;
  X[0] = X0;
  X[1] = X1;
  X[2] = X2;
  *zi = X2;
  *zj = ((R[6] * X0 + R[7] * X1) + R[8] * X2) + t[2];
  return w != 0.0 && is_finite(w) && is_finite(X0) && is_finite(X1) && is_finite(X2);
}

// the depths alone
__device__ __forceinline__ bool two_view_depths(const double *R, const double *t, double a, double b, double u, double v,
                                                double *zi, double *zj) {
  double X[3];
  return two_view_point(R, t, a, b, u, v, X, zi, zj);
}

}  // namespace
}  // namespace sfmloc
