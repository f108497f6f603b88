// The two-view point of one match on bearings, shared by the cheirality count of the relative poses (relpose.hip), the
// depths of the wedge scales (pairscales.hip) and the starting points of the two-view refinement (relrefine.hip):
// triangulate.hip's hypothesis from [I | 0] and [R | t].  Everything is in the anonymous namespace: each translation
// unit compiles its own copy, no device symbol crosses one.
#pragma once

#include "geom_device.h"

namespace sfmloc {
namespace {

// sfmloc.h "bearings": the pixel (x, y) of a view whose intrinsic is K = f, ppx, ppy, k1, k2, k3 of type 0 or 3
__device__ __forceinline__ void view_bearing(const double *K, uint32_t type, double x, double y, double *bx, double *by) {
  double ux = x, uy = y;
  if (type == 3) geom::ud_pixel_k3(K[0], K[1], K[2], K[3], K[4], K[5], x, y, &ux, &uy);
  *bx = (ux - K[1]) / K[0];
  *by = (uy - K[2]) / K[0];
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
