// Device code the bundle adjustment kernels share (ba_separable.hip, ba_joint.hip; relrefine.hip takes the solve and the
// lambda rules): one observation's weighted residual and derivatives, the in-wave butterfly, the damped Cholesky solve,
// the rotation step and the Levenberg-Marquardt state.
// f64, unfused (the library's -ffp-contract=off); every expression is parenthesised explicitly, so both files round alike.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

namespace sfmloc {
namespace {

constexpr int kBaGroup = 8;        // lanes per landmark
constexpr int kBaMaxSteps = 500;   // steps tried per block
constexpr double kBaFtol = 1e-14;  // sfmloc.h "stopping"
constexpr double kHuberA = 16.0;   // HuberLoss(Square(4.0))

// one observation at camera coordinates Xc: the weighted residual r (2), the weighted d r / d Xc (2 x 3, rows J0 J1)
// and rho / 2 (sfmloc.h "residual", "loss"; first-order reweighting: both times sqrt(rho')).  kIntr (the joint
// adjustment): also the weighted d r / d intrinsic (2 x 6, rows I0 I1 over f, ppx, ppy, k1, k2, k3; the k columns are 0
// for a pinhole); without it I0, I1 are not touched
template <bool kIntr>
__device__ __forceinline__ double ba_observation(const double *__restrict__ K, bool radial, const double Xc[3],
                                                  double ox, double oy, double r[2], double J0[3], double J1[3],
                                                  double *I0 = nullptr, double *I1 = nullptr) {
  const double f = K[0];
  const double iz = 1.0 / Xc[2];
  const double p0 = Xc[0] / Xc[2], p1 = Xc[1] / Xc[2];
  double rc = 1.0, drc = 0.0, r2 = 0.0, r4 = 0.0, r6 = 0.0;
  if (radial) {
    r2 = p0 * p0 + p1 * p1;
    r4 = r2 * r2;
    r6 = r4 * r2;
    rc = ((1.0 + K[3] * r2) + K[4] * r4) + K[5] * r6;
    drc = (K[3] + 2.0 * K[4] * r2) + 3.0 * K[5] * r4;
  }
  r[0] = (f * (p0 * rc) + K[1]) - ox;
  r[1] = (f * (p1 * rc) + K[2]) - oy;
  // d q / d p of q = p rc(|p|^2), then d p / d Xc = [[iz, 0, -p0 iz], [0, iz, -p1 iz]]
  const double q00 = rc + 2.0 * drc * p0 * p0, q01 = 2.0 * drc * p0 * p1, q11 = rc + 2.0 * drc * p1 * p1;
  J0[0] = f * q00 * iz;
  J0[1] = f * q01 * iz;
  J0[2] = -f * (q00 * p0 + q01 * p1) * iz;
  J1[0] = f * q01 * iz;
  J1[1] = f * q11 * iz;
  J1[2] = -f * (q01 * p0 + q11 * p1) * iz;
  if constexpr (kIntr) {  // d r / d f = p rc, d r / d pp = I, d r / d k_j = f p r2^j
    I0[0] = p0 * rc;
    I0[1] = 1.0;
    I0[2] = 0.0;
    I0[3] = f * (p0 * r2);
    I0[4] = f * (p0 * r4);
    I0[5] = f * (p0 * r6);
    I1[0] = p1 * rc;
    I1[1] = 0.0;
    I1[2] = 1.0;
    I1[3] = f * (p1 * r2);
    I1[4] = f * (p1 * r4);
    I1[5] = f * (p1 * r6);
  }
  const double s = r[0] * r[0] + r[1] * r[1];
  if (s > kHuberA * kHuberA) {
    const double sq = sqrt(s);
    const double w = sqrt(kHuberA / sq);
    r[0] *= w;
    r[1] *= w;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      J0[k] *= w;
      J1[k] *= w;
    }
    if constexpr (kIntr) {
#pragma unroll
      for (int k = 0; k < 6; ++k) {
        I0[k] *= w;
        I1[k] *= w;
      }
    }
    return 0.5 * (2.0 * kHuberA * sq - kHuberA * kHuberA);
  }
  return 0.5 * s;
}

// the sum over the W lanes of a group (W = 8: a landmark's lanes, W = 64: the wave) as a butterfly: the same tree on
// every run, and every lane of the group ends with the same bits (a + b and b + a round alike)
template <int W>
__device__ __forceinline__ double ba_group_sum(double v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

// (A + lam D) d = -g by Cholesky, D = diag(A) clamped to [1e-6, 1e32]; A symmetric, full storage.  Returns false when a
// pivot is not positive or the step is not finite.  *model = -(g.d + d.A d / 2), the decrease the quadratic model promises.
template <int N>
__device__ __forceinline__ bool ba_solve(const double (&A)[N][N], const double (&g)[N], double lam, double (&d)[N],
                                         double *model) {
  double L[N][N];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < N; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
      if (i == j) {
        const double dd = fmin(fmax(A[i][i], 1e-6), 1e32);
        s += lam * dd;
      }
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) {
        ok = ok && (s > 0.0);
        L[i][i] = sqrt(s);
      } else {
        L[i][j] = s / L[j][j];
      }
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double s = -g[i];
#pragma unroll
    for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
    y[i] = s / L[i][i];
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double s = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) s -= L[k][i] * d[k];
    d[i] = s / L[i][i];
  }
  double gd = 0.0, dAd = 0.0;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    gd += g[i] * d[i];
    double s = 0.0;
#pragma unroll
    for (int j = 0; j < N; ++j) s += A[i][j] * d[j];
    dAd += d[i] * s;
    ok = ok && isfinite(d[i]);
  }
  *model = -(gd + 0.5 * dAd);
  return ok && (*model > 0.0);
}

struct BaLm {
  double lam = 1e-4, nu = 2.0;
  // after a trial: true = stop.  accepted: the caller has taken the trial point.
  __device__ __forceinline__ bool accepted(double c, double cn, double model) {
    const double q = (c - cn) / model;
    const double e = 2.0 * q - 1.0;
    lam = fmax(lam * fmax(1.0 / 3.0, 1.0 - e * e * e), 1e-32);
    nu = 2.0;
    return (c - cn) <= kBaFtol * c;
  }
  __device__ __forceinline__ bool rejected(double c, double model) {
    if (isfinite(model) && model <= kBaFtol * c) return true;
    lam *= nu;
    nu *= 2.0;
    return !(lam < 1e32);
  }
};

// Rn = exp([w]x) R
__device__ __forceinline__ void ba_rotate(const double w[3], const double R[9], double Rn[9]) {
  const double th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
  const double th = sqrt(th2);
  const bool small = th < 1e-4;
  const double a = small ? 1.0 - th2 / 6.0 : sin(th) / th;
  const double b = small ? 0.5 - th2 / 24.0 : (1.0 - cos(th)) / th2;
  // E = I + a K + b K^2, K = [w]x, K^2 = w w^T - th2 I
  double E[9];
  E[0] = 1.0 + b * (w[0] * w[0] - th2);
  E[4] = 1.0 + b * (w[1] * w[1] - th2);
  E[8] = 1.0 + b * (w[2] * w[2] - th2);
  E[1] = b * (w[0] * w[1]) - a * w[2];
  E[3] = b * (w[0] * w[1]) + a * w[2];
  E[2] = b * (w[0] * w[2]) + a * w[1];
  E[6] = b * (w[0] * w[2]) - a * w[1];
  E[5] = b * (w[1] * w[2]) - a * w[0];
  E[7] = b * (w[1] * w[2]) + a * w[0];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (E[3 * i] * R[j] + E[3 * i + 1] * R[3 + j]) + E[3 * i + 2] * R[6 + j];
}

}  // namespace
}  // namespace sfmloc
