// sfmloc_refine_relative_poses: the two-view adjustment of every relative pose on its inliers (what OpenMVG does to a
// pair before it averages).  The semantics are stated in include/sfmloc.h ("Two-view refinement");
// tests/relrefine_np.py restates every operation.  f64, unfused (the library's -ffp-contract=off), only + - * / sqrt,
// every sum in a fixed order, no float atomics: the records are the restatement's bits.  Scene and poses: PairScene and
// PairPoses on the host (pair_scene.h), PairDev and PairPosesDev on the device (twoview_device.h), the bases of RrDev.
//
//   k_relrefine   one workgroup of 256 threads per pair, the whole Levenberg-Marquardt loop inside the kernel.  Lane l
//                 owns the inliers l, l + 256, ... from the triangulation to the end: nobody reads a point another
//                 lane wrote, so the slabs in global memory need no fence.  A step is two passes over the points:
//                   linearise   per point the 3 x 3 block, the 5 x 3 coupling and the gradient; its part of the reduced
//                               5 x 5 system and of the cost, 21 sums through the workgroup's tree (rr_block_sums).
//                   solve       thread 0: ba_solve<5> (ba_device.h), the step and the promised decrease through LDS.
//                   trial       the point's linearisation again (recomputing it costs less than the 24 doubles per
//                               point that keeping it would), its step, the trial point to the second slab, the cost
//                               there; one sum and one flag (a depth that is not finite and positive).
//                 Acceptance swaps the two slab pointers.  BaLm and kBaFtol (ba_device.h) decide as they do for the
//                 separable bundle adjustment.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "ba_device.h"
#include "ransac_device.h"
#include "relrefine_host.h"
#include "twoview_device.h"

namespace sfmloc {
namespace {

constexpr int kRrThreads = 256;
constexpr int kRrSums = 21;  // the reduced system's upper triangle by rows 0..14, its gradient 15..19, sum r^2 20

thread_local double g_relrefine_last_ms = 0.0;

struct Relrefine {
  std::vector<sfmloc_relrefine_result> res;
};

struct RrDev : PairDev, PairPosesDev {
  double *bear;         // [4][n] per pair at 4 inl_off[k]: a, b (view I), u, v (view J)
  double *pts, *trial;  // [3][n] per pair at 3 inl_off[k]; X_2 = 0 marks an inlier that is not used
  sfmloc_relrefine_result *res;
  // (behind the pointers: the kernel sits at the register limit, and with these two between the bases and the
  // pointers it measured 1 % slower -- profiles/pair_scene_time.json)
  uint32_t max_steps, min_points;
};

// sfmloc.h "reduction": v[k] over the workgroup, the same bits in every thread.  sh [N][4].
template <int N>
__device__ __forceinline__ void rr_block_sums(double (&v)[N], double (*sh)[4]) {
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ba_group_sum<64>(v[k]);
  __syncthreads();  // the sums of the pass before are no longer read
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < N; ++k) sh[k][threadIdx.x >> 6] = v[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; ++k) v[k] = ((sh[k][0] + sh[k][1]) + sh[k][2]) + sh[k][3];
}

// sfmloc.h "parameters": the tangent basis of the unit sphere at t, B[i][0] = b1, B[i][1] = b2
__device__ __forceinline__ void rr_basis(const double t[3], double B[3][2]) {
  const double a0 = geom::dabs(t[0]), a1 = geom::dabs(t[1]), a2 = geom::dabs(t[2]);
  int k = 0;
  double m = a0;
  if (a1 < m) {
    k = 1;
    m = a1;
  }
  if (a2 < m) k = 2;
  // c = t x e_k
  const double c0 = k == 0 ? 0.0 : k == 1 ? -t[2] : t[1];
  const double c1 = k == 0 ? t[2] : k == 1 ? 0.0 : -t[0];
  const double c2 = k == 0 ? -t[1] : k == 1 ? t[0] : 0.0;
  const double n = sqrt((c0 * c0 + c1 * c1) + c2 * c2);
  const double b0 = c0 / n, b1 = c1 / n, b2 = c2 / n;
  B[0][0] = b0;
  B[1][0] = b1;
  B[2][0] = b2;
  B[0][1] = t[1] * b2 - t[2] * b1;
  B[1][1] = t[2] * b0 - t[0] * b2;
  B[2][1] = t[0] * b1 - t[1] * b0;
}

// Rn = C(w) R, Cayley's C as k_gp_trial's (globalposes.hip)
__device__ __forceinline__ void rr_rotate(const double w[3], const double R[9], double Rn[9]) {
  const double xx = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2], f = 2.0 / (1.0 + xx);
  const double K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j)
      M[3 * i + j] = (i == j ? 1.0 : 0.0) + f * (K[3 * i + j] + (w[i] * w[j] - (i == j ? xx : 0.0)));
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) Rn[3 * i + j] = (M[3 * i] * R[j] + M[3 * i + 1] * R[3 + j]) + M[3 * i + 2] * R[6 + j];
}

// tn = (t + B d) / |t + B d|
__device__ __forceinline__ void rr_translate(const double t[3], const double B[3][2], double d0, double d1, double tn[3]) {
  double v[3];
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = t[i] + (B[i][0] * d0 + B[i][1] * d1);
  const double n = sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
#pragma unroll
  for (int i = 0; i < 3; ++i) tn[i] = v[i] / n;
}

// sfmloc.h "status": E = [t]x R over its Frobenius norm, zeros where that is zero
__device__ __forceinline__ void rr_essential(const double R[9], const double t[3], double E[9]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    E[j] = t[1] * R[6 + j] - t[2] * R[3 + j];
    E[3 + j] = t[2] * R[j] - t[0] * R[6 + j];
    E[6 + j] = t[0] * R[3 + j] - t[1] * R[j];
  }
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) s = s + E[i] * E[i];
  const double n = sqrt(s);
#pragma unroll
  for (int i = 0; i < 9; ++i) E[i] = n > 0.0 ? E[i] / n : 0.0;
}

// sfmloc.h "residual" of the point X at (R, t): r [4], Z = R X, Y = Z + t.  False when a depth is not finite and positive.
__device__ __forceinline__ bool rr_residual(const double R[9], const double t[3], double fi, double fj, const double X[3],
                                            const double b[4], double r[4], double Z[3], double Y[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    Z[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2];
    Y[i] = Z[i] + t[i];
  }
  r[0] = fi * (X[0] / X[2] - b[0]);
  r[1] = fi * (X[1] / X[2] - b[1]);
  r[2] = fj * (Y[0] / Y[2] - b[2]);
  r[3] = fj * (Y[1] / Y[2] - b[3]);
  return X[2] > 0.0 && geom::is_finite(X[2]) && Y[2] > 0.0 && geom::is_finite(Y[2]);
}

__device__ __forceinline__ double rr_sq(const double r[4]) { return ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]) + r[3] * r[3]; }

// the inverse of a symmetric positive definite 3 x 3 by Cholesky (jt_inv_spd of ba_joint.hip); a pivot that is not
// positive gives NaNs, the step that follows is then not finite and counts as rejected
__device__ __forceinline__ void rr_inv3(const double (&A)[3][3], double (&Ai)[3][3]) {
  double L[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j <= i; ++j) {
      double s = A[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) s -= L[i][k] * L[j][k];
      if (i == j) L[i][i] = sqrt(s > 0.0 ? s : -1.0);
      else L[i][j] = s / L[j][j];
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double y[3], d[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < i; ++k) s -= L[i][k] * y[k];
      y[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 2; i >= 0; --i) {
      double s = y[i];
#pragma unroll
      for (int k = i + 1; k < 3; ++k) s -= L[k][i] * d[k];
      d[i] = s / L[i][i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) Ai[i][c] = d[i];
  }
}

// sfmloc.h "step", one point at (R, t, X) under lambda: Vi = Vd^-1, W, gx = Jx^T r, the point's part of the reduced
// system (Ap: upper triangle by rows, gp) and r^2
__device__ __forceinline__ void rr_point(const double R[9], const double t[3], const double B[3][2], double fi, double fj,
                                         double lam, const double X[3], const double b[4], double (&Vi)[3][3],
                                         double (&W)[5][3], double (&gx)[3], double (&Ap)[15], double (&gp)[5], double *sq) {
  double r[4], Z[3], Y[3];
  rr_residual(R, t, fi, fj, X, b, r, Z, Y);
  *sq = rr_sq(r);
  // Jx [4 x 3] = d r / d X: rows 0, 1 the first view's, rows 2, 3 = (d r / d Y) R
  const double ix = 1.0 / X[2], iy = 1.0 / Y[2];
  const double d = fi * ix, e0 = -(fi * (X[0] / X[2])) * ix, e1 = -(fi * (X[1] / X[2])) * ix;
  const double a = fj * iy, c0 = -(fj * (Y[0] / Y[2])) * iy, c1 = -(fj * (Y[1] / Y[2])) * iy;
  double Jx[4][3] = {{d, 0.0, e0}, {0.0, d, e1}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}};
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    Jx[2][k] = a * R[k] + c0 * R[6 + k];
    Jx[3][k] = a * R[3 + k] + c1 * R[6 + k];
  }
  // Jp [2 x 5] = d (r2, r3) / d (w, d): (d r / d Y) (-2 [Z]x | B)
  double P0[5], P1[5];
  P0[0] = 2.0 * (c0 * Z[1]);
  P0[1] = 2.0 * (a * Z[2] - c0 * Z[0]);
  P0[2] = -2.0 * (a * Z[1]);
  P1[0] = 2.0 * (c1 * Z[1] - a * Z[2]);
  P1[1] = -2.0 * (c1 * Z[0]);
  P1[2] = 2.0 * (a * Z[0]);
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    P0[3 + m] = a * B[0][m] + c0 * B[2][m];
    P1[3 + m] = a * B[1][m] + c1 * B[2][m];
  }
  double V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) {
      V[i][j] = ((Jx[0][i] * Jx[0][j] + Jx[1][i] * Jx[1][j]) + Jx[2][i] * Jx[2][j]) + Jx[3][i] * Jx[3][j];
      V[j][i] = V[i][j];
    }
    gx[i] = ((Jx[0][i] * r[0] + Jx[1][i] * r[1]) + Jx[2][i] * r[2]) + Jx[3][i] * r[3];
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) V[i][i] = V[i][i] + lam * fmin(fmax(V[i][i], 1e-6), 1e32);
  rr_inv3(V, Vi);
  double F[5][3];  // W Vd^-1
#pragma unroll
  for (int q = 0; q < 5; ++q) {
#pragma unroll
    for (int i = 0; i < 3; ++i) W[q][i] = P0[q] * Jx[2][i] + P1[q] * Jx[3][i];
#pragma unroll
    for (int i = 0; i < 3; ++i) F[q][i] = (W[q][0] * Vi[0][i] + W[q][1] * Vi[1][i]) + W[q][2] * Vi[2][i];
    gp[q] = (P0[q] * r[2] + P1[q] * r[3]) - ((F[q][0] * gx[0] + F[q][1] * gx[1]) + F[q][2] * gx[2]);
  }
  int n = 0;
#pragma unroll
  for (int q = 0; q < 5; ++q)
#pragma unroll
    for (int p = q; p < 5; ++p)
      Ap[n++] = (P0[q] * P0[p] + P1[q] * P1[p]) - ((F[q][0] * W[p][0] + F[q][1] * W[p][1]) + F[q][2] * W[p][2]);
}

__global__ __launch_bounds__(kRrThreads) void k_relrefine(RrDev D) {
  __shared__ double sh[kRrSums][4];
  __shared__ double s_x[5], s_model;
  __shared__ int s_ok;
  __shared__ uint32_t s_used;
  const uint32_t k = blockIdx.x;
  if (k >= D.n_pairs) return;
  const uint32_t tid = threadIdx.x;
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = D.relR[9 * (size_t)k + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = D.relt[3 * (size_t)k + i];
  const uint64_t i0 = D.inl_off[k];
  const size_t n = (size_t)(D.inl_off[k + 1] - i0);
  double *bear = D.bear + 4 * i0, *X = D.pts + 3 * i0, *Xn = D.trial + 3 * i0;
  uint32_t status = 0, n_used = 0, steps = 0;
  double c0 = 0.0, c = 0.0;
  if (D.use[k]) {  // (the same in every thread of the workgroup, as every branch on the way to a barrier below)
    const uint32_t vi = D.pairs[2 * (size_t)k], vj = D.pairs[2 * (size_t)k + 1];
    const ViewCam ci = view_cam(D, vi), cj = view_cam(D, vj);
    const double fi = ci.K[0], fj = cj.K[0];
    const uint64_t m0 = D.offsets[k];
    if (tid == 0) s_used = 0;
    __syncthreads();
    // sfmloc.h "bearings", "points"
    uint32_t mine = 0;
    for (size_t p = tid; p < n; p += kRrThreads) {
      const uint64_t mt = m0 + D.inl_idx[i0 + p];
      double b[4], P[3], zi, zj;
      feature_bearing(D, ci, D.match_i[mt], &b[0], &b[1]);
      feature_bearing(D, cj, D.match_j[mt], &b[2], &b[3]);
      const bool ok =
          two_view_point(R, t, b[0], b[1], b[2], b[3], P, &zi, &zj) && geom::is_finite(zj) && zi > 0.0 && zj > 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) bear[q * n + p] = b[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) X[q * n + p] = Xn[q * n + p] = ok ? P[q] : 0.0;
      mine += ok ? 1u : 0u;
    }
    atomicAdd(&s_used, mine);  // (an integer count: the same whatever the order)
    __syncthreads();
    n_used = s_used;
    if (n_used < D.min_points) {
      status = 2;
    } else {
      BaLm lm;
      bool stop = false, moved = false, finite0 = true;
      double B[3][2];
      rr_basis(t, B);
      while (!stop && steps < D.max_steps) {
        ++steps;
        // linearise
        double acc[kRrSums];
#pragma unroll
        for (int q = 0; q < kRrSums; ++q) acc[q] = 0.0;
        for (size_t p = tid; p < n; p += kRrThreads) {
          const double P[3] = {X[p], X[n + p], X[2 * n + p]};
          if (!(P[2] > 0.0)) continue;
          const double b[4] = {bear[p], bear[n + p], bear[2 * n + p], bear[3 * n + p]};
          double Vi[3][3], W[5][3], gx[3], Ap[15], gp[5], sq;
          rr_point(R, t, B, fi, fj, lm.lam, P, b, Vi, W, gx, Ap, gp, &sq);
#pragma unroll
          for (int q = 0; q < 15; ++q) acc[q] += Ap[q];
#pragma unroll
          for (int q = 0; q < 5; ++q) acc[15 + q] += gp[q];
          acc[20] += sq;
        }
        rr_block_sums<kRrSums>(acc, sh);
        if (steps == 1) {
#pragma unroll
          for (int q = 0; q < kRrSums; ++q) finite0 = finite0 && geom::is_finite(acc[q]);
          if (!finite0) break;
          c = c0 = 0.5 * acc[20];
        }
        // solve
        if (tid == 0) {
          double A[5][5], g[5], x[5], model;
          int q = 0;
#pragma unroll
          for (int i = 0; i < 5; ++i) {
#pragma unroll
            for (int j = i; j < 5; ++j) {
              A[i][j] = acc[q];
              A[j][i] = acc[q++];
            }
            g[i] = acc[15 + i];
          }
          const bool ok = ba_solve<5>(A, g, lm.lam, x, &model);
#pragma unroll
          for (int i = 0; i < 5; ++i) s_x[i] = x[i];
          s_model = model;
          s_ok = ok ? 1 : 0;
        }
        __syncthreads();
        bool ok = s_ok != 0;
        const double model = s_model;
        const double x[5] = {s_x[0], s_x[1], s_x[2], s_x[3], s_x[4]};
        // trial
        double Rn[9], tn[3], cn = 0.0;
        if (ok) {
          rr_rotate(x, R, Rn);
          rr_translate(t, B, x[3], x[4], tn);
          double sum[1] = {0.0};
          int bad = 0;
          for (size_t p = tid; p < n; p += kRrThreads) {
            const double P[3] = {X[p], X[n + p], X[2 * n + p]};
            if (!(P[2] > 0.0)) continue;
            const double b[4] = {bear[p], bear[n + p], bear[2 * n + p], bear[3 * n + p]};
            double Vi[3][3], W[5][3], gx[3], Ap[15], gp[5], sq;
            rr_point(R, t, B, fi, fj, lm.lam, P, b, Vi, W, gx, Ap, gp, &sq);
            double h[3], Pn[3];
#pragma unroll
            for (int i = 0; i < 3; ++i)
              h[i] = gx[i] + ((((W[0][i] * x[0] + W[1][i] * x[1]) + W[2][i] * x[2]) + W[3][i] * x[3]) + W[4][i] * x[4]);
#pragma unroll
            for (int i = 0; i < 3; ++i) {
              Pn[i] = P[i] - ((Vi[i][0] * h[0] + Vi[i][1] * h[1]) + Vi[i][2] * h[2]);
              Xn[i * n + p] = Pn[i];
            }
            double r[4], Z[3], Y[3];
            if (!rr_residual(Rn, tn, fi, fj, Pn, b, r, Z, Y)) bad = 1;
            sum[0] += rr_sq(r);
          }
          rr_block_sums<1>(sum, sh);
          bad = __syncthreads_or(bad);
          cn = 0.5 * sum[0];
          ok = !bad && geom::is_finite(cn) && cn < c && (c - cn) / model > 1e-3;
        }
        if (ok) {
          stop = lm.accepted(c, cn, model);
          c = cn;
          moved = true;
#pragma unroll
          for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
          for (int i = 0; i < 3; ++i) t[i] = tn[i];
          rr_basis(t, B);
          double *sw = X;
          X = Xn;
          Xn = sw;
        } else {
          stop = lm.rejected(c, model);
        }
      }
      status = !moved ? 4u : stop ? 1u : 3u;
      if (!finite0) c = c0 = 0.0;
    }
  }
  if (tid == 0) {
    sfmloc_relrefine_result &o = D.res[k];
    double E[9];
    rr_essential(R, t, E);
    o.status = status;
    o.n_used = n_used;
    o.steps = steps;
    o.reserved = 0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      o.R[i] = R[i];
      o.E[i] = E[i];
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) o.t[i] = t[i];
    o.cost_initial = c0;
    o.cost = c;
  }
}

int relrefine_device(const PairScene &sc, const PairPoses &po, const sfmloc_relrefine_options &opt, hipStream_t s,
                     Relrefine *r) {
  const size_t P = sc.n_pairs, n_inl = (size_t)po.inlier_off[P];
  PairSceneBufs scene;
  PairPosesBufs poses;
  DevBuf<double> d_bear, d_pts, d_trial;
  DevBuf<sfmloc_relrefine_result> d_res;
  SFM_RC(scene.upload(sc, s));
  SFM_RC(poses.upload(sc, po, s));
  SFM_RC(d_bear.alloc(nullptr, 4 * n_inl));
  SFM_RC(d_pts.alloc(nullptr, 3 * n_inl));
  SFM_RC(d_trial.alloc(nullptr, 3 * n_inl));
  SFM_RC(d_res.alloc(nullptr, P));
  SFM_RC(d_res.zero(P, s));
  RrDev D{};
  static_cast<PairDev &>(D) = scene.dev();
  static_cast<PairPosesDev &>(D) = poses.dev();
  D.max_steps = opt.max_steps;
  D.min_points = opt.min_points;
  D.bear = d_bear, D.pts = d_pts, D.trial = d_trial, D.res = d_res;
  SFM_RC(dev_launch(k_relrefine, dim3(sc.n_pairs), dim3(kRrThreads), 0, s, D));
  SFM_RC(d_res.download(r->res.data(), P, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

int relrefine_impl(int device, const PairScene &sc, const PairPoses &po, const sfmloc_relrefine_options &opt, Relrefine *r) {
  std::string err;
  const int rc = relrefine_host::check(sc, po, opt, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  r->res.assign(sc.n_pairs, sfmloc_relrefine_result{});
  return timed_call(device, &g_relrefine_last_ms, sc.n_pairs != 0,
                    [&](hipStream_t s) { return relrefine_device(sc, po, opt, s, r); });
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_relrefine_default_options(sfmloc_relrefine_options *o) {
  if (!o) return;
  o->max_steps = 100;
  o->min_points = 13;
}

int sfmloc_refine_relative_poses(int device, const uint64_t *view_off, uint32_t n_views, const float *kpt_xy,
                                 const uint32_t *view_intrinsic, const double *intrinsics, const uint32_t *intrinsic_type,
                                 uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                                 const uint32_t *match_i, const uint32_t *match_j, const double *rel_R, const double *rel_t,
                                 const uint64_t *inlier_off, const uint32_t *inlier_idx, const uint8_t *use_pair,
                                 const sfmloc_relrefine_options *opt, sfmloc_relrefine **out) {
  const PairScene sc{view_off,     n_views, kpt_xy,  nullptr, view_intrinsic, intrinsics, intrinsic_type,
                     n_intrinsics, pairs,   n_pairs, offsets, match_i,        match_j};
  const PairPoses po{rel_R, rel_t, inlier_off, inlier_idx, use_pair};
  const sfmloc_relrefine_options o = options_or(opt, sfmloc_relrefine_default_options);
  return make_handle<Relrefine>("sfmloc_refine_relative_poses", out,
                                [&](Relrefine *r) { return relrefine_impl(device, sc, po, o, r); });
}

int sfmloc_relrefine_results(const sfmloc_relrefine *rr, sfmloc_relrefine_result *out) {
  SFM_CHECK(rr, SFMLOC_EINVAL, "sfmloc_relrefine_results: null handle");
  const Relrefine *r = reinterpret_cast<const Relrefine *>(rr);
  SFM_CHECK(out || r->res.empty(), SFMLOC_EINVAL, "sfmloc_relrefine_results: null argument");
  if (!r->res.empty()) memcpy(out, r->res.data(), r->res.size() * sizeof(sfmloc_relrefine_result));
  return SFMLOC_OK;
}

void sfmloc_relrefine_destroy(sfmloc_relrefine *r) { delete reinterpret_cast<Relrefine *>(r); }

double sfmloc_relrefine_last_ms(void) { return g_relrefine_last_ms; }

}  // extern "C"
