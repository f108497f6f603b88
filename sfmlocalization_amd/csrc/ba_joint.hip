// The joint commands of OpenMVG_BA -c on a device-resident sfm_data (sfmloc_sfm_adjust_joint): poses, intrinsics and
// structure in one Levenberg-Marquardt loop with one lambda.  The semantics are stated in include/sfmloc.h ("parameters"
// .. "after the call"); the residual, the loss, the rotation step and the lambda rules are ba_device.h's.
//
// Every kernel is a plain launch and every all-to-all seam is a launch boundary; nothing waits inside a kernel for
// another workgroup.  The parameter blocks of the reduced system are the poses [0, n_poses) and then the intrinsics,
// six values each (a part the command does not free has zero Jacobian columns: its step is exactly 0 and it is never
// written).
//
//   linearise   k_jt_lin        one thread per observation stores kLin = 32 doubles (256 B): the weighted residual (2), Jc
//     (once     (2 x 6 over [rotation, translation]), Ji (2 x 6) and Jx (2 x 3); the cost goes through the workgroup's
//     per LM    tree into one partial per workgroup.
//     step)     k_jt_landmark   kBaGroup = 8 lanes per landmark: C_l = Jx^T Jx + lambda D, its inverse by Cholesky, Jx^T r.
//               k_jt_blocks     one wave per pose over its views' lists (ascending view index), and one wave per view for
//               the intrinsics: kBlk = 54 sums (J^T J 21, the block's own Schur term 21, J^T r 6, E C^-1 g_l 6) through
//               the six-level butterfly.
//               k_jt_intr_sum   one workgroup of 256 per intrinsic sums its views' partials: thread-strided in ascending
//               view index, then the workgroup's tree (store, then sum).
//               k_jt_setup      one workgroup of 1024: D, the inverse of every block of the preconditioner, x = 0,
//               r = b, z = M^-1 r, p = z, and the cost from k_jt_lin's partials.
//   PCG         k_jt_pcg_landmark   z_l = C_l^-1 sum Jx^T (Jc p + Ji p), 8 lanes per landmark
//     (one      k_jt_pcg_blocks     q = sum J^T (u - Jx z_l) + lambda D p per pose (wave) with its part of p.q; per view
//     iteration)                    the intrinsic's partial
//               k_jt_pcg_intr       the intrinsics' q from the views' partials (only with i in the command)
//               k_jt_pcg_update     one workgroup of 1024: alpha, x, r, z = M^-1 r, beta, p, and the done flag the three
//                                   kernels above read first (a finished solve makes the rest of its chunk return at once)
//   trial       k_jt_pcg_landmark on x, k_jt_trial (trial copies of R, t, K, X), k_jt_eval (cost and model decrease
//               -(g.d) - |J d|^2 / 2 from one pass, partials per workgroup), k_jt_decide (one workgroup: accept or
//               reject, lambda), k_jt_commit (the trial over the state only when accepted; C = -R^T t).
//
// The host enqueues kPcgChunk iterations at a time and reads the small state record after each chunk and once per LM
// step.  Storing the linearisation (256 B per observation, 256 MB at 1 M observations) is chosen over recomputing it:
// the PCG reads it twice per iteration, tens of times per step.  f64, unfused; no float atomics, every sum is a fixed
// tree, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "ba_device.h"
#include "devmem.h"
#include "sfm_data.h"

namespace sfmloc {
namespace {

constexpr int kLin = 32;       // doubles per observation: r 0..1, Jc 2..13, Ji 14..25, Jx 26..31 (rows of 6, 6, 3)
constexpr int kBlk = 54;       // sums per block: B 0..20, S 21..41, g 42..47, E C^-1 g_l 48..53
constexpr int kPcgChunk = 32;  // PCG iterations enqueued between two looks at the done flag

struct JtState {
  double lam, nu, cost, cost0, cost_new, model, rz, rr0, pcg_tol, ftol;
  uint32_t steps_tried, steps_accepted, pcg_total, pcg_max, pcg_iter, pcg_done, max_pcg, max_steps;
  uint32_t running, stop, take, zero_grad;
};

// the resident arrays (SfmDev: R, C, t, K and X are its pose_R, pose_C, pose_t, intr and lm_X) and this call's workspace
struct JtDev : SfmDev {
  uint32_t n_par, nb_obs, what;
  const uint32_t *intr_view_off, *intr_views;
  const uint8_t *ent, *pose_in, *intr_in, *lm_in;  // an observation enters; a block is free and has one that enters
  double *Rn, *tn, *Kn, *Xn;
  double *lin, *lm_Ci, *lm_Cg, *lm_z, *view_part, *blk, *Minv, *D, *x, *r, *z, *p, *q, *pq_part, *red;
  JtState *st;
};

// the sum over a workgroup of T threads: the wave's butterfly, then the waves' sums in ascending wave index
template <int T>
__device__ __forceinline__ double jt_block_sum(double v, double *sh) {
  v = ba_group_sum<64>(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  double s = sh[0];
#pragma unroll
  for (int i = 1; i < T / 64; ++i) s += sh[i];
  return s;
}

// the inverse of a symmetric positive definite matrix by Cholesky; a pivot that is not positive gives NaNs (the step
// that follows is then not finite and counts as rejected)
template <int N>
__device__ __forceinline__ void jt_inv_spd(const double (&A)[N][N], double (&Ai)[N][N]) {
  double L[N][N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
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
  for (int c = 0; c < N; ++c) {
    double y[N], d[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
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
#pragma unroll
    for (int i = 0; i < N; ++i) Ai[i][c] = d[i];
  }
}

__device__ __forceinline__ double jt_clamp_d(double a) { return fmin(fmax(a, 1e-6), 1e32); }

// ---- linearise -------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_jt_lin(JtDev v) {
  __shared__ double sh[4];
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  double cost = 0.0;
  if (o < v.n_obs && v.ent[o]) {
    const uint32_t vw = v.obs_view[o], l = v.obs_lm[o];
    const uint32_t pi = v.view_pose[vw], ii = v.view_intr[vw];
    const double *R = v.pose_R + 9 * (size_t)pi, *t = v.pose_t + 3 * (size_t)pi, *X = v.lm_X + 3 * (size_t)l;
    double Y[3], Xc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      Y[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2];
      Xc[i] = Y[i] + t[i];
    }
    double r[2], J0[3], J1[3], I0[6], I1[6];
    cost = ba_observation<true>(v.intr + 6 * (size_t)ii, v.intr_type[ii] == 3, Xc, v.obs_x[2 * o], v.obs_x[2 * o + 1], r, J0,
                               J1, I0, I1);
    double *L = v.lin + kLin * o;
    L[0] = r[0];
    L[1] = r[1];
    const bool rot = v.what & SFMLOC_BA_ROTATION, trn = v.what & SFMLOC_BA_TRANSLATION;
    const bool intr = v.what & SFMLOC_BA_INTRINSICS, stru = v.what & SFMLOC_BA_STRUCTURE;
    // d Xc / d w = -[Y]x for R <- exp([w]x) R, d Xc / d t = I
    L[2] = rot ? J0[2] * Y[1] - J0[1] * Y[2] : 0.0;
    L[3] = rot ? J0[0] * Y[2] - J0[2] * Y[0] : 0.0;
    L[4] = rot ? J0[1] * Y[0] - J0[0] * Y[1] : 0.0;
    L[8] = rot ? J1[2] * Y[1] - J1[1] * Y[2] : 0.0;
    L[9] = rot ? J1[0] * Y[2] - J1[2] * Y[0] : 0.0;
    L[10] = rot ? J1[1] * Y[0] - J1[0] * Y[1] : 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      L[5 + k] = trn ? J0[k] : 0.0;
      L[11 + k] = trn ? J1[k] : 0.0;
      // d r / d X = (d r / d Xc) R
      L[26 + k] = stru ? (J0[0] * R[k] + J0[1] * R[3 + k]) + J0[2] * R[6 + k] : 0.0;
      L[29 + k] = stru ? (J1[0] * R[k] + J1[1] * R[3 + k]) + J1[2] * R[6 + k] : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
      L[14 + k] = intr ? I0[k] : 0.0;
      L[20 + k] = intr ? I1[k] : 0.0;
    }
  }
  const double s = jt_block_sum<256>(cost, sh);
  if (threadIdx.x == 0) v.red[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void k_jt_landmark(JtDev v) {
  const uint32_t l = (blockIdx.x * 256 + threadIdx.x) / kBaGroup;
  const int sub = threadIdx.x & (kBaGroup - 1);
  if (l >= v.n_lm || !v.lm_in[l]) return;  // (the whole group leaves: its lanes share l)
  double acc[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (uint64_t o = v.obs_off[l] + sub; o < v.obs_off[l + 1]; o += kBaGroup) {
    if (!v.ent[o]) continue;
    const double *L = v.lin + kLin * o;
    const double *j0 = L + 26, *j1 = L + 29;
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = i; j < 3; ++j) acc[q++] += j0[i] * j0[j] + j1[i] * j1[j];
      acc[6 + i] += j0[i] * L[0] + j1[i] * L[1];
    }
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) acc[k] = ba_group_sum<kBaGroup>(acc[k]);
  const double lam = v.st->lam;
  double A[3][3], Ai[3][3];
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      A[i][j] = acc[q];
      A[j][i] = acc[q++];
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) A[i][i] += lam * jt_clamp_d(A[i][i]);
  jt_inv_spd<3>(A, Ai);
  if (sub == 0) {
    double *ci = v.lm_Ci + 6 * (size_t)l, *cg = v.lm_Cg + 3 * (size_t)l;
    ci[0] = Ai[0][0];
    ci[1] = Ai[0][1];
    ci[2] = Ai[0][2];
    ci[3] = Ai[1][1];
    ci[4] = Ai[1][2];
    ci[5] = Ai[2][2];
#pragma unroll
    for (int i = 0; i < 3; ++i) cg[i] = (Ai[i][0] * acc[6] + Ai[i][1] * acc[7]) + Ai[i][2] * acc[8];
  }
}

// one observation's part of a block's kBlk sums; kOff = 2: the pose's columns, 14: the intrinsic's
template <int kOff>
__device__ __forceinline__ void jt_block_accum(const JtDev &v, uint32_t o, bool stru, double (&acc)[kBlk]) {
  const double *L = v.lin + kLin * (size_t)o;
  const double *j0 = L + kOff, *j1 = L + kOff + 6;
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) acc[q++] += j0[i] * j0[j] + j1[i] * j1[j];
    acc[42 + i] += j0[i] * L[0] + j1[i] * L[1];
  }
  if (!stru) return;
  const uint32_t l = v.obs_lm[o];
  const double *ci = v.lm_Ci + 6 * (size_t)l, *cg = v.lm_Cg + 3 * (size_t)l;
  const double Ci[3][3] = {{ci[0], ci[1], ci[2]}, {ci[1], ci[3], ci[4]}, {ci[2], ci[4], ci[5]}};
  double E[6][3], F[6][3];  // E = J^T Jx, F = E C^-1
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int k = 0; k < 3; ++k) E[i][k] = j0[i] * L[26 + k] + j1[i] * L[29 + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) F[i][k] = (E[i][0] * Ci[0][k] + E[i][1] * Ci[1][k]) + E[i][2] * Ci[2][k];
    acc[48 + i] += (E[i][0] * cg[0] + E[i][1] * cg[1]) + E[i][2] * cg[2];
  }
  q = 21;
#pragma unroll
  for (int i = 0; i < 6; ++i)
#pragma unroll
    for (int j = i; j < 6; ++j) acc[q++] += (F[i][0] * E[j][0] + F[i][1] * E[j][1]) + F[i][2] * E[j][2];
}

// the entering observations of view vw, lane-strided
template <int kOff>
__device__ __forceinline__ void jt_view_accum(const JtDev &v, uint32_t vw, int lane, bool stru, double (&acc)[kBlk]) {
  const uint32_t b0 = v.view_off[vw], nv = v.view_off[vw + 1] - b0;
  for (uint32_t k = lane; k < nv; k += 64) {
    const uint32_t o = v.vlist[b0 + k];
    if (v.ent[o]) jt_block_accum<kOff>(v, o, stru, acc);
  }
}

// waves [0, n_poses): a pose's sums -> blk; waves [n_poses, n_poses + n_views): a view's sums for its intrinsic
__global__ __launch_bounds__(256) void k_jt_blocks(JtDev v) {
  const uint32_t w = (blockIdx.x * 256 + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  const bool stru = v.what & SFMLOC_BA_STRUCTURE;
  double acc[kBlk];
#pragma unroll
  for (int k = 0; k < kBlk; ++k) acc[k] = 0.0;
  double *dst;
  if (w < v.n_poses) {
    for (uint32_t vi = v.pose_view_off[w]; vi < v.pose_view_off[w + 1]; ++vi)
      jt_view_accum<2>(v, v.pose_views[vi], lane, stru, acc);
    dst = v.blk + kBlk * (size_t)w;
  } else if (w < v.n_poses + v.n_views && (v.what & SFMLOC_BA_INTRINSICS)) {
    jt_view_accum<14>(v, w - v.n_poses, lane, stru, acc);
    dst = v.view_part + kBlk * (size_t)(w - v.n_poses);
  } else {
    return;  // (the whole wave leaves)
  }
#pragma unroll
  for (int k = 0; k < kBlk; ++k) acc[k] = ba_group_sum<64>(acc[k]);
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < kBlk; ++k) dst[k] = acc[k];
  }
}

// an intrinsic's NV sums from its views' partials (view_part [n_views * NV]): thread-strided in ascending view index,
// then the workgroup's tree; every thread returns the sums
template <int NV>
__device__ __forceinline__ void jt_intr_sums(const JtDev &v, uint32_t i, double *sh, double (&acc)[NV]) {
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = 0.0;
  for (uint32_t vi = v.intr_view_off[i] + threadIdx.x; vi < v.intr_view_off[i + 1]; vi += 256) {
    const double *src = v.view_part + NV * (size_t)v.intr_views[vi];
#pragma unroll
    for (int k = 0; k < NV; ++k) acc[k] += src[k];
  }
#pragma unroll
  for (int k = 0; k < NV; ++k) acc[k] = jt_block_sum<256>(acc[k], sh);
}

__global__ __launch_bounds__(256) void k_jt_intr_sum(JtDev v) {
  __shared__ double sh[4];
  double acc[kBlk];
  jt_intr_sums<kBlk>(v, blockIdx.x, sh, acc);
  if (threadIdx.x == 0) {
    double *dst = v.blk + kBlk * (size_t)(v.n_poses + blockIdx.x);
#pragma unroll
    for (int k = 0; k < kBlk; ++k) dst[k] = acc[k];
  }
}

// thread-strided sum of a[0..n) by the one workgroup of 1024, then its tree
__device__ __forceinline__ double jt_sum_1024(const double *a, uint32_t n, double *sh) {
  double s = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += 1024) s += a[i];
  return jt_block_sum<1024>(s, sh);
}

__global__ __launch_bounds__(1024) void k_jt_setup(JtDev v) {
  __shared__ double sh[16];
  JtState *st = v.st;
  const double cost = jt_sum_1024(v.red, v.nb_obs, sh);
  const double lam = st->lam;
  const bool stru = v.what & SFMLOC_BA_STRUCTURE;
  double rz = 0.0, rr = 0.0;
  for (uint32_t b = threadIdx.x; b < v.n_par; b += 1024) {
    const double *s = v.blk + kBlk * (size_t)b;
    const bool in = b < v.n_poses ? v.pose_in[b] : v.intr_in[b - v.n_poses];
    double A[6][6], Ai[6][6], r[6];
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) {
        const double a = in ? s[q] : 0.0, sc = (in && stru) ? s[21 + q] : 0.0;
        A[i][j] = a - sc;
        A[j][i] = a - sc;
        if (i == j) {
          const double d = jt_clamp_d(a);
          v.D[6 * (size_t)b + i] = d;
          A[i][i] = (a + lam * d) - sc;
        }
        ++q;
      }
    jt_inv_spd<6>(A, Ai);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      r[i] = in ? (stru ? s[48 + i] - s[42 + i] : -s[42 + i]) : 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) v.Minv[36 * (size_t)b + 6 * i + j] = Ai[i][j];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double z = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) z += Ai[i][j] * r[j];
      v.x[6 * (size_t)b + i] = 0.0;
      v.r[6 * (size_t)b + i] = r[i];
      v.z[6 * (size_t)b + i] = z;
      v.p[6 * (size_t)b + i] = z;
      rz += r[i] * z;
      rr += r[i] * r[i];
    }
  }
  rz = jt_block_sum<1024>(rz, sh);
  rr = jt_block_sum<1024>(rr, sh);
  // the landmarks' own gradient: C^-1 g_l is zero exactly where g_l is (lm_Cg is zero for a landmark that does not enter)
  double gl = 0.0;
  if (stru)
    for (uint32_t i = threadIdx.x; i < 3 * v.n_lm; i += 1024) gl += v.lm_Cg[i] * v.lm_Cg[i];
  gl = jt_block_sum<1024>(gl, sh);
  if (threadIdx.x == 0) {
    st->cost = cost;
    if (st->steps_tried == 0) st->cost0 = cost;
    st->rz = rz;
    st->rr0 = rr;
    st->pcg_iter = 0;
    st->zero_grad = rr == 0.0 && gl == 0.0;  // (rr alone is 0 whenever no pose or intrinsic is free: -c=s)
    st->pcg_done = !(rr > 0.0) || !(rz > 0.0) || st->max_pcg == 0;
  }
}

// ---- PCG -------------------------------------------------------------------------------------------------------------

// u = Jc vec[pose] + Ji vec[intrinsic] of observation o
__device__ __forceinline__ void jt_u(const JtDev &v, const double *L, uint32_t o, const double *vec, double u[2]) {
  const uint32_t vw = v.obs_view[o];
  const double *a = vec + 6 * (size_t)v.view_pose[vw], *b = vec + 6 * (size_t)(v.n_poses + v.view_intr[vw]);
  double u0 = 0.0, u1 = 0.0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    u0 += L[2 + i] * a[i];
    u1 += L[8 + i] * a[i];
  }
  if (v.what & SFMLOC_BA_INTRINSICS) {
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      u0 += L[14 + i] * b[i];
      u1 += L[20 + i] * b[i];
    }
  }
  u[0] = u0;
  u[1] = u1;
}

// z_l = C_l^-1 sum Jx^T (Jc vec + Ji vec); gate: return at once when the solve is done
__global__ __launch_bounds__(256) void k_jt_pcg_landmark(JtDev v, const double *__restrict__ vec, int gate) {
  if (gate && v.st->pcg_done) return;
  const uint32_t l = (blockIdx.x * 256 + threadIdx.x) / kBaGroup;
  const int sub = threadIdx.x & (kBaGroup - 1);
  if (l >= v.n_lm || !v.lm_in[l]) return;
  double acc[3] = {0.0, 0.0, 0.0};
  for (uint64_t o = v.obs_off[l] + sub; o < v.obs_off[l + 1]; o += kBaGroup) {
    if (!v.ent[o]) continue;
    const double *L = v.lin + kLin * o;
    double u[2];
    jt_u(v, L, (uint32_t)o, vec, u);
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] += L[26 + k] * u[0] + L[29 + k] * u[1];
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) acc[k] = ba_group_sum<kBaGroup>(acc[k]);
  if (sub == 0) {
    const double *ci = v.lm_Ci + 6 * (size_t)l;
    double *z = v.lm_z + 3 * (size_t)l;
    z[0] = (ci[0] * acc[0] + ci[1] * acc[1]) + ci[2] * acc[2];
    z[1] = (ci[1] * acc[0] + ci[3] * acc[1]) + ci[4] * acc[2];
    z[2] = (ci[2] * acc[0] + ci[4] * acc[1]) + ci[5] * acc[2];
  }
}

template <int kOff>
__device__ __forceinline__ void jt_view_product(const JtDev &v, uint32_t vw, int lane, bool stru, const double *vec,
                                                double (&acc)[6]) {
  const uint32_t b0 = v.view_off[vw], nv = v.view_off[vw + 1] - b0;
  for (uint32_t k = lane; k < nv; k += 64) {
    const uint32_t o = v.vlist[b0 + k];
    if (!v.ent[o]) continue;
    const double *L = v.lin + kLin * (size_t)o;
    double u[2];
    jt_u(v, L, o, vec, u);
    if (stru) {
      const double *z = v.lm_z + 3 * (size_t)v.obs_lm[o];
      u[0] -= (L[26] * z[0] + L[27] * z[1]) + L[28] * z[2];
      u[1] -= (L[29] * z[0] + L[30] * z[1]) + L[31] * z[2];
    }
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] += L[kOff + i] * u[0] + L[kOff + 6 + i] * u[1];
  }
}

__global__ __launch_bounds__(256) void k_jt_pcg_blocks(JtDev v) {
  if (v.st->pcg_done) return;
  const uint32_t w = (blockIdx.x * 256 + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  const bool stru = v.what & SFMLOC_BA_STRUCTURE;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (w < v.n_poses) {
    for (uint32_t vi = v.pose_view_off[w]; vi < v.pose_view_off[w + 1]; ++vi)
      jt_view_product<2>(v, v.pose_views[vi], lane, stru, v.p, acc);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = ba_group_sum<64>(acc[i]);
    if (lane == 0) {
      const double lam = v.st->lam;
      double pq = 0.0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
        const double pi = v.p[6 * (size_t)w + i];
        const double qi = acc[i] + lam * v.D[6 * (size_t)w + i] * pi;
        v.q[6 * (size_t)w + i] = qi;
        pq += pi * qi;
      }
      v.pq_part[w] = pq;
    }
  } else if (w < v.n_poses + v.n_views && (v.what & SFMLOC_BA_INTRINSICS)) {
    const uint32_t vw = w - v.n_poses;
    jt_view_product<14>(v, vw, lane, stru, v.p, acc);
#pragma unroll
    for (int i = 0; i < 6; ++i) acc[i] = ba_group_sum<64>(acc[i]);
    if (lane == 0) {
#pragma unroll
      for (int i = 0; i < 6; ++i) v.view_part[6 * (size_t)vw + i] = acc[i];
    }
  }
}

// the intrinsics' q (zero, plus the damping, without i in the command: the launch is then skipped and k_jt_setup's p = 0
// there keeps q unread) -- one workgroup per intrinsic
__global__ __launch_bounds__(256) void k_jt_pcg_intr(JtDev v) {
  __shared__ double sh[4];
  if (v.st->pcg_done) return;
  double acc[6];
  jt_intr_sums<6>(v, blockIdx.x, sh, acc);
  if (threadIdx.x == 0) {
    const uint32_t b = v.n_poses + blockIdx.x;
    const double lam = v.st->lam;
    double pq = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const double pi = v.p[6 * (size_t)b + i];
      const double qi = acc[i] + lam * v.D[6 * (size_t)b + i] * pi;
      v.q[6 * (size_t)b + i] = qi;
      pq += pi * qi;
    }
    v.pq_part[b] = pq;
  }
}

__global__ __launch_bounds__(1024) void k_jt_pcg_update(JtDev v, uint32_t n_active) {
  __shared__ double sh[16];
  JtState *st = v.st;
  if (st->pcg_done) return;  // (every thread reads it before thread 0 may write it: the barrier in the sum below)
  const double pq = jt_sum_1024(v.pq_part, n_active, sh);
  const double rz = st->rz;
  const double alpha = rz / pq;
  if (!(pq > 0.0) || !isfinite(alpha)) {  // (not a descent direction of a positive definite system: keep x)
    if (threadIdx.x == 0) st->pcg_done = 1;
    return;
  }
  double rz_n = 0.0, rr = 0.0;
  for (uint32_t b = threadIdx.x; b < n_active; b += 1024) {
    double r[6];
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      const size_t k = 6 * (size_t)b + i;
      v.x[k] += alpha * v.p[k];
      r[i] = v.r[k] - alpha * v.q[k];
      v.r[k] = r[i];
    }
    const double *Mi = v.Minv + 36 * (size_t)b;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
      double z = 0.0;
#pragma unroll
      for (int j = 0; j < 6; ++j) z += Mi[6 * i + j] * r[j];
      v.z[6 * (size_t)b + i] = z;
      rz_n += r[i] * z;
      rr += r[i] * r[i];
    }
  }
  rz_n = jt_block_sum<1024>(rz_n, sh);
  rr = jt_block_sum<1024>(rr, sh);
  const double beta = rz_n / rz;
  for (uint32_t k = threadIdx.x; k < 6 * n_active; k += 1024) v.p[k] = v.z[k] + beta * v.p[k];
  if (threadIdx.x == 0) {
    st->rz = rz_n;
    const uint32_t it = ++st->pcg_iter;
    const double tol = st->pcg_tol;
    if (!(rr > tol * tol * st->rr0) || !(rz_n > 0.0) || it >= st->max_pcg) st->pcg_done = 1;
  }
}

// ---- trial and acceptance ------------------------------------------------------------------------------------------

// the trial point in the scratch copies; lm_z becomes the landmark's step d_l = -C^-1 g_l - C^-1 E^T x
__global__ __launch_bounds__(256) void k_jt_trial(JtDev v) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < v.n_poses) {
    const double *R = v.pose_R + 9 * (size_t)i, *t = v.pose_t + 3 * (size_t)i, *x = v.x + 6 * (size_t)i;
    double *Rn = v.Rn + 9 * (size_t)i, *tn = v.tn + 3 * (size_t)i;
    if (v.pose_in[i] && (v.what & SFMLOC_BA_ROTATION)) {
      const double w[3] = {x[0], x[1], x[2]};
      double Ro[9], Rt[9];
#pragma unroll
      for (int k = 0; k < 9; ++k) Ro[k] = R[k];
      ba_rotate(w, Ro, Rt);
#pragma unroll
      for (int k = 0; k < 9; ++k) Rn[k] = Rt[k];
    } else {
#pragma unroll
      for (int k = 0; k < 9; ++k) Rn[k] = R[k];
    }
    const bool trn = v.pose_in[i] && (v.what & SFMLOC_BA_TRANSLATION);
#pragma unroll
    for (int k = 0; k < 3; ++k) tn[k] = trn ? t[k] + x[3 + k] : t[k];
  }
  if (i < v.n_intr) {
    const double *K = v.intr + 6 * (size_t)i, *x = v.x + 6 * (size_t)(v.n_poses + i);
    double *Kn = v.Kn + 6 * (size_t)i;
    const int nf = (v.intr_in[i] && (v.what & SFMLOC_BA_INTRINSICS)) ? (v.intr_type[i] == 3 ? 6 : 3) : 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) Kn[k] = k < nf ? K[k] + x[k] : K[k];
  }
  if (i < v.n_lm) {
    const double *X = v.lm_X + 3 * (size_t)i;
    double *Xn = v.Xn + 3 * (size_t)i;
    if (v.lm_in[i]) {
      double *z = v.lm_z + 3 * (size_t)i;
      const double *cg = v.lm_Cg + 3 * (size_t)i;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const double d = -cg[k] - z[k];
        z[k] = d;
        Xn[k] = X[k] + d;
      }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) Xn[k] = X[k];
    }
  }
}

// per observation: the cost at the trial point, and its part of the model decrease -(r . J d) - |J d|^2 / 2
__global__ __launch_bounds__(256) void k_jt_eval(JtDev v) {
  __shared__ double sh[4];
  const uint64_t o = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  double cost = 0.0, model = 0.0;
  if (o < v.n_obs && v.ent[o]) {
    const uint32_t vw = v.obs_view[o], l = v.obs_lm[o];
    const uint32_t pi = v.view_pose[vw], ii = v.view_intr[vw];
    const double *R = v.Rn + 9 * (size_t)pi, *t = v.tn + 3 * (size_t)pi, *X = v.Xn + 3 * (size_t)l;
    double Xc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Xc[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i];
    double r[2], J0[3], J1[3], I0[6], I1[6];  // (the function k_jt_lin costs the state with: one rounding for both)
    cost = ba_observation<true>(v.Kn + 6 * (size_t)ii, v.intr_type[ii] == 3, Xc, v.obs_x[2 * o], v.obs_x[2 * o + 1], r, J0,
                               J1, I0, I1);
    const double *L = v.lin + kLin * o;
    double u[2];
    jt_u(v, L, (uint32_t)o, v.x, u);
    if ((v.what & SFMLOC_BA_STRUCTURE) && v.lm_in[l]) {
      const double *d = v.lm_z + 3 * (size_t)l;
      u[0] += (L[26] * d[0] + L[27] * d[1]) + L[28] * d[2];
      u[1] += (L[29] * d[0] + L[30] * d[1]) + L[31] * d[2];
    }
    model = -(L[0] * u[0] + L[1] * u[1]) - 0.5 * (u[0] * u[0] + u[1] * u[1]);
  }
  const double c = jt_block_sum<256>(cost, sh);
  const double m = jt_block_sum<256>(model, sh);
  if (threadIdx.x == 0) {
    v.red[blockIdx.x] = c;
    v.red[v.nb_obs + blockIdx.x] = m;
  }
}

__global__ __launch_bounds__(1024) void k_jt_decide(JtDev v) {
  __shared__ double sh[16];
  const double cn = jt_sum_1024(v.red, v.nb_obs, sh);
  const double model = jt_sum_1024(v.red + v.nb_obs, v.nb_obs, sh);
  if (threadIdx.x != 0) return;
  JtState *st = v.st;
  const double c = st->cost;
  st->cost_new = cn;
  st->model = model;
  ++st->steps_tried;
  st->pcg_total += st->pcg_iter;
  if (st->pcg_iter > st->pcg_max) st->pcg_max = st->pcg_iter;
  const bool ok = isfinite(cn) && isfinite(model) && model > 0.0 && cn < c && (c - cn) / model > 1e-3;
  st->take = ok;
  if (st->zero_grad) {  // (nothing to do at a stationary point)
    st->take = 0;
    st->stop = 0;
    st->running = 0;
    return;
  }
  if (ok) {
    ++st->steps_accepted;
    const double q = (c - cn) / model;
    const double e = 2.0 * q - 1.0;
    st->lam = fmax(st->lam * fmax(1.0 / 3.0, 1.0 - e * e * e), 1e-32);
    st->nu = 2.0;
    st->cost = cn;
    if ((c - cn) <= st->ftol * c) {
      st->stop = 0;
      st->running = 0;
    }
  } else {
    if (isfinite(model) && model > 0.0 && model <= st->ftol * c) {  // the model itself promises less than the tolerance
      st->stop = 0;
      st->running = 0;
    }
    st->lam *= st->nu;
    st->nu *= 2.0;
    if (st->running && !(st->lam < 1e32)) {
      st->stop = 2;
      st->running = 0;
    }
  }
  if (st->running && st->steps_tried >= st->max_steps) {
    st->stop = 1;
    st->running = 0;
  }
}

// the trial over the state, only when k_jt_decide took it; C = -R^T t for the poses that moved
__global__ __launch_bounds__(256) void k_jt_commit(JtDev v) {
  if (!v.st->take) return;
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < v.n_poses && v.pose_in[i]) {
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = v.Rn[9 * (size_t)i + k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = v.tn[3 * (size_t)i + k];
    if (v.what & SFMLOC_BA_ROTATION) {
#pragma unroll
      for (int k = 0; k < 9; ++k) v.pose_R[9 * (size_t)i + k] = R[k];
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      v.pose_t[3 * (size_t)i + k] = t[k];
      v.pose_C[3 * (size_t)i + k] = -((R[k] * t[0] + R[3 + k] * t[1]) + R[6 + k] * t[2]);
    }
  }
  if (i < v.n_intr && v.intr_in[i]) {
#pragma unroll
    for (int k = 0; k < 6; ++k) v.intr[6 * (size_t)i + k] = v.Kn[6 * (size_t)i + k];
  }
  if (i < v.n_lm && v.lm_in[i]) {
#pragma unroll
    for (int k = 0; k < 3; ++k) v.lm_X[3 * (size_t)i + k] = v.Xn[3 * (size_t)i + k];
  }
}

// sfmloc_sfm_adjust_joint's body
int ba_joint_run(Sfm &s, uint32_t what, const sfmloc_ba_joint_options &opt, sfmloc_ba_joint_report *rep) {
  const int rc_pose = sfm_check_poses(s, "adjusted");  // (fetches the keep masks of the last cleanup)
  if (rc_pose) return rc_pose;
  // the host decides which observations enter: its copies of the index arrays and of the keep masks
  const uint8_t *obs_keep = s.cleaned ? s.h_obs_keep.data() : nullptr;
  const uint8_t *lm_stage = s.cleaned ? s.h_lm_stage.data() : nullptr;
  sfmloc_ba_joint_report out{};
  const bool pose = what & (SFMLOC_BA_ROTATION | SFMLOC_BA_TRANSLATION), intr = what & SFMLOC_BA_INTRINSICS;
  const bool stru = what & SFMLOC_BA_STRUCTURE;
  // which observations enter and which blocks they refer to (sfmloc.h "entering"), on the host once per call
  std::vector<uint8_t> ent(s.n_obs, 0), pose_in(s.n_poses, 0), intr_in(s.n_intr, 0), lm_in(s.n_lm, 0);
  uint64_t n_ent = 0;
  for (uint32_t l = 0; l < s.n_lm; ++l) {
    if (lm_stage && lm_stage[l] != 3) continue;
    for (uint64_t o = s.h_obs_off[l]; o < s.h_obs_off[l + 1]; ++o) {
      if (obs_keep && !obs_keep[o]) continue;
      const uint32_t vw = s.h_obs_view[o];
      ent[o] = 1;
      ++n_ent;
      if (pose) pose_in[s.h_view_pose[vw]] = 1;
      if (intr) intr_in[s.h_view_intr[vw]] = 1;
      if (stru) lm_in[l] = 1;
    }
  }
  for (uint8_t b : pose_in) out.n_pose_blocks += b;
  for (uint8_t b : intr_in) out.n_intrinsic_blocks += b;
  for (uint8_t b : lm_in) out.n_landmark_blocks += b;
  if (n_ent == 0) {
    if (rep) *rep = out;
    return SFMLOC_OK;  // (nothing moved: the host's copies of the poses and intrinsics hold)
  }
  std::vector<uint32_t> iv_off((size_t)s.n_intr + 1, 0), iv(s.n_views);
  for (uint32_t vw = 0; vw < s.n_views; ++vw) ++iv_off[s.h_view_intr[vw] + 1];
  for (uint32_t i = 0; i < s.n_intr; ++i) iv_off[i + 1] += iv_off[i];
  {
    std::vector<uint32_t> at(iv_off.begin(), iv_off.end() - 1);
    for (uint32_t vw = 0; vw < s.n_views; ++vw) iv[at[s.h_view_intr[vw]]++] = vw;  // (ascending view index)
  }

  const uint32_t n_par = s.n_poses + s.n_intr;
  const uint32_t nb_obs = (uint32_t)((s.n_obs + 255) / 256);
  hipStream_t st = s.s;
  // the workspace, before the loop
  DevBuf<uint8_t> d_ent, d_pose_in, d_intr_in, d_lm_in;
  DevBuf<uint32_t> d_iv_off, d_iv;
  DevBuf<double> d_Rn, d_tn, d_Kn, d_Xn, d_lin, d_lm_Ci, d_lm_Cg, d_lm_z, d_view_part, d_blk, d_Minv, d_D, d_x, d_r, d_z,
      d_p, d_q, d_pq, d_red;
  DevBuf<JtState> d_st;
  int rc = SFMLOC_OK;
#define JT_TRY(x)      \
  do {                 \
    rc = (x);          \
    if (rc) return rc; \
  } while (0)
  JT_TRY(dev_upload(nullptr, d_ent, ent.data(), ent.size(), st, 1));
  JT_TRY(dev_upload(nullptr, d_pose_in, pose_in.data(), pose_in.size(), st, 1));
  JT_TRY(dev_upload(nullptr, d_intr_in, intr_in.data(), intr_in.size(), st, 1));
  JT_TRY(dev_upload(nullptr, d_lm_in, lm_in.data(), lm_in.size(), st, 1));
  JT_TRY(dev_upload(nullptr, d_iv_off, iv_off.data(), iv_off.size(), st, 1));
  JT_TRY(dev_upload(nullptr, d_iv, iv.data(), iv.size(), st, 1));
  JT_TRY(d_Rn.alloc(nullptr, 9 * (size_t)s.n_poses));
  JT_TRY(d_tn.alloc(nullptr, 3 * (size_t)s.n_poses));
  JT_TRY(d_Kn.alloc(nullptr, 6 * (size_t)s.n_intr));
  JT_TRY(d_Xn.alloc(nullptr, 3 * (size_t)s.n_lm + 1));
  JT_TRY(d_lin.alloc(nullptr, kLin * (size_t)s.n_obs));
  JT_TRY(d_lm_Ci.alloc(nullptr, 6 * (size_t)s.n_lm + 1));
  JT_TRY(d_lm_Cg.alloc(nullptr, 3 * (size_t)s.n_lm + 1));
  JT_TRY(d_lm_z.alloc(nullptr, 3 * (size_t)s.n_lm + 1));
  JT_TRY(d_view_part.alloc(nullptr, kBlk * (size_t)s.n_views));
  JT_TRY(d_blk.alloc(nullptr, kBlk * (size_t)n_par));
  JT_TRY(d_Minv.alloc(nullptr, 36 * (size_t)n_par));
  JT_TRY(d_D.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_x.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_r.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_z.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_p.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_q.alloc(nullptr, 6 * (size_t)n_par));
  JT_TRY(d_pq.alloc(nullptr, n_par));
  JT_TRY(d_red.alloc(nullptr, 2 * (size_t)nb_obs));
  JT_TRY(d_st.alloc(nullptr, 1));
#undef JT_TRY
  JtState h{};
  h.lam = 1e-4;
  h.nu = 2.0;
  h.pcg_tol = opt.pcg_tolerance;
  h.ftol = opt.function_tolerance;
  h.max_pcg = opt.max_pcg;
  h.max_steps = opt.max_steps;
  h.running = 1;
  h.stop = 1;
  SFM_RC(d_st.upload(&h, 1, st));
  // (without i the intrinsics' blocks stay out of the vectors the update pass walks: their p, q are never written)
  const uint32_t n_active = intr ? n_par : s.n_poses;
  SFM_RC(d_blk.zero(kBlk * (size_t)n_par, st));
  SFM_RC(dev_zero(d_x.get(), 6 * (size_t)n_par, st));
  SFM_RC(d_p.zero(6 * (size_t)n_par, st));
  SFM_RC(d_lm_Cg.zero(3 * (size_t)s.n_lm + 1, st));

  JtDev v{};
  static_cast<SfmDev &>(v) = sfm_dev(s);
  v.n_par = n_par;
  v.nb_obs = nb_obs;
  v.what = what;
  v.intr_view_off = d_iv_off;
  v.intr_views = d_iv;
  v.ent = d_ent;
  v.pose_in = d_pose_in;
  v.intr_in = d_intr_in;
  v.lm_in = d_lm_in;
  v.Rn = d_Rn;
  v.tn = d_tn;
  v.Kn = d_Kn;
  v.Xn = d_Xn;
  v.lin = d_lin;
  v.lm_Ci = d_lm_Ci;
  v.lm_Cg = d_lm_Cg;
  v.lm_z = d_lm_z;
  v.view_part = d_view_part;
  v.blk = d_blk;
  v.Minv = d_Minv;
  v.D = d_D;
  v.x = d_x;
  v.r = d_r;
  v.z = d_z;
  v.p = d_p;
  v.q = d_q;
  v.pq_part = d_pq;
  v.red = d_red;
  v.st = d_st;

  const dim3 b256(256), g_obs(nb_obs), g_lm((s.n_lm + 256 / kBaGroup - 1) / (256 / kBaGroup) + 0);
  const dim3 g_blocks(((intr ? s.n_poses + s.n_views : s.n_poses) + 3) / 4), g_intr(s.n_intr);
  const dim3 g_each((std::max(std::max(s.n_poses, s.n_intr), s.n_lm) + 255) / 256);
  rc = ba_pose_t(v, st);
  if (rc) return rc;
  auto read_state = [&]() -> int {
    SFM_RC(d_st.download(&h, 1, st));
    SFM_HIP(hipStreamSynchronize(st));
    return SFMLOC_OK;
  };
  while (h.running) {
    SFM_RC(dev_launch(k_jt_lin, g_obs, b256, 0, st, v));
    if (stru) SFM_RC(dev_launch(k_jt_landmark, g_lm, b256, 0, st, v));
    SFM_RC(dev_launch(k_jt_blocks, g_blocks, b256, 0, st, v));
    if (intr) SFM_RC(dev_launch(k_jt_intr_sum, g_intr, b256, 0, st, v));
    SFM_RC(dev_launch(k_jt_setup, dim3(1), dim3(1024), 0, st, v));
    for (uint32_t it = 0; it < opt.max_pcg; it += kPcgChunk) {
      for (int k = 0; k < kPcgChunk; ++k) {
        if (stru) SFM_RC(dev_launch(k_jt_pcg_landmark, g_lm, b256, 0, st, v, d_p, 1));
        SFM_RC(dev_launch(k_jt_pcg_blocks, g_blocks, b256, 0, st, v));
        if (intr) SFM_RC(dev_launch(k_jt_pcg_intr, g_intr, b256, 0, st, v));
        SFM_RC(dev_launch(k_jt_pcg_update, dim3(1), dim3(1024), 0, st, v, n_active));
      }
      rc = read_state();
      if (rc) return rc;
      if (h.pcg_done) break;
    }
    if (stru) SFM_RC(dev_launch(k_jt_pcg_landmark, g_lm, b256, 0, st, v, d_x, 0));
    SFM_RC(dev_launch(k_jt_trial, g_each, b256, 0, st, v));
    SFM_RC(dev_launch(k_jt_eval, g_obs, b256, 0, st, v));
    SFM_RC(dev_launch(k_jt_decide, dim3(1), dim3(1024), 0, st, v));
    SFM_RC(dev_launch(k_jt_commit, g_each, b256, 0, st, v));
    rc = read_state();
    if (rc) return rc;
  }
  out.cost_initial = h.cost0;
  out.cost_final = h.cost;
  out.steps_tried = h.steps_tried;
  out.steps_accepted = h.steps_accepted;
  out.pcg_total = h.pcg_total;
  out.pcg_max = h.pcg_max;
  out.stop = h.stop;
  if (rep) *rep = out;
  if (what & SFMLOC_BA_INTRINSICS)
    SFM_RC(dev_download(s.h_intr.data(), v.intr, 6 * (size_t)s.n_intr, st));
  return sfm_fetch_poses(s);
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_ba_joint_default_options(sfmloc_ba_joint_options *o) {
  if (!o) return;
  o->max_steps = 50;            // Ceres max_num_iterations
  o->max_pcg = 500;             // Ceres max_linear_solver_iterations
  o->function_tolerance = 1e-6;
  o->pcg_tolerance = 0.1;       // Ceres eta
}

int sfmloc_sfm_adjust_joint(sfmloc_sfm *hh, uint32_t what, const sfmloc_ba_joint_options *opt,
                            sfmloc_ba_joint_report *rep) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_adjust_joint: null handle");
  const uint32_t all = SFMLOC_BA_ROTATION | SFMLOC_BA_TRANSLATION | SFMLOC_BA_INTRINSICS | SFMLOC_BA_STRUCTURE;
  SFM_CHECK(what != 0 && (what & ~all) == 0, SFMLOC_EINVAL,
            "sfmloc_sfm_adjust_joint: what = %u: a non-zero combination of the four SFMLOC_BA_ bits (-c's r, t, i, s)",
            what);
  sfmloc_ba_joint_options o;
  if (opt) o = *opt;
  else sfmloc_ba_joint_default_options(&o);
  SFM_CHECK(o.max_steps > 0 && o.function_tolerance >= 0.0 && o.pcg_tolerance >= 0.0, SFMLOC_EINVAL,
            "sfmloc_sfm_adjust_joint: max_steps must be positive and the tolerances not negative");
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  if (rep) memset(rep, 0, sizeof *rep);
  SFM_HIP(hipSetDevice(h->device));
  try {
    return ba_joint_run(*h, what, o, rep);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_adjust_joint: out of host memory");
    return SFMLOC_ENOMEM;
  }
}

}  // extern "C"
