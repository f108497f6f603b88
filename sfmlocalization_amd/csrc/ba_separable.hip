// The separable commands of OpenMVG_BA -c on a device-resident sfm_data (sfmloc_sfm_adjust): structure alone, or the
// poses alone.  The semantics are stated in include/sfmloc.h ("blocks" .. "order"); every block -- a landmark's X, or a
// pose's rotation / translation / both -- is a Levenberg-Marquardt problem of its own and all of its iterations run
// inside one launch.
//
//   k_ba_structure   kBaGroup = 8 lanes per landmark (eight landmarks per wave) stride over the landmark's CSR range;
//                    the 3x3 normal matrix (6 values), the gradient (3) and the cost (1) go through a three-level
//                    in-wave butterfly, after which every lane of the group holds the same bits and solves the same
//                    damped system by Cholesky.
//   k_ba_motion      one wave per pose strides over the view-sorted lists of the pose's views (ascending view index) and
//                    gathers the landmarks; 21 + 6 + 1 doubles go through a six-level butterfly; 6x6 Cholesky for rt,
//                    3x3 for r or t.  The rotation steps in the tangent space at the current R.
//
// f64, unfused (the library's -ffp-contract=off).  No LDS, no atomics: a block's sums depend on its own observations'
// order only, so two runs give the same bits.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <new>
#include <vector>

#include "ba_device.h"
#include "sfm_data.h"

namespace sfmloc {
namespace {

constexpr uint32_t kInfoEntered = 1u << 29, kInfoMoved = 1u << 30, kInfoCap = 1u << 31;

// t = -R C of every pose (sfmloc.h "blocks"), before either adjustment (ba_pose_t)
__global__ __launch_bounds__(256) void k_ba_pose_t(uint32_t n_poses, const double *__restrict__ R,
                                                   const double *__restrict__ C, double *__restrict__ t) {
  const uint32_t p = blockIdx.x * 256 + threadIdx.x;
  if (p >= n_poses) return;
  const double *r = R + 9 * (size_t)p, *c = C + 3 * (size_t)p;
#pragma unroll
  for (int i = 0; i < 3; ++i) t[3 * (size_t)p + i] = -((r[3 * i] * c[0] + r[3 * i + 1] * c[1]) + r[3 * i + 2] * c[2]);
}

// ---- structure -----------------------------------------------------------------------------------------------------

// the group's sums at X over the landmark's entering observations [a, b): A (3 x 3), g (3), cost; *n = how many entered
__device__ __forceinline__ void ba_structure_eval(const SfmDev &v, uint64_t a, uint64_t b, int sub, const double X[3],
                                                  double (&A)[3][3], double (&g)[3], double *cost, uint32_t *n) {
  double acc[10] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  uint32_t cnt = 0;
  for (uint64_t o = a + sub; o < b; o += kBaGroup) {
    if (v.obs_keep && !v.obs_keep[o]) continue;
    const uint32_t vw = v.obs_view[o];
    const uint32_t pi = v.view_pose[vw], ii = v.view_intr[vw];
    const double *R = v.pose_R + 9 * (size_t)pi, *t = v.pose_t + 3 * (size_t)pi;
    double Xc[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) Xc[i] = ((R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2]) + t[i];
    double r[2], J0[3], J1[3];
    acc[9] += ba_observation<false>(v.intr + 6 * (size_t)ii, v.intr_type[ii] == 3, Xc, v.obs_x[2 * o], v.obs_x[2 * o + 1], r, J0,
                             J1);
    double j0[3], j1[3];  // d r / d X = (d r / d Xc) R
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      j0[k] = (J0[0] * R[k] + J0[1] * R[3 + k]) + J0[2] * R[6 + k];
      j1[k] = (J1[0] * R[k] + J1[1] * R[3 + k]) + J1[2] * R[6 + k];
    }
    int q = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = i; j < 3; ++j) acc[q++] += j0[i] * j0[j] + j1[i] * j1[j];
      acc[6 + i] += j0[i] * r[0] + j1[i] * r[1];
    }
    ++cnt;
  }
#pragma unroll
  for (int k = 0; k < 10; ++k) acc[k] = ba_group_sum<kBaGroup>(acc[k]);
  if (n) {
#pragma unroll
    for (int m = kBaGroup / 2; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    *n = cnt;
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = i; j < 3; ++j) {
      A[i][j] = acc[q];
      A[j][i] = acc[q++];
    }
    g[i] = acc[6 + i];
  }
  *cost = acc[9];
}

__global__ __launch_bounds__(256) void k_ba_structure(SfmDev v) {
  const uint32_t l = (blockIdx.x * 256 + threadIdx.x) / kBaGroup;
  const int sub = threadIdx.x & (kBaGroup - 1);
  if (l >= v.n_lm) return;  // (the whole group leaves: its lanes share l)
  uint32_t info = 0;
  double c0 = 0.0, c = 0.0;
  if (!v.lm_stage || v.lm_stage[l] == 3) {
    const uint64_t a = v.obs_off[l], b = v.obs_off[l + 1];
    double X[3] = {v.lm_X[3 * (size_t)l], v.lm_X[3 * (size_t)l + 1], v.lm_X[3 * (size_t)l + 2]};
    double A[3][3], g[3];
    uint32_t n = 0;
    ba_structure_eval(v, a, b, sub, X, A, g, &c, &n);
    c0 = c;
    if (n) {
      info = kInfoEntered;
      BaLm lm;
      uint32_t steps = 0;
      bool stop = false, moved = false;
      while (!stop && steps < (uint32_t)kBaMaxSteps) {
        ++steps;
        double d[3], model;
        bool ok = ba_solve<3>(A, g, lm.lam, d, &model);
        double Xn[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
        double An[3][3], gn[3], cn = 0.0;
        if (ok) {
          ba_structure_eval(v, a, b, sub, Xn, An, gn, &cn, nullptr);
          ok = isfinite(cn) && cn < c && (c - cn) / model > 1e-3;
#pragma unroll
          for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) ok = ok && isfinite(An[i][j]);
        }
        if (ok) {
          stop = lm.accepted(c, cn, model);
          c = cn;
          moved = true;
#pragma unroll
          for (int i = 0; i < 3; ++i) {
            X[i] = Xn[i];
            g[i] = gn[i];
#pragma unroll
            for (int j = 0; j < 3; ++j) A[i][j] = An[i][j];
          }
        } else {
          stop = lm.rejected(c, model);
        }
      }
      info |= steps | (moved ? kInfoMoved : 0u) | (stop ? 0u : kInfoCap);
      if (moved && sub == 0) {
        v.lm_X[3 * (size_t)l] = X[0];
        v.lm_X[3 * (size_t)l + 1] = X[1];
        v.lm_X[3 * (size_t)l + 2] = X[2];
      }
    }
  }
  if (sub == 0) {
    v.blk_cost[2 * (size_t)l] = c0;
    v.blk_cost[2 * (size_t)l + 1] = c;
    v.blk_info[l] = info;
  }
}

// ---- motion ----------------------------------------------------------------------------------------------------------

// the wave's sums at (R, t) over the entering observations of pose p: A (6 x 6 over [rotation, translation]), g, cost
__device__ __forceinline__ void ba_motion_eval(const SfmDev &v, uint32_t p, int lane, const double R[9], const double t[3],
                                               double (&A)[6][6], double (&g)[6], double *cost, uint32_t *n) {
  double acc[28];
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  uint32_t cnt = 0;
  for (uint32_t vi = v.pose_view_off[p]; vi < v.pose_view_off[p + 1]; ++vi) {
    const uint32_t vw = v.pose_views[vi];
    const uint32_t ii = v.view_intr[vw];
    const double *K = v.intr + 6 * (size_t)ii;
    const bool radial = v.intr_type[ii] == 3;
    const uint32_t b0 = v.view_off[vw], nv = v.view_off[vw + 1] - b0;
    for (uint32_t k = lane; k < nv; k += 64) {
      const uint32_t o = v.vlist[b0 + k], l = v.obs_lm[o];
      if (v.obs_keep && (!v.obs_keep[o] || v.lm_stage[l] != 3)) continue;
      const double *X = v.lm_X + 3 * (size_t)l;
      double Y[3], Xc[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        Y[i] = (R[3 * i] * X[0] + R[3 * i + 1] * X[1]) + R[3 * i + 2] * X[2];
        Xc[i] = Y[i] + t[i];
      }
      double r[2], J0[3], J1[3];
      acc[27] += ba_observation<false>(K, radial, Xc, v.obs_x[2 * (size_t)o], v.obs_x[2 * (size_t)o + 1], r, J0, J1);
      // d Xc / d w = -[Y]x for R <- exp([w]x) R, d Xc / d t = I
      const double j0[6] = {J0[2] * Y[1] - J0[1] * Y[2], J0[0] * Y[2] - J0[2] * Y[0], J0[1] * Y[0] - J0[0] * Y[1],
                            J0[0],                       J0[1],                       J0[2]};
      const double j1[6] = {J1[2] * Y[1] - J1[1] * Y[2], J1[0] * Y[2] - J1[2] * Y[0], J1[1] * Y[0] - J1[0] * Y[1],
                            J1[0],                       J1[1],                       J1[2]};
      int q = 0;
#pragma unroll
      for (int i = 0; i < 6; ++i) {
#pragma unroll
        for (int j = i; j < 6; ++j) acc[q++] += j0[i] * j0[j] + j1[i] * j1[j];
        acc[21 + i] += j0[i] * r[0] + j1[i] * r[1];
      }
      ++cnt;
    }
  }
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = ba_group_sum<64>(acc[k]);
  if (n) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cnt += __shfl_xor(cnt, m, 64);
    *n = cnt;
  }
  int q = 0;
#pragma unroll
  for (int i = 0; i < 6; ++i) {
#pragma unroll
    for (int j = i; j < 6; ++j) {
      A[i][j] = acc[q];
      A[j][i] = acc[q++];
    }
    g[i] = acc[21 + i];
  }
  *cost = acc[27];
}

// N free parameters starting at row kOff of [rotation (3), translation (3)]: (3, 0) = r, (3, 3) = t, (6, 0) = rt
template <int N, int kOff>
__global__ __launch_bounds__(256) void k_ba_motion(SfmDev v) {
  const uint32_t p = (blockIdx.x * 256 + threadIdx.x) / 64;
  const int lane = threadIdx.x & 63;
  if (p >= v.n_poses) return;  // (the whole wave leaves)
  constexpr bool kRot = kOff == 0, kTrn = (N + kOff) == 6;
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = v.pose_R[9 * (size_t)p + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = v.pose_t[3 * (size_t)p + i];
  double A6[6][6], g6[6], c = 0.0;
  uint32_t n = 0, info = 0;
  ba_motion_eval(v, p, lane, R, t, A6, g6, &c, &n);
  const double c0 = c;
  if (n) {
    info = kInfoEntered;
    BaLm lm;
    uint32_t steps = 0;
    bool stop = false, moved = false;
    while (!stop && steps < (uint32_t)kBaMaxSteps) {
      ++steps;
      double A[N][N], g[N], d[N], model;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        g[i] = g6[kOff + i];
#pragma unroll
        for (int j = 0; j < N; ++j) A[i][j] = A6[kOff + i][kOff + j];
      }
      bool ok = ba_solve<N>(A, g, lm.lam, d, &model);
      double Rn[9], tn[3], An[6][6], gn[6], cn = 0.0;
      if (ok) {
        if (kRot) {
          const double w[3] = {d[0], d[1], d[2]};
          ba_rotate(w, R, Rn);
        } else {
#pragma unroll
          for (int i = 0; i < 9; ++i) Rn[i] = R[i];
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) tn[i] = kTrn ? t[i] + d[N - 3 + i] : t[i];
        ba_motion_eval(v, p, lane, Rn, tn, An, gn, &cn, nullptr);
        ok = isfinite(cn) && cn < c && (c - cn) / model > 1e-3;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = 0; j < 6; ++j) ok = ok && isfinite(An[i][j]);
      }
      if (ok) {
        stop = lm.accepted(c, cn, model);
        c = cn;
        moved = true;
#pragma unroll
        for (int i = 0; i < 9; ++i) R[i] = Rn[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) t[i] = tn[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          g6[i] = gn[i];
#pragma unroll
          for (int j = 0; j < 6; ++j) A6[i][j] = An[i][j];
        }
      } else {
        stop = lm.rejected(c, model);
      }
    }
    info |= steps | (moved ? kInfoMoved : 0u) | (stop ? 0u : kInfoCap);
    if (moved && lane == 0) {
      if (kRot) {
#pragma unroll
        for (int i = 0; i < 9; ++i) v.pose_R[9 * (size_t)p + i] = R[i];
      }
#pragma unroll
      for (int i = 0; i < 3; ++i)  // C = -R^T t
        v.pose_C[3 * (size_t)p + i] = -((R[i] * t[0] + R[3 + i] * t[1]) + R[6 + i] * t[2]);
    }
  }
  if (lane == 0) {
    v.blk_cost[2 * (size_t)p] = c0;
    v.blk_cost[2 * (size_t)p + 1] = c;
    v.blk_info[p] = info;
  }
}

// sfmloc_sfm_adjust's body: the blocks of `what` on the handle's stream, then the report from the blocks' records
int ba_separable_run(Sfm &h, uint32_t what, sfmloc_ba_report *rep) {
  const int rc = sfm_check_poses(h, "adjusted");
  if (rc) return rc;
  const SfmDev v = sfm_dev(h);
  const bool structure = what == SFMLOC_BA_STRUCTURE;
  const uint32_t nb = structure ? h.n_lm : h.n_poses;
  sfmloc_ba_report r{};
  if (nb) {
    const int rc_t = ba_pose_t(v, h.s);
    if (rc_t) return rc_t;
    if (structure) {
      const uint32_t per = 256 / kBaGroup;
      SFM_RC(dev_launch(k_ba_structure, dim3((nb + per - 1) / per), dim3(256), 0, h.s, v));
    } else {
      const dim3 grid((nb + 3) / 4);
      if (what == SFMLOC_BA_ROTATION) SFM_RC(dev_launch(k_ba_motion<3, 0>, grid, dim3(256), 0, h.s, v));
      else if (what == SFMLOC_BA_TRANSLATION) SFM_RC(dev_launch(k_ba_motion<3, 3>, grid, dim3(256), 0, h.s, v));
      else SFM_RC(dev_launch(k_ba_motion<6, 0>, grid, dim3(256), 0, h.s, v));
    }
    std::vector<double> cost(2 * (size_t)nb);
    std::vector<uint32_t> info(nb);
    SFM_RC(dev_download(cost.data(), v.blk_cost, cost.size(), h.s));
    SFM_RC(dev_download(info.data(), v.blk_info, info.size(), h.s));
    SFM_HIP(hipStreamSynchronize(h.s));
    for (uint32_t b = 0; b < nb; ++b) {  // (ascending block index: the totals' order is fixed)
      if (!(info[b] & kInfoEntered)) continue;
      ++r.n_blocks;
      r.cost_initial += cost[2 * (size_t)b];
      r.cost_final += cost[2 * (size_t)b + 1];
      r.n_at_cap += (info[b] & kInfoCap) != 0;
      r.n_unchanged += (info[b] & kInfoMoved) == 0;
      const uint32_t steps = info[b] & 0xFFFFu;
      if (steps > r.max_iterations) r.max_iterations = steps;
    }
  }
  if (rep) *rep = r;
  if (!structure) return sfm_fetch_poses(h);
  return SFMLOC_OK;
}

}  // namespace

int ba_pose_t(const SfmDev &v, hipStream_t s) {
  return dev_launch(k_ba_pose_t, dim3((v.n_poses + 255) / 256), dim3(256), 0, s, v.n_poses, v.pose_R, v.pose_C,
                    v.pose_t);
}

}  // namespace sfmloc

using namespace sfmloc;

extern "C" int sfmloc_sfm_adjust(sfmloc_sfm *hh, uint32_t what, sfmloc_ba_report *rep) {
  SFM_CHECK(hh, SFMLOC_EINVAL, "sfmloc_sfm_adjust: null handle");
  SFM_CHECK(what == 0 || what == SFMLOC_BA_ROTATION || what == SFMLOC_BA_TRANSLATION ||
                what == (SFMLOC_BA_ROTATION | SFMLOC_BA_TRANSLATION) || what == SFMLOC_BA_STRUCTURE,
            SFMLOC_EINVAL,
            "sfmloc_sfm_adjust: what = %u: only the separable commands (-c) are supported: structure alone, or "
            "rotations / translations alone; nothing with intrinsics, no structure together with a pose part", what);
  Sfm *h = reinterpret_cast<Sfm *>(hh);
  if (rep) memset(rep, 0, sizeof *rep);
  if (what == 0) return SFMLOC_OK;
  SFM_HIP(hipSetDevice(h->device));
  try {
    return ba_separable_run(*h, what, rep);
  } catch (const std::bad_alloc &) {
    set_error("sfmloc_sfm_adjust: out of host memory");
    return SFMLOC_ENOMEM;
  }
}
