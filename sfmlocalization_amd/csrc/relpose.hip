// sfmloc_relative_poses: the relative pose of every matched view pair (the first stage of openMVG_main_GlobalSfM): the
// essential matrix by the five-point solver under AC-RANSAC, its decomposition, the cheirality count.  The semantics
// are stated in include/sfmloc.h ("Relative poses"); tests/relpose_np.py restates every operation.  f64, only + - * /
// sqrt, unfused (the library's -ffp-contract=off), every sum in a fixed order, no float atomics.  The call's scene is a
// PairScene on the host (pair_scene.h: its checks) and a PairDev on the device (twoview_device.h: its upload).
//
//   bearings    k_rp_bearings: (a, b, u, v) per match, once (the undistortion's bisection is the expensive part).
//   pairs       k_relpose: one workgroup of 256 threads per pair, K3's block-wide AC-RANSAC loop (fmatrix_filter_view of
//               acransac.hip: residuals -> bitonic sort -> best_nfa_block, the 10 % reserve, the reduction to the inlier
//               set) with the match arrays, the keys and the logcombi tables in LDS through the same Store abstraction.
//               While sampling is uniform the hypotheses are solved kRpPre = 16 at a time, one per group of 16 lanes
//               (essential_device.h); afterwards group 0 solves the iteration's one.  After the rounds thread 0
//               decomposes the winner and the inliers x 4 candidates are spread over the lanes for the cheirality count
//               (integer atomics on LDS).
//   large       k_relpose_large: the pairs with more than kLdsMaxM matches, kRpLargeSlots persistent workgroups each
//               owning a global-memory slot; the same function, the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "essential_device.h"
#include "ransac_device.h"
#include "relpose_host.h"
#include "twoview_device.h"

namespace sfmloc {
namespace {

using essential::RpGroupLds;

thread_local double g_relpose_last_ms = 0.0;

constexpr uint32_t STAGE_RELPOSE = 6;  // (geom_device.h's stage ids end at 5)
constexpr int kRpPre = kThreads / essential::kRpGroup;  // hypotheses solved side by side: one per group of lanes
constexpr int kRpLdsMaxM = (int)relpose_host::kLdsMaxM;
constexpr int kRpLargeSlots = 8;
constexpr int kRpL10 = (int)relpose_host::kLargeMaxM + 2;
static_assert(kRpLdsMaxM == kFMaxM, "the LDS form holds what K3's does");

struct Relpose {
  std::vector<sfmloc_relpose_result> res;
  std::vector<uint64_t> off;  // [n_pairs + 1]
  std::vector<uint32_t> idx;
};

struct RpArgs : PairDev {
  int n_iter;
  double precision;
  uint64_t seed;
  const double *bear;  // [match][4]: a, b (view I), u, v (view J)
  const double *L10;
  sfmloc_relpose_result *res;
  uint32_t *inl;
};

struct RpSmall {
  double pre_models[kRpPre][9 * essential::kRpMaxModels];
  int pre_nm[kRpPre];
  int pre_smp[kRpPre][5];
  double best_model[9];
  int best_smp[5];
  double red_nfa[kThreads / 64];
  int red_k[kThreads / 64];
  double cand_R[2][9], cand_t[3];
  int front[4];
};
struct RpShared {
  uint64_t key[kRpLdsMaxM];
  uint32_t idx[kRpLdsMaxM];
  int32_t vec_index[kRpLdsMaxM];
  int32_t best_inl[kRpLdsMaxM];
  float logc_n[kRpLdsMaxM + 1];
  float logc_k[kRpLdsMaxM + 1];
  RpSmall small;
  RpGroupLds grp[kRpPre];
};
static_assert(sizeof(RpShared) <= 160 * 1024, "one workgroup's LDS on gfx950");
struct RpLargeShared {
  RpSmall small;
  RpGroupLds grp[kRpPre];
};
struct RpStoreLds {
  RpShared *S;
  __device__ __forceinline__ uint64_t *key() const { return S->key; }
  __device__ __forceinline__ uint32_t *idx() const { return S->idx; }
  __device__ __forceinline__ int32_t *vec_index() const { return S->vec_index; }
  __device__ __forceinline__ int32_t *best_inl() const { return S->best_inl; }
  __device__ __forceinline__ float *logc_n() const { return S->logc_n; }
  __device__ __forceinline__ float *logc_k() const { return S->logc_k; }
};
struct RpStoreGlobal {
  uint64_t *k;
  uint32_t *i;
  int32_t *vi, *bi;
  float *ln, *lk;
  __device__ __forceinline__ uint64_t *key() const { return k; }
  __device__ __forceinline__ uint32_t *idx() const { return i; }
  __device__ __forceinline__ int32_t *vec_index() const { return vi; }
  __device__ __forceinline__ int32_t *best_inl() const { return bi; }
  __device__ __forceinline__ float *logc_n() const { return ln; }
  __device__ __forceinline__ float *logc_k() const { return lk; }
};
struct RpLargeArgs {
  const uint32_t *list;
  uint32_t n;
  uint64_t *key;
  uint32_t *idx;
  int32_t *vec_index, *best_inl;
  float *logc_n, *logc_k;
  int slot_m;
};

__global__ void k_rp_fill_log10(double *L10, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) L10[i] = (i == 0) ? 0.0 : det_log10((double)i);
}

// sfmloc.h "bearings": one workgroup per pair walks the pair's matches
__global__ __launch_bounds__(256) void k_rp_bearings(PairDev D, double *__restrict__ bear) {
  const uint32_t k = blockIdx.x;
  if (k >= D.n_pairs) return;
  const ViewCam ci = view_cam(D, D.pairs[2 * (size_t)k]), cj = view_cam(D, D.pairs[2 * (size_t)k + 1]);
  for (uint64_t t = D.offsets[k] + threadIdx.x; t < D.offsets[k + 1]; t += 256) {
    feature_bearing(D, ci, D.match_i[t], &bear[4 * t], &bear[4 * t + 1]);
    feature_bearing(D, cj, D.match_j[t], &bear[4 * t + 2], &bear[4 * t + 3]);
  }
}

// sfmloc.h "sample": OpenMVG UniformSample over five draws of two Philox blocks; the counter words are (iteration, I,
// J, stage | block << 8)
__device__ __forceinline__ void rp_sample5(const int32_t *vec_index, int n, uint64_t seed, uint32_t vi, uint32_t vj,
                                           uint32_t iter, int32_t *samples) {
  uint32_t c0[4] = {iter, vi, vj, STAGE_RELPOSE};
  uint32_t c1[4] = {iter, vi, vj, STAGE_RELPOSE | (1u << 8)};
  philox4x32_10(c0, (uint32_t)seed, (uint32_t)(seed >> 32));
  philox4x32_10(c1, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint32_t d[5] = {c0[0], c0[1], c0[2], c0[3], c1[0]};
  int32_t s[5] = {0, 0, 0, 0, 0};
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    int32_t r = (int32_t)(d[i] % (uint32_t)(n - i));
    int j = 0;
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if (q < i && j == q && r >= s[q]) {
        ++r;
        ++j;
      }
#pragma unroll
    for (int q = 4; q > 0; --q)
      if (q <= i && q > j) s[q] = s[q - 1];
#pragma unroll
    for (int q = 0; q < 5; ++q)
      if (q == j) s[q] = r;
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) samples[i] = vec_index ? vec_index[s[i]] : s[i];
}

// sfmloc.h "cheirality": the two-view point of one match under (R, t) lies in front of both cameras
__device__ __forceinline__ bool rp_in_front(const double *R, const double *t, double a, double b, double u, double v) {
  double zi, zj;
  const bool ok = two_view_depths(R, t, a, b, u, v, &zi, &zj);
  return ok && zi > 0.0 && zj > 0.0;
}

// One pair by the whole workgroup; `st` says where the per-match arrays are (they hold the pair's matches: the caller
// checked).  The loop is fmatrix_filter_view's (acransac.hip) with the five-point kernel.
template <typename Store>
__device__ void relpose_pair(const RpArgs &A, uint32_t k, Store st, RpSmall &S, RpGroupLds *grp) {
  const int tid = threadIdx.x;
  const uint64_t off = A.offsets[k];
  const int m = (int)(A.offsets[k + 1] - off);
  const uint32_t vi = A.pairs[2 * (size_t)k], vj = A.pairs[2 * (size_t)k + 1];
  sfmloc_relpose_result &R = A.res[k];
  constexpr int s = 5;
  if (tid == 0) {
    R.ok = 0;
    R.n_matches = (uint32_t)m;
    R.n_inliers = 0;
    for (int i = 0; i < 5; ++i) R.sample[i] = 0;
    for (int i = 0; i < 4; ++i) R.front[i] = 0;
    R.choice = 0;
    for (int i = 0; i < 9; ++i) {
      R.E[i] = 0.0;
      R.R[i] = 0.0;
    }
    for (int i = 0; i < 3; ++i) R.t[i] = 0.0;
    R.error_max_px = 0.0;
    R.nfa = 0.0;
  }
  if (m <= s) return;  // sfmloc.h "gate"
  const double *bear = A.bear + 4 * off;
  const double fj = A.intr[6 * (size_t)A.view_intr[vj]];
  const double fj2 = fj * fj;
  const double w2 = (double)A.view_wh[2 * (size_t)vj], h2 = (double)A.view_wh[2 * (size_t)vj + 1];
  const double Dg = sqrt(w2 * w2 + h2 * h2);
  const double logalpha0 = det_log10(2.0 * Dg / (w2 * h2));
  const double max_thr = A.precision * A.precision;
  const double loge0 = det_log10(10.0 * (double)(m - s));
  const int P = next_pow2(m);
  const int g = tid / essential::kRpGroup;

  // the hypothesis of iteration `it` on this lane's group (a group without one runs on zeros); every lane of the group
  // holds the same sample
  auto solve = [&](bool have, const int32_t *vec_index, int n_index, long it) {
    int32_t smp[5] = {0, 0, 0, 0, 0};
    double x1[10], x2[10];
#pragma unroll
    for (int i = 0; i < 10; ++i) x1[i] = x2[i] = 0.0;
    if (have) {
      rp_sample5(vec_index, n_index, A.seed, vi, vj, (uint32_t)it, smp);
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        x1[2 * i] = bear[4 * smp[i]];
        x1[2 * i + 1] = bear[4 * smp[i] + 1];
        x2[2 * i] = bear[4 * smp[i] + 2];
        x2[2 * i + 1] = bear[4 * smp[i] + 3];
      }
    }
    const int nm = essential::five_point_group(grp[g], x1, x2, S.pre_models[g]);
    if ((tid & (essential::kRpGroup - 1)) == 0) {
      S.pre_nm[g] = have ? nm : 0;
#pragma unroll
      for (int i = 0; i < 5; ++i) S.pre_smp[g][i] = smp[i];
    }
  };

  logcombi_tables_block(s, m, A.L10, reinterpret_cast<double *>(st.key()), st.logc_n(), st.logc_k());  // the key array is free until the first sort

  double min_nfa = pos_inf();
  int n_in = 0;
  long n_iter = A.n_iter;
  long n_reserve = n_iter / 10;
  n_iter -= n_reserve;
  bool identity = true;
  int n_index = m;
  long pre_base = -1;

  for (long iter = 0; iter < n_iter; ++iter) {
    int slot;
    if (identity) {
      if (pre_base < 0 || iter >= pre_base + kRpPre) {
        __syncthreads();
        pre_base = iter;
        solve(true, nullptr, m, pre_base + g);
        __syncthreads();
      }
      slot = (int)(iter - pre_base);
    } else {
      __syncthreads();
      solve(g == 0, st.vec_index(), n_index, iter);
      __syncthreads();
      slot = 0;
    }
    const double *models = S.pre_models[slot];
    const int nm = S.pre_nm[slot];
    bool better = false;
    for (int q = 0; q < nm; ++q) {
      double M[9];
      for (int e = 0; e < 9; ++e) M[e] = models[9 * q + e];
      __syncthreads();  // key/idx of the previous model are no longer read
      for (int p = tid; p < P; p += kThreads) {
        uint64_t kv = ~0ull;
        if (p < m) kv = d2u(err_fmatrix(M, bear[4 * p], bear[4 * p + 1], bear[4 * p + 2], bear[4 * p + 3]) * fj2);
        st.key()[p] = kv;
        st.idx()[p] = (uint32_t)p;
      }
      __syncthreads();
      bitonic_sort(st.key(), st.idx(), P);
      const NfaBest b = best_nfa_block(st.key(), m, s, max_thr, logalpha0, 0.5, loge0, st.logc_n(), st.logc_k(), S.red_nfa,
                                       S.red_k);
      if (b.nfa < min_nfa) {
        better = true;
        min_nfa = b.nfa;
        n_in = b.k;
        for (int p = tid; p < n_in; p += kThreads) st.best_inl()[p] = (int32_t)st.idx()[p];
        if (tid < 9) S.best_model[tid] = M[tid];
        if (tid < 5) S.best_smp[tid] = S.pre_smp[slot][tid];
      }
    }
    if ((better && min_nfa < 0.0) || (iter + 1 == n_iter && n_reserve)) {
      if (n_in == 0) {
        n_iter++;
        n_reserve--;
      } else {
        __syncthreads();
        for (int p = tid; p < n_in; p += kThreads) st.vec_index()[p] = st.best_inl()[p];
        n_index = n_in;
        identity = false;
        if (n_reserve) {
          n_iter = iter + 1 + n_reserve;
          n_reserve = 0;
        }
      }
    }
  }
  __syncthreads();
  if (min_nfa >= 0.0) {  // sfmloc.h "decision": nothing meaningful
    if (tid == 0) R.nfa = min_nfa;
    return;
  }
  // sfmloc.h "decompose", "cheirality"
  if (tid == 0) {
    const double *E = S.best_model;
    double Am[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) Am[i][j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
    jacobi_fixed<3>(Am, V);
    const double d[3] = {Am[0][0], Am[1][1], Am[2][2]};
    essential::decompose_from_jacobi(E, d, V, S.cand_R[0], S.cand_R[1], S.cand_t);
  }
  if (tid < 4) S.front[tid] = 0;
  __syncthreads();
  for (int q = tid; q < 4 * n_in; q += kThreads) {
    const int c = q & 3, p = st.best_inl()[q >> 2];
    const double sg = (c & 1) ? -1.0 : 1.0;
    const double t[3] = {sg * S.cand_t[0], sg * S.cand_t[1], sg * S.cand_t[2]};
    if (rp_in_front(S.cand_R[c >> 1], t, bear[4 * p], bear[4 * p + 1], bear[4 * p + 2], bear[4 * p + 3]))
      atomicAdd(&S.front[c], 1);  // (an integer count: the same whatever the order)
  }
  for (int p = tid; p < n_in; p += kThreads) A.inl[off + p] = (uint32_t)st.best_inl()[p];
  __syncthreads();
  if (tid == 0) {
    int choice = 0;
    for (int c = 1; c < 4; ++c)
      if (S.front[c] > S.front[choice]) choice = c;
    const int last = st.best_inl()[n_in - 1];
    const double errmax =
        err_fmatrix(S.best_model, bear[4 * last], bear[4 * last + 1], bear[4 * last + 2], bear[4 * last + 3]) * fj2;
    R.n_inliers = (uint32_t)n_in;
    for (int i = 0; i < 5; ++i) R.sample[i] = (uint32_t)S.best_smp[i];
    for (int c = 0; c < 4; ++c) R.front[c] = (uint32_t)S.front[c];
    R.choice = (uint32_t)choice;
    const double sg = (choice & 1) ? -1.0 : 1.0;
    for (int i = 0; i < 9; ++i) {
      R.E[i] = S.best_model[i];
      R.R[i] = S.cand_R[choice >> 1][i];
    }
    for (int i = 0; i < 3; ++i) R.t[i] = sg * S.cand_t[i];
    R.error_max_px = sqrt(errmax);
    R.nfa = min_nfa;
    R.ok = ((double)n_in > 2.5 * s && S.front[choice] > 0) ? 1u : 0u;
  }
}

__global__ __launch_bounds__(kThreads) void k_relpose(RpArgs A) {
  extern __shared__ unsigned char smem_raw[];
  RpShared &S = *reinterpret_cast<RpShared *>(smem_raw);
  const uint32_t k = blockIdx.x;
  if (k >= A.n_pairs) return;
  if (A.offsets[k + 1] - A.offsets[k] > (uint64_t)kRpLdsMaxM) return;  // k_relpose_large's
  relpose_pair(A, k, RpStoreLds{&S}, S.small, S.grp);
}

__global__ __launch_bounds__(kThreads) void k_relpose_large(RpArgs A, RpLargeArgs W) {
  extern __shared__ unsigned char smem_raw[];
  RpLargeShared &S = *reinterpret_cast<RpLargeShared *>(smem_raw);
  const size_t o = (size_t)blockIdx.x * W.slot_m;
  RpStoreGlobal st{W.key + o, W.idx + o, W.vec_index + o, W.best_inl + o, W.logc_n + (size_t)blockIdx.x * (W.slot_m + 1),
                   W.logc_k + (size_t)blockIdx.x * (W.slot_m + 1)};
  for (uint32_t t = blockIdx.x; t < W.n; t += gridDim.x) {
    const uint32_t k = W.list[t];
    if (A.offsets[k + 1] - A.offsets[k] <= (uint64_t)W.slot_m) relpose_pair(A, k, st, S.small, S.grp);
    __syncthreads();
  }
}

// sfmloc_debug_five_point: four hypotheses per wave
__global__ __launch_bounds__(64) void k_debug_five_point(const double *in, int n, double *out) {
  __shared__ RpGroupLds L[4];
  __shared__ double models[4][90];
  const int g = threadIdx.x / essential::kRpGroup;
  const int h = blockIdx.x * 4 + g;
  double x1[10], x2[10];
  for (int i = 0; i < 10; ++i) {
    x1[i] = h < n ? in[20 * (size_t)h + i] : 0.0;
    x2[i] = h < n ? in[20 * (size_t)h + 10 + i] : 0.0;
  }
  const int nm = essential::five_point_group(L[g], x1, x2, models[g]);
  if (h < n && (threadIdx.x & (essential::kRpGroup - 1)) == 0) {
    double *o = out + 91 * (size_t)h;
    o[0] = (double)nm;
    for (int i = 0; i < 90; ++i) o[1 + i] = i < 9 * nm ? models[g][i] : 0.0;
  }
}

int relpose_device(const PairScene &sc, const sfmloc_relpose_options &opt, const std::vector<uint32_t> &large,
                   uint32_t large_max_m, hipStream_t s, Relpose *r) {
  const uint32_t n_pairs = sc.n_pairs;
  const uint64_t *offsets = sc.offsets;
  const uint64_t total = offsets[n_pairs];
  PairSceneBufs scene;
  DevBuf<uint32_t> d_inl, d_large;
  DevBuf<double> d_bear, d_L10;
  DevBuf<sfmloc_relpose_result> d_res;
  SFM_RC(scene.upload(sc, s));
  SFM_RC(d_bear.alloc(nullptr, 4 * (size_t)total));
  SFM_RC(d_inl.alloc(nullptr, (size_t)total));
  SFM_RC(d_L10.alloc(nullptr, kRpL10));
  SFM_RC(d_res.alloc(nullptr, n_pairs));
  SFM_RC(d_res.zero(n_pairs, s));  // (the records' padding too)
  SFM_RC(dev_launch(k_rp_fill_log10, dim3((kRpL10 + 255) / 256), dim3(256), 0, s, d_L10, kRpL10));
  SFM_RC(dev_launch(k_rp_bearings, dim3(n_pairs), dim3(256), 0, s, scene.dev(), d_bear));
  RpArgs A{};
  static_cast<PairDev &>(A) = scene.dev();
  A.n_iter = (int)opt.max_iteration;
  A.precision = opt.precision_px;
  A.seed = opt.seed;
  A.bear = d_bear;
  A.L10 = d_L10;
  A.res = d_res;
  A.inl = d_inl;
  SFM_RC(dev_launch(k_relpose, dim3(n_pairs), dim3(kThreads), sizeof(RpShared), s, A));
  DevBuf<uint64_t> d_key;
  DevBuf<uint32_t> d_idx;
  DevBuf<int32_t> d_vi, d_bi;
  DevBuf<float> d_ln, d_lk;
  if (!large.empty()) {  // the pairs the LDS form left: slots of a power of two that holds the longest
    int slot_m = 2 * kRpLdsMaxM;
    while (slot_m < (int)large_max_m) slot_m <<= 1;
    const size_t n_slots = large.size() < (size_t)kRpLargeSlots ? large.size() : (size_t)kRpLargeSlots;
    SFM_RC(dev_upload(nullptr, d_large, large.data(), large.size(), s));
    SFM_RC(d_key.alloc(nullptr, n_slots * slot_m));
    SFM_RC(d_idx.alloc(nullptr, n_slots * slot_m));
    SFM_RC(d_vi.alloc(nullptr, n_slots * slot_m));
    SFM_RC(d_bi.alloc(nullptr, n_slots * slot_m));
    SFM_RC(d_ln.alloc(nullptr, n_slots * ((size_t)slot_m + 1)));
    SFM_RC(d_lk.alloc(nullptr, n_slots * ((size_t)slot_m + 1)));
    RpLargeArgs W;
    W.list = d_large;
    W.n = (uint32_t)large.size();
    W.key = d_key;
    W.idx = d_idx;
    W.vec_index = d_vi;
    W.best_inl = d_bi;
    W.logc_n = d_ln;
    W.logc_k = d_lk;
    W.slot_m = slot_m;
    SFM_RC(dev_launch(k_relpose_large, dim3((unsigned)n_slots), dim3(kThreads), sizeof(RpLargeShared), s, A, W));
  }
  std::vector<uint32_t> inl((size_t)total);
  SFM_RC(d_res.download(r->res.data(), n_pairs, s));
  if (total) SFM_RC(d_inl.download(inl.data(), total, s));
  SFM_HIP(hipStreamSynchronize(s));
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t n = r->res[k].n_inliers;
    r->idx.insert(r->idx.end(), inl.begin() + (size_t)offsets[k], inl.begin() + (size_t)offsets[k] + n);
    r->off[k + 1] = r->idx.size();
  }
  return SFMLOC_OK;
}

int relpose_impl(int device, const PairScene &sc, const sfmloc_relpose_options &opt, Relpose *r) {
  std::string err;
  const int rc = relpose_host::check(sc, opt, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  std::vector<uint32_t> large;
  uint32_t large_max_m = 0;
  relpose_host::split_large(sc, &large, &large_max_m);
  r->res.assign(sc.n_pairs, sfmloc_relpose_result{});
  r->off.assign((size_t)sc.n_pairs + 1, 0);
  return timed_call(device, &g_relpose_last_ms, sc.n_pairs != 0,
                    [&](hipStream_t s) { return relpose_device(sc, opt, large, large_max_m, s, r); });
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_relpose_default_options(sfmloc_relpose_options *o) {
  if (!o) return;
  o->max_iteration = 256;
  o->reserved = 0;
  o->precision_px = 2.5;
  o->seed = 0x5F3759DF12345678ull;
}

int sfmloc_relative_poses(int device, const uint64_t *view_off, uint32_t n_views, const float *kpt_xy,
                          const uint32_t *view_wh, const uint32_t *view_intrinsic, const double *intrinsics,
                          const uint32_t *intrinsic_type, uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs,
                          const uint64_t *offsets, const uint32_t *match_i, const uint32_t *match_j,
                          const sfmloc_relpose_options *opt, sfmloc_relpose **out) {
  const PairScene sc{view_off,     n_views, kpt_xy,  view_wh, view_intrinsic, intrinsics, intrinsic_type,
                     n_intrinsics, pairs,   n_pairs, offsets, match_i,        match_j};
  const sfmloc_relpose_options o = options_or(opt, sfmloc_relpose_default_options);
  return make_handle<Relpose>("sfmloc_relative_poses", out, [&](Relpose *r) { return relpose_impl(device, sc, o, r); });
}

int sfmloc_relpose_results(const sfmloc_relpose *rr, sfmloc_relpose_result *out) {
  SFM_CHECK(rr, SFMLOC_EINVAL, "sfmloc_relpose_results: null handle");
  const Relpose *r = reinterpret_cast<const Relpose *>(rr);
  SFM_CHECK(out || r->res.empty(), SFMLOC_EINVAL, "sfmloc_relpose_results: null argument");
  if (!r->res.empty()) memcpy(out, r->res.data(), r->res.size() * sizeof(sfmloc_relpose_result));
  return SFMLOC_OK;
}

int sfmloc_relpose_inliers(const sfmloc_relpose *rr, uint64_t *off, uint32_t *idx) {
  SFM_CHECK(rr, SFMLOC_EINVAL, "sfmloc_relpose_inliers: null handle");
  const Relpose *r = reinterpret_cast<const Relpose *>(rr);
  if (off) memcpy(off, r->off.data(), r->off.size() * sizeof(uint64_t));
  if (idx && !r->idx.empty()) memcpy(idx, r->idx.data(), r->idx.size() * sizeof(uint32_t));
  return SFMLOC_OK;
}

void sfmloc_relpose_destroy(sfmloc_relpose *r) { delete reinterpret_cast<Relpose *>(r); }

double sfmloc_relpose_last_ms(void) { return g_relpose_last_ms; }

int sfmloc_debug_five_point(int device, const double *in, int n, double *out) {
  SFM_CHECK(in && out && n > 0, SFMLOC_EINVAL, "sfmloc_debug_five_point: bad argument");
  int rc = CallScope::use_device(device);
  if (rc) return rc;
  CallScope d;
  double ms = 0.0;
  if ((rc = d.open(false, &ms))) return rc;
  DevBuf<double> d_in, d_out;
  if ((rc = dev_upload(nullptr, d_in, in, 20 * (size_t)n, d.s))) return rc;
  if ((rc = d_out.alloc(nullptr, 91 * (size_t)n))) return rc;
  SFM_RC(dev_launch(k_debug_five_point, dim3((n + 3) / 4), dim3(64), 0, d.s, d_in, n, d_out));
  SFM_RC(d_out.download(out, 91 * (size_t)n, d.s));
  SFM_HIP(hipStreamSynchronize(d.s));
  return SFMLOC_OK;
}

}  // extern "C"
