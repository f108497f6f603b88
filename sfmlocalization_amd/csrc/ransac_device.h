// What more than one translation unit's AC-RANSAC uses on the device: K3 and K5 (acransac.hip), K4 (k4_matchset.hip),
// whose last kernel starts K5, and the relative poses (relpose.hip).  Everything is in the anonymous namespace: each unit compiles its own
// copy, no device symbol crosses one.
#pragma once

#include <float.h>

#include "geom_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
using namespace geom;

namespace {

constexpr int kThreads = 256;

// ---- block-wide helpers of the AC-RANSAC loops (256 threads): K3 and K5 (acransac.hip), relative poses (relpose.hip)
__device__ __forceinline__ bool pair_less(uint64_t ka, uint32_t ia, uint64_t kb, uint32_t ib) {
  return ka < kb || (ka == kb && ia < ib);
}

// ascending bitonic sort of (key, idx) pairs, P a power of two
__device__ void bitonic_sort(uint64_t *key, uint32_t *idx, int P) {
  for (int k = 2; k <= P; k <<= 1) {
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int t = threadIdx.x; t < (P >> 1); t += kThreads) {
        const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int l = i + j;
        const bool up = (i & k) == 0;
        const uint64_t ka = key[i], kb = key[l];
        const uint32_t ia = idx[i], ib = idx[l];
        const bool a_gt_b = pair_less(kb, ib, ka, ia);
        if (a_gt_b == up) {
          key[i] = kb;
          key[l] = ka;
          idx[i] = ib;
          idx[l] = ia;
        }
      }
      __syncthreads();
    }
  }
}

struct NfaBest {
  double nfa;
  int k;
};

// bestNFA of OpenMVG over the sorted residuals key[0..n): min over k in (s, n] with e_k <= max_thr of
//   loge0 + logalpha(e_k) * (k - s) + logc_n[k] + logc_k[k];  first k on ties.  All threads return the result.
__device__ NfaBest best_nfa_block(const uint64_t *key, int n, int s, double max_thr, double logalpha0, double mult,
                                  double loge0, const float *logc_n, const float *logc_k, double *red_nfa,
                                  int *red_k) {
  double lb = pos_inf();
  int lk = 0x7FFFFFFF;
  for (int kk = s + 1 + (int)threadIdx.x; kk <= n; kk += kThreads) {
    const double ek = u2d(key[kk - 1]);
    if (ek <= max_thr) {
      const double logalpha = logalpha0 + mult * det_log10(ek + (double)FLT_EPSILON);
      const double nfa = loge0 + logalpha * (double)(kk - s) + (double)logc_n[kk] + (double)logc_k[kk];
      if (nfa < lb) {
        lb = nfa;
        lk = kk;
      }
    }
  }
  // wave reduce (64 lanes), then across the 4 waves through LDS
  for (int off = 32; off > 0; off >>= 1) {
    const double ob = __shfl_down(lb, off, 64);
    const int ok = __shfl_down(lk, off, 64);
    if (ob < lb || (ob == lb && ok < lk)) {
      lb = ob;
      lk = ok;
    }
  }
  __syncthreads();  // red_* may still be read by the previous call's consumers
  if ((threadIdx.x & 63) == 0) {
    red_nfa[threadIdx.x >> 6] = lb;
    red_k[threadIdx.x >> 6] = lk;
  }
  __syncthreads();
  NfaBest r{red_nfa[0], red_k[0]};
  for (int w = 1; w < kThreads / 64; ++w) {
    if (red_nfa[w] < r.nfa || (red_nfa[w] == r.nfa && red_k[w] < r.k)) {
      r.nfa = red_nfa[w];
      r.k = red_k[w];
    }
  }
  return r;
}

__device__ __forceinline__ int next_pow2(int n) {
  int p = 64;
  while (p < n) p <<= 1;
  return p;
}


// logcombi tables of OpenMVG (float): logc_n[k] = log10 C(n,k), logc_k[m] = log10 C(m,s); L10[i] = log10(i).
// logcombi(k,n) = sum_{i=1..min(k,n-k)} (L10[n-i+1] - L10[i]) accumulated in double in that order, so the
// values for k = 0..n/2 are the running sums of one sequential pass; the rest is symmetry.  The pass itself cannot be
// split (the rounding of every partial sum is part of the result), but its terms can be fetched by the whole
// workgroup: `terms` (n / 2 + 1 doubles of LDS) takes L10[n-k+1] - L10[k], then thread 0 adds them up out of LDS with
// eight loads in flight -- the same sums as a loop over global memory, which cost ~50 us of dependent L2 latency per
// call on the critical path of K3 and K5.
__device__ void logc_n_block(int n, const double *__restrict__ L10, double *terms, float *logc_n, int n_threads) {
  const int kmax = n / 2;  // 2 k <= n
  for (int k = 1 + (int)threadIdx.x; k <= kmax; k += n_threads) terms[k] = L10[n - k + 1] - L10[k];
  __syncthreads();
  if (threadIdx.x == 0) {
    double r = 0.0;
    logc_n[0] = 0.0f;
    logc_n[n] = 0.0f;
    int k = 1;
    for (; k + 7 <= kmax; k += 8) {
      double t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) t[u] = terms[k + u];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        r += t[u];
        logc_n[k + u] = (float)r;
        logc_n[n - k - u] = (float)r;
      }
    }
    for (; k <= kmax; ++k) {
      r += terms[k];
      logc_n[k] = (float)r;
      logc_n[n - k] = (float)r;
    }
  }
}

__device__ void logcombi_tables_block(int s, int n, const double *__restrict__ L10, double *terms, float *logc_n,
                                      float *logc_k, int n_threads = kThreads) {
  logc_n_block(n, L10, terms, logc_n, n_threads);
  for (int m = threadIdx.x; m <= n; m += n_threads) {
    float v = 0.0f;
    if (s < m) {
      int k = s;
      if (m - k < k) k = m - k;
      double r = 0.0;
      for (int i = 1; i <= k; ++i) r += L10[m - i + 1] - L10[i];
      v = (float)r;
    }
    logc_k[m] = v;
  }
  __syncthreads();
}

// the start of K5: the state machine's initial state, the K^-1-normalised image points and the logcombi tables.  A
// workgroup of n_threads threads; n = the number of 2D-3D correspondences (what k_match_set_finish counted).
__device__ void p3p_init_block(const P3pArgs &A, int n, int n_threads, double *s_terms) {
  P3pState &st = *A.state;
  __shared__ int go;
  if (threadIdx.x == 0) {
    st.n = n;
    st.iter = 0;
    const long maxit = A.max_iteration;
    st.n_reserve = (int)(maxit / 10);
    st.n_iter = (int)(maxit - maxit / 10);
    st.n_index = n;
    st.identity = 1;
    st.n_in = 0;
    st.done = 0;
    st.rounds = 0;
    st.status = 0;
    st.arrive = 0u;
    st.finished = 0;
    st.batch_limit = 1 << 30;
    st.switch_iter = 0;
    st.prep_iter = -1;
    st.prep_n = 0;
    st.first_hit = ~0u;
    st.min_nfa = pos_inf();
    st.errmax = pos_inf();
    for (int i = 0; i < 12; ++i) st.model[i] = 0.0;
    go = 1;
    // localization.cpp:506 "cpt > MINUM_NUMBER_OF_POINT_RESECTION"; ACRANSAC: nData <= sizeSample -> nothing
    if (n <= A.min_resection_points || n <= (A.uncal ? 6 : 3)) {
      st.done = 1;
      st.finished = 1;  // nothing to estimate: the result record written below is final
      go = 0;
    }
    if (n > A.max_n) {
      st.done = 1;
      st.finished = 1;
      st.status = 4;
      go = 0;
    }
    A.result->ok = 0;
    A.result->n_inliers = 0;
    A.result->n_matches_2d3d = n;
    A.result->iterations = 0;
    A.result->status = st.status;
    // a query that ends here (too few correspondences) must not report the PREVIOUS query's numbers: the record is the
    // context's, and a result is a function of the query alone (bench.py / tests compare results bit for bit)
    A.result->reserved = 0;
    A.result->nfa = 0.0;
    A.result->error_max = 0.0;
    for (int i = 0; i < 12; ++i) A.result->P[i] = 0.0;
    for (int i = 0; i < 9; ++i) {
      A.result->K[i] = 0.0;
      A.result->R[i] = 0.0;
    }
    for (int i = 0; i < 3; ++i) {
      A.result->t[i] = 0.0;
      A.result->center[i] = 0.0;
    }
  }
  __syncthreads();
  if (!go) return;
  // normalise by K^-1: x * (1/f) + (-pp/f)
  const double inv_f = 1.0 / A.focal;
  const double cx = -A.ppx * inv_f, cy = -A.ppy * inv_f;
  for (int i = threadIdx.x; i < n; i += n_threads) {
    A.xn[2 * i] = A.pt2d[2 * i] * inv_f + cx;
    A.xn[2 * i + 1] = A.pt2d[2 * i + 1] * inv_f + cy;
  }
  // (the table pass wants n / 2 + 1 doubles of scratch: LDS up to kP3pMaxN correspondences, global beyond)
  logcombi_tables_block(A.uncal ? 6 : 3, n, A.L10, n > kP3pMaxN ? A.ws_terms : s_terms, A.logc_n, A.logc_k, n_threads);
}

}  // namespace
}  // namespace sfmloc
