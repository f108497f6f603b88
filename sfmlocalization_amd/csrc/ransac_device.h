// What more than one translation unit of the query path's AC-RANSAC uses on the device: K3 and K5 (acransac.hip) and K4
// (k4_matchset.hip), whose last kernel starts K5.  Everything is in the anonymous namespace: each unit compiles its own
// copy, no device symbol crosses one.
#pragma once

#include "geom_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
using namespace geom;

namespace {

constexpr int kThreads = 256;

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
