// sfmloc_global_poses: rotation and translation averaging over relative poses, the middle stage of
// openMVG_main_GlobalSfM.  The semantics are stated in include/sfmloc.h ("Global poses"); the kernels below name the
// paragraph they implement.
//
// The workload is small for the chip (10 000 views, 50 000 pairs in the project's corridor): the stage is bound by
// launch latency and by dependent reductions, not by bandwidth.  Hence
//   gather      every matrix-vector product and every per-view sum is a gather over the CSR adjacency: one lane per
//               view, one wave per view above gposes_host::kWaveDegree pairs (gp_pick / gp_gather), neighbours in index
//               order.  Nothing is atomically added; the sum order is fixed and independent of the pair list's order.
//   partials    scalar products and costs leave one partial per workgroup; every workgroup of the next kernel sums them
//               itself by the same fixed tree (gp_sum): store, then sum.  No kernel waits for another workgroup.
//   one PCG     k_gp_apply / k_gp_step1 / k_gp_step2, templated on the block kind: 0 the chordal system (3 x 3 blocks
//               rel_R, 9 values per view), 1 the IRLS system (scalar weights, 3 values per view), 2 the translations
//               (3 x 3 blocks W, 3 values per view), 3 the scales of sfmloc_global_poses_scaled (scalar weights, 1 value
//               per node: there the "views" of GpDev are the pairs and its "pairs" the wedges).  The host passes the iteration number; a solve that has stopped at
//               iteration done_at makes every later queued launch return at once.  kPcgChunk iterations are queued
//               between two looks at the state record.
// f64, unfused (-ffp-contract=off), only + - * / sqrt on the device.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "geom_device.h"
#include "globalposes_host.h"
#include "graph_device.h"
#include "pairscales_host.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

using gposes_host::kDirBit;
using gposes_host::kWaveDegree;

thread_local double g_gposes_last_ms = 0.0;

constexpr int kPcgChunk = 32;            // PCG iterations enqueued between two looks at the state record
constexpr uint32_t kNever = 0xFFFFFFFFu;  // GpState::done_at of a solve that runs

struct Gposes {
  uint32_t n_views = 0;
  std::vector<uint8_t> in_comp;
  std::vector<double> R, C;
  std::vector<sfmloc_gposes_pair> pairs;
  sfmloc_gposes_report rep{};
  std::vector<double> base, wedge_w;  // sfmloc_global_poses_scaled: per pair, per wedge
  sfmloc_gpscale_report srep{};
};

// what sfmloc_global_poses_scaled adds to the arguments
struct GpScaleIn {
  const uint32_t *kl;
  const double *ratio;
  uint32_t n_wedges;
  sfmloc_gpscale_options opt;
};

// values per view (node) of a block kind
template <int KIND>
constexpr int gp_nv() {
  return KIND == 0 ? 9 : KIND == 3 ? 1 : 3;
}

struct GpState {
  double lam, nu, cost, cost0, cost_new, model, rz[2], rr0, rr, pcg_tol, ftol;
  uint32_t steps_tried, steps_accepted, pcg_total, pcg_iter, pcg_stop, done_at, max_pcg, max_steps;
  uint32_t running, stop, take, zero_grad;
};

struct GpDev {
  uint32_t n, n_pairs, nb_view, n_heavy, n_part, root;
  const uint32_t *adj_off, *adj_nbr, *adj_pe, *heavy, *pairs;
  const double *relR, *relt;
  const uint8_t *use_t, *inc;
  const double *base;  // sfmloc.h "centres": the fixed baseline per pair; null in sfmloc_global_poses
  uint32_t *ntri, *nok;
  uint8_t *erot, *etr;
  double *R, *Rn, *C, *Cn;
  double *dir, *ev, *W, *ew, *rho, *res, *mterm;  // per pair: 3, 3, 9, 1, 1, 1, 1
  double *diag, *Minv, *x, *r, *z, *p, *q;        // per view: 9 each
  double *part;                                   // 3 x n_part partial sums
  GpState *st;
};

// ---- sums -------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ double gp_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}

// the sum over a workgroup of 256: the wave's butterfly, then the four waves in ascending order; every thread gets it
__device__ __forceinline__ double gp_block_sum(double v, double *sh) {
  v = gp_wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

// "partials": thread-strided in ascending index, then the workgroup's tree
__device__ __forceinline__ double gp_sum(const double *p, uint32_t n, double *sh) {
  double a = 0.0;
  for (uint32_t i = threadIdx.x; i < n; i += 256) a += p[i];
  return gp_block_sum(a, sh);
}

// ---- gather -----------------------------------------------------------------------------------------------------------

// the view of this lane (workgroups [0, nb_view): one lane per view, the heavy views left out) or of this wave (the
// workgroups after them: four heavy views each); false: none.  `wave` is uniform over a workgroup.
__device__ __forceinline__ bool gp_pick(const GpDev &D, uint32_t *v, bool *wave) {
  if (blockIdx.x < D.nb_view) {
    *wave = false;
    *v = blockIdx.x * 256 + threadIdx.x;
    return *v < D.n && D.adj_off[*v + 1] - D.adj_off[*v] <= kWaveDegree;
  }
  *wave = true;
  const uint32_t w = (blockIdx.x - D.nb_view) * 4 + (threadIdx.x >> 6);
  if (w >= D.n_heavy) return false;
  *v = D.heavy[w];
  return true;
}

// acc += f over the adjacency entries of v in index order (a lane), or lane-strided and then through the butterfly (a
// wave: every lane ends with the sums).  f(entry, acc).
template <int N, class F>
__device__ __forceinline__ void gp_gather(const GpDev &D, uint32_t v, bool wave, double (&acc)[N], F f) {
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  const uint32_t b = D.adj_off[v], e = D.adj_off[v + 1];
  if (!wave) {
    for (uint32_t t = b; t < e; ++t) f(t, acc);
  } else {
    for (uint32_t t = b + (threadIdx.x & 63); t < e; t += 64) f(t, acc);
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] = gp_wave_sum(acc[i]);
  }
}

// the lane that owns the view's result
__device__ __forceinline__ bool gp_owner(bool wave) { return !wave || (threadIdx.x & 63) == 0; }

__device__ __forceinline__ bool gp_active(const GpDev &D, uint32_t v) { return D.inc[v] && v != D.root; }

// ---- small matrices, row-major ---------------------------------------------------------------------------------------

// C = A B, or A^T B
__device__ __forceinline__ void gp_mul(const double *A, bool transpose, const double *B, double *C) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int c = 0; c < 3; ++c)
      C[3 * a + c] = transpose ? (A[a] * B[c] + A[3 + a] * B[3 + c]) + A[6 + a] * B[6 + c]
                               : (A[3 * a] * B[c] + A[3 * a + 1] * B[3 + c]) + A[3 * a + 2] * B[6 + c];
}

// y = A x, or A^T x
__device__ __forceinline__ void gp_mulv(const double *A, bool transpose, const double *x, double *y) {
#pragma unroll
  for (int a = 0; a < 3; ++a)
    y[a] = transpose ? (A[a] * x[0] + A[3 + a] * x[1]) + A[6 + a] * x[2]
                     : (A[3 * a] * x[0] + A[3 * a + 1] * x[1]) + A[3 * a + 2] * x[2];
}

__device__ __forceinline__ double gp_det(const double *M) {
  return (M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6])) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// the inverse of a symmetric positive definite 3 x 3 block by cofactors
__device__ __forceinline__ void gp_inv_sym(const double *A, double *I) {
  const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
  const double det = (A[0] * c00 + A[1] * c01) + A[2] * c02;
  const double c11 = A[0] * A[8] - A[2] * A[6], c12 = A[1] * A[6] - A[0] * A[7], c22 = A[0] * A[4] - A[1] * A[3];
  I[0] = c00 / det;
  I[1] = I[3] = c01 / det;
  I[2] = I[6] = c02 / det;
  I[4] = c11 / det;
  I[5] = I[7] = c12 / det;
  I[8] = c22 / det;
}

// ---- sfmloc.h "triplets" ---------------------------------------------------------------------------------------------

// rel_R of pair p as the rotation from view x (to its other view)
__device__ __forceinline__ void gp_load_from(const GpDev &D, uint32_t p, uint32_t x, double *R) {
  const double *S = D.relR + 9 * (size_t)p;
  const bool tr = D.pairs[2 * (size_t)p] != x;
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) R[3 * a + b] = tr ? S[3 * b + a] : S[3 * a + b];
}

// one wave per pair: the entries of I's list looked up in J's
__global__ __launch_bounds__(256) void k_gp_triplets(GpDev D, double thr) {
  const uint32_t k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= D.n_pairs) return;
  const uint32_t I = D.pairs[2 * (size_t)k], J = D.pairs[2 * (size_t)k + 1];
  const uint32_t bI = D.adj_off[I], eI = D.adj_off[I + 1], bJ = D.adj_off[J], eJ = D.adj_off[J + 1];
  uint32_t nt = 0, no = 0;
  for (uint32_t t = bI + (threadIdx.x & 63); t < eI; t += 64) {
    const uint32_t w = D.adj_nbr[t];
    if (w == J) continue;
    uint32_t lo = bJ, hi = eJ;
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      if (D.adj_nbr[mid] < w) lo = mid + 1;
      else hi = mid;
    }
    if (lo >= eJ || D.adj_nbr[lo] != w) continue;
    const uint32_t kIw = D.adj_pe[t] & ~kDirBit, kJw = D.adj_pe[lo] & ~kDirBit;
    uint32_t a = I, b = J, c = w, s;
    if (a > b) s = a, a = b, b = s;
    if (b > c) s = b, b = c, c = s;
    if (a > b) s = a, a = b, b = s;
    auto pr = [&](uint32_t x, uint32_t y) { return (x != w && y != w) ? k : (x != J && y != J) ? kIw : kJw; };
    double Rab[9], Rbc[9], Rca[9], T[9];
    gp_load_from(D, pr(a, b), a, Rab);
    gp_load_from(D, pr(b, c), b, Rbc);
    gp_load_from(D, pr(c, a), c, Rca);
    gp_mul(Rbc, false, Rab, T);
    double tr = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) tr += (Rca[3 * i] * T[i] + Rca[3 * i + 1] * T[3 + i]) + Rca[3 * i + 2] * T[6 + i];
    ++nt;
    if (tr > thr) ++no;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {  // (a pair is one wave's: its counts need no atomic)
    nt += __shfl_xor(nt, o);
    no += __shfl_xor(no, o);
  }
  if ((threadIdx.x & 63) == 0) {
    D.ntri[k] = nt;
    D.nok[k] = no;
  }
}

// ---- sfmloc.h "component" --------------------------------------------------------------------------------------------

// the edge list of graph_device.h: a pair that is not kept or carries no translation joins a view to itself
__global__ __launch_bounds__(256) void k_gp_cc_edges(GpDev D, uint32_t *ea, uint32_t *eb, uint32_t *parent) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.n) parent[i] = i;
  if (i >= D.n_pairs) return;
  const uint32_t I = D.pairs[2 * (size_t)i];
  ea[i] = I;
  eb[i] = (D.nok[i] > 0 && D.use_t[i]) ? D.pairs[2 * (size_t)i + 1] : I;
}

__global__ __launch_bounds__(256) void k_gp_flags(GpDev D) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= D.n_pairs) return;
  const uint8_t rot = D.nok[k] > 0 && D.inc[D.pairs[2 * (size_t)k]] && D.inc[D.pairs[2 * (size_t)k + 1]];
  D.erot[k] = rot;
  D.etr[k] = rot && D.use_t[k];
}

// ---- the systems: setup ----------------------------------------------------------------------------------------------

// r = b, z = M^-1 r, p = z, x = 0 for an active view (zeros for every other), and the view's part of r.z and r.r
template <int NV>
__device__ __forceinline__ void gp_start(const GpDev &D, uint32_t v, bool active, const double *b, const double *z,
                                         double *rz, double *rr) {
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const size_t o = NV * (size_t)v + i;
    const double bi = active ? b[i] : 0.0, zi = active ? z[i] : 0.0;
    D.x[o] = 0.0;
    D.q[o] = 0.0;
    D.r[o] = bi;
    D.z[o] = zi;
    D.p[o] = zi;
    *rz += bi * zi;
    *rr += bi * bi;
  }
}

// KIND 0 "chordal", 1 "IRLS" (after k_gp_rot_edges), 2 "translation" (after k_gp_tr_edges), 3 "scales" (after
// k_gp_sc_edges): the view's diagonal, its
// preconditioner and right-hand side; partials: r.z, r.r, and the cost over the pairs to a larger neighbour
template <int KIND>
__global__ __launch_bounds__(256) void k_gp_setup(GpDev D) {
  __shared__ double sh[4];
  constexpr int NV = gp_nv<KIND>();
  uint32_t v = 0;
  bool wave = false;
  const bool have = gp_pick(D, &v, &wave);
  double rz = 0.0, rr = 0.0, cost = 0.0;
  if (have) {
    const bool active = gp_active(D, v);
    double b[NV], z[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) b[i] = z[i] = 0.0;
    if constexpr (KIND == 0) if (active) {
      double acc[10];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[10]) {
        const uint32_t pe = D.adj_pe[t], k = pe & ~kDirBit;
        if (!D.erot[k]) return;
        a[9] += 1.0;
        if (D.adj_nbr[t] != D.root) return;
        const double *S = D.relR + 9 * (size_t)k;
        const bool tr = !(pe & kDirBit);
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
          for (int j = 0; j < 3; ++j) a[3 * i + j] += tr ? S[3 * j + i] : S[3 * i + j];
      });
#pragma unroll
      for (int i = 0; i < 9; ++i) {
        b[i] = acc[i];
        z[i] = acc[i] / acc[9];
      }
      if (gp_owner(wave)) D.diag[v] = acc[9];
    }
    if constexpr (KIND == 1) if (active) {
      double acc[5];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[5]) {
        const uint32_t pe = D.adj_pe[t], k = pe & ~kDirBit;
        if (!D.erot[k]) return;
        a[3] += D.ew[k];
        const double sg = (pe & kDirBit) ? 1.0 : -1.0;
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] += sg * D.ev[3 * (size_t)k + i];
        if (D.adj_nbr[t] > v) a[4] += D.rho[k];
      });
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        b[i] = acc[i];
        z[i] = acc[3] > 0.0 ? acc[i] / acc[3] : 0.0;
      }
      if (gp_owner(wave)) D.diag[v] = acc[3];
      cost = acc[4];
    }
    if constexpr (KIND == 3) if (active) {
      double acc[3];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[3]) {
        const uint32_t pe = D.adj_pe[t], k = pe & ~kDirBit;
        if (!D.erot[k]) return;
        a[1] += D.ew[k];
        a[0] += ((pe & kDirBit) ? -1.0 : 1.0) * D.ev[k];  // b = -gradient: - in l's row, + in k's
        if (D.adj_nbr[t] > v) a[2] += D.rho[k];
      });
      b[0] = acc[0];
      z[0] = acc[1] > 0.0 ? acc[0] / acc[1] : 0.0;
      if (gp_owner(wave)) D.diag[v] = acc[1];
      cost = acc[2];
    }
    if constexpr (KIND == 1 || KIND == 3) if (!active && D.inc[v]) {  // (the root: only its share of the cost)
      double acc[1];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[1]) {
        const uint32_t k = D.adj_pe[t] & ~kDirBit;
        if (D.erot[k] && D.adj_nbr[t] > v) a[0] += D.rho[k];
      });
      cost = acc[0];
    }
    if constexpr (KIND == 2) if (active) {
      double acc[13];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[13]) {
        const uint32_t pe = D.adj_pe[t], k = pe & ~kDirBit;
        if (!D.etr[k]) return;
#pragma unroll
        for (int i = 0; i < 9; ++i) a[i] += D.W[9 * (size_t)k + i];
        const double sg = (pe & kDirBit) ? -1.0 : 1.0;  // b = -gradient
#pragma unroll
        for (int i = 0; i < 3; ++i) a[9 + i] += sg * D.ev[3 * (size_t)k + i];
        if (D.adj_nbr[t] > v) a[12] += D.rho[k];
      });
      const double lam = D.st->lam;
      double A[9], Mi[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) A[i] = acc[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) A[4 * i] += lam * fmin(fmax(acc[4 * i], 1e-6), 1e32);
      gp_inv_sym(A, Mi);
#pragma unroll
      for (int i = 0; i < 3; ++i) b[i] = acc[9 + i];
      gp_mulv(Mi, false, b, z);
      if (gp_owner(wave)) {
#pragma unroll
        for (int i = 0; i < 9; ++i) {
          D.diag[9 * (size_t)v + i] = A[i];
          D.Minv[9 * (size_t)v + i] = Mi[i];
        }
      }
      cost = acc[12];
    }
    if constexpr (KIND == 2) if (!active && D.inc[v]) {
      double acc[1];
      gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[1]) {
        const uint32_t k = D.adj_pe[t] & ~kDirBit;
        if (D.etr[k] && D.adj_nbr[t] > v) a[0] += D.rho[k];
      });
      cost = acc[0];
    }
    if (gp_owner(wave)) gp_start<NV>(D, v, active, b, z, &rz, &rr);
    else cost = 0.0;
  }
  rz = gp_block_sum(rz, sh);
  rr = gp_block_sum(rr, sh);
  cost = gp_block_sum(cost, sh);
  if (threadIdx.x == 0) {
    D.part[blockIdx.x] = rz;
    D.part[D.n_part + blockIdx.x] = rr;
    D.part[2 * D.n_part + blockIdx.x] = cost;
  }
}

// one workgroup: the solve's starting scalars, and with_cost the cost of the state the system was set up at
__global__ __launch_bounds__(256) void k_gp_begin(GpDev D, int with_cost) {
  __shared__ double sh[4];
  const double rz = gp_sum(D.part, D.n_part, sh);
  const double rr = gp_sum(D.part + D.n_part, D.n_part, sh);
  const double cost = gp_sum(D.part + 2 * D.n_part, D.n_part, sh);
  if (threadIdx.x != 0) return;
  GpState *st = D.st;
  st->rz[0] = rz;
  st->rr0 = rr;
  st->rr = rr;
  st->pcg_iter = 0;
  st->pcg_stop = 0;
  st->zero_grad = !(rr > 0.0);
  st->done_at = (rr > 0.0 && rz > 0.0) ? kNever : 0u;
  if (with_cost) {
    if (st->steps_tried == 0) st->cost0 = cost;
    st->cost = cost;
  }
}

// ---- sfmloc.h "PCG" --------------------------------------------------------------------------------------------------

// q = A p per view, and the workgroup's part of p.q
template <int KIND>
__global__ __launch_bounds__(256) void k_gp_apply(GpDev D, uint32_t it) {
  __shared__ double sh[4];
  if (D.st->done_at <= it) return;
  constexpr int NV = gp_nv<KIND>();
  uint32_t v = 0;
  bool wave = false;
  double pq = 0.0;
  if (gp_pick(D, &v, &wave) && gp_active(D, v)) {
    double acc[NV];
    gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[NV]) {
      const uint32_t pe = D.adj_pe[t], k = pe & ~kDirBit;
      if (!(KIND == 2 ? D.etr[k] : D.erot[k])) return;
      const double *pn = D.p + NV * (size_t)D.adj_nbr[t];
      if constexpr (KIND == 0) {
        double y[9];
        gp_mul(D.relR + 9 * (size_t)k, !(pe & kDirBit), pn, y);
#pragma unroll
        for (int i = 0; i < 9; ++i) a[i] += y[i];
      } else if constexpr (KIND == 1 || KIND == 3) {
        const double w = D.ew[k];
#pragma unroll
        for (int i = 0; i < NV; ++i) a[i] += w * pn[i];
      } else {
        double y[3];
        gp_mulv(D.W + 9 * (size_t)k, false, pn, y);
#pragma unroll
        for (int i = 0; i < 3; ++i) a[i] += y[i];
      }
    });
    if (gp_owner(wave)) {
      const double *pv = D.p + NV * (size_t)v;
      double dp[NV];
      if constexpr (KIND == 2) {
        gp_mulv(D.diag + 9 * (size_t)v, false, pv, dp);
      } else {
        const double dg = D.diag[v];
#pragma unroll
        for (int i = 0; i < NV; ++i) dp[i] = dg * pv[i];
      }
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const double qi = dp[i] - acc[i];
        D.q[NV * (size_t)v + i] = qi;
        pq += pv[i] * qi;
      }
    }
  }
  pq = gp_block_sum(pq, sh);
  if (threadIdx.x == 0) D.part[blockIdx.x] = pq;
}

// x += alpha p, r -= alpha q, z = M^-1 r, and the workgroup's parts of r.z and r.r (one lane per view)
template <int KIND>
__global__ __launch_bounds__(256) void k_gp_step1(GpDev D, uint32_t it) {
  __shared__ double sh[4];
  if (D.st->done_at <= it) return;
  constexpr int NV = gp_nv<KIND>();
  const double pq = gp_sum(D.part, D.n_part, sh);
  const double alpha = D.st->rz[it & 1] / pq;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  double rz = 0.0, rr = 0.0;
  if (pq > 0.0 && v < D.n && gp_active(D, v)) {
    double r[NV], z[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const size_t o = NV * (size_t)v + i;
      D.x[o] += alpha * D.p[o];
      r[i] = D.r[o] - alpha * D.q[o];
      D.r[o] = r[i];
    }
    if constexpr (KIND == 2) {
      gp_mulv(D.Minv + 9 * (size_t)v, false, r, z);
    } else {
      const double dg = D.diag[v];
#pragma unroll
      for (int i = 0; i < NV; ++i) z[i] = dg > 0.0 ? r[i] / dg : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      D.z[NV * (size_t)v + i] = z[i];
      rz += r[i] * z[i];
      rr += r[i] * r[i];
    }
  }
  rz = gp_block_sum(rz, sh);
  rr = gp_block_sum(rr, sh);
  if (threadIdx.x == 0) {
    D.part[D.n_part + blockIdx.x] = rz;
    D.part[2 * D.n_part + blockIdx.x] = rr;
  }
}

// p = z + beta p, and (the first workgroup) the stopping rule.  r.z alternates between two slots by the iteration's
// parity and done_at only ever becomes it + 1, so what the first workgroup writes is nothing a workgroup of this
// launch reads.
template <int KIND>
__global__ __launch_bounds__(256) void k_gp_step2(GpDev D, uint32_t it) {
  __shared__ double sh[4];
  GpState *st = D.st;
  if (st->done_at <= it) return;
  constexpr int NV = gp_nv<KIND>();
  const double pq = gp_sum(D.part, D.n_part, sh);
  const double rzn = gp_sum(D.part + D.n_part, D.nb_view, sh);
  const double rr = gp_sum(D.part + 2 * D.n_part, D.nb_view, sh);
  const double beta = rzn / st->rz[it & 1];
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (pq > 0.0 && v < D.n && gp_active(D, v)) {
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const size_t o = NV * (size_t)v + i;
      D.p[o] = D.z[o] + beta * D.p[o];
    }
  }
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (!(pq > 0.0)) {  // (the step was not taken)
    st->pcg_iter = it;
    st->pcg_stop = 2;
    st->done_at = it + 1;
    return;
  }
  st->rz[(it + 1) & 1] = rzn;
  st->rr = rr;
  st->pcg_iter = it + 1;
  const double tol = st->pcg_tol;
  if (!(rr > tol * tol * st->rr0)) {
    st->pcg_stop = 0;
    st->done_at = it + 1;
  } else if (!(rzn > 0.0)) {
    st->pcg_stop = 2;
    st->done_at = it + 1;
  } else if (it + 1 >= st->max_pcg) {
    st->pcg_stop = 1;
    st->done_at = it + 1;
  }
}

// ---- sfmloc.h "chordal": the projection ------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void k_gp_project(GpDev D) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= D.n) return;
  double R[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = (D.inc[v] && (i & 3) == 0) ? 1.0 : 0.0;  // the root's; outside: zeros
  if (gp_active(D, v)) {
    double X[9], S[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) X[i] = D.x[9 * (size_t)v + i];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[i][j] = (X[i] * X[j] + X[3 + i] * X[3 + j]) + X[6 + i] * X[6 + j];
    geom::jacobi_fixed<3>(S, V);
    int lo = 0;
    if (S[1][1] < S[lo][lo]) lo = 1;
    if (S[2][2] < S[lo][lo]) lo = 2;
    const bool flip = gp_det(X) < 0.0;
    double B[9];  // X V with column i scaled by s_i / sqrt(l_i)
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      const double sc = ((flip && i == lo) ? -1.0 : 1.0) / sqrt(S[i][i]);
#pragma unroll
      for (int a = 0; a < 3; ++a) B[3 * a + i] = ((X[3 * a] * V[0][i] + X[3 * a + 1] * V[1][i]) + X[3 * a + 2] * V[2][i]) * sc;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int c = 0; c < 3; ++c) R[3 * a + c] = (B[3 * a] * V[c][0] + B[3 * a + 1] * V[c][1]) + B[3 * a + 2] * V[c][2];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) D.R[9 * (size_t)v + i] = R[i];
#pragma unroll
  for (int i = 0; i < 3; ++i) D.C[3 * (size_t)v + i] = 0.0;
}

// ---- sfmloc.h "IRLS" and "translation": per pair ---------------------------------------------------------------------

// Huber in s with delta: the weight and the cost
__device__ __forceinline__ void gp_huber(double s, double delta, double *w, double *rho) {
  if (s <= delta) {
    *w = 1.0;
    *rho = 0.5 * s * s;
  } else {
    *w = delta / s;
    *rho = delta * (s - 0.5 * delta);
  }
}

// at the rotations Rs.  trial: only the cost is written (the linearisation of the step stays)
__global__ __launch_bounds__(256) void k_gp_rot_edges(GpDev D, const double *Rs, double delta, int trial) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= D.n_pairs) return;
  double g[3] = {0.0, 0.0, 0.0}, w = 0.0, rho = 0.0, s = 0.0, chord = 0.0;
  if (D.erot[k]) {
    const uint32_t I = D.pairs[2 * (size_t)k], J = D.pairs[2 * (size_t)k + 1];
    double T[9], E[9];
    gp_mul(D.relR + 9 * (size_t)k, false, Rs + 9 * (size_t)I, T);
    gp_mul(Rs + 9 * (size_t)J, true, T, E);
#pragma unroll
    for (int i = 0; i < 9; ++i) {  // sfmloc.h "chordal": the pair's |R_j - R_ij R_i|_F^2
      const double e = Rs[9 * (size_t)J + i] - T[i];
      chord += e * e;
    }
    const double den = 1.0 + ((E[0] + E[4]) + E[8]);
    if (den > 1e-12) {
      g[0] = (E[7] - E[5]) / den;
      g[1] = (E[2] - E[6]) / den;
      g[2] = (E[3] - E[1]) / den;
      s = sqrt((g[0] * g[0] + g[1] * g[1]) + g[2] * g[2]);
      gp_huber(s, delta, &w, &rho);
    }
  }
  D.rho[k] = rho;
  if (trial) return;
  D.ew[k] = w;
  D.res[k] = s;
  D.mterm[k] = chord;  // (k_gp_cost sums it beside the trial's cost: GpState::model of an IRLS step)
#pragma unroll
  for (int i = 0; i < 3; ++i) D.ev[3 * (size_t)k + i] = w * g[i];
}

__global__ __launch_bounds__(256) void k_gp_dirs(GpDev D) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= D.n_pairs) return;
  double d[3] = {0.0, 0.0, 0.0};
  if (D.etr[k]) {
    gp_mulv(D.R + 9 * (size_t)D.pairs[2 * (size_t)k + 1], true, D.relt + 3 * (size_t)k, d);
    const double nn = sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] = -d[i] / nn;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) D.dir[3 * (size_t)k + i] = d[i];
}

// at the centres Cs.  trial: the cost there, and the pair's part of the model decrease of the step x from the stored
// linearisation (which stays)
__global__ __launch_bounds__(256) void k_gp_tr_edges(GpDev D, const double *Cs, double delta, int trial) {
  const uint32_t k = blockIdx.x * 256 + threadIdx.x;
  if (k >= D.n_pairs) return;
  double r[3] = {0.0, 0.0, 0.0}, w = 0.0, rho = 0.0, nr = 0.0, s = 0.0, m = 0.0;
  const double *d = D.dir + 3 * (size_t)k;
  const bool on = D.etr[k];
  if (on) {
    const uint32_t I = D.pairs[2 * (size_t)k], J = D.pairs[2 * (size_t)k + 1];
    double dl[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) dl[i] = Cs[3 * (size_t)J + i] - Cs[3 * (size_t)I + i];
    s = (d[0] * dl[0] + d[1] * dl[1]) + d[2] * dl[2];
    const double sc = D.base ? D.base[k] : (s > 1.0 ? s : 1.0);  // sfmloc.h "centres": the baseline is given
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = dl[i] - sc * d[i];
    nr = sqrt((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    gp_huber(nr, delta, &w, &rho);
    if (trial) {
      double u[3], Wu[3];
#pragma unroll
      for (int i = 0; i < 3; ++i) u[i] = D.x[3 * (size_t)J + i] - D.x[3 * (size_t)I + i];
      gp_mulv(D.W + 9 * (size_t)k, false, u, Wu);
      const double *ev = D.ev + 3 * (size_t)k;
      m = -((ev[0] * u[0] + ev[1] * u[1]) + ev[2] * u[2]) - 0.5 * ((u[0] * Wu[0] + u[1] * Wu[1]) + u[2] * Wu[2]);
    }
  }
  D.rho[k] = rho;
  D.mterm[k] = m;
  if (trial) return;
  D.res[k] = nr;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    D.ev[3 * (size_t)k + i] = w * r[i];
#pragma unroll
    for (int j = 0; j < 3; ++j)
      D.W[9 * (size_t)k + 3 * i + j] = on ? w * ((i == j ? 1.0 : 0.0) - ((!D.base && s > 1.0) ? d[i] * d[j] : 0.0)) : 0.0;
  }
}

// sfmloc.h "scales": per wedge (the "pairs" of this GpDev; its "views" are the pairs k, l) at the log scales xs, y = the
// log ratios.  trial: only the cost is written
__global__ __launch_bounds__(256) void k_gp_sc_edges(GpDev D, const double *xs, const double *y, double delta, int trial) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= D.n_pairs) return;
  double r = 0.0, w = 0.0, rho = 0.0, s = 0.0;
  if (D.erot[e]) {
    r = (xs[D.pairs[2 * (size_t)e + 1]] - xs[D.pairs[2 * (size_t)e]]) - y[e];
    s = r < 0.0 ? -r : r;
    gp_huber(s, delta, &w, &rho);
  }
  D.rho[e] = rho;
  if (trial) return;
  D.ew[e] = w;
  D.res[e] = s;
  D.mterm[e] = 0.0;
  D.ev[e] = w * r;
}

// parent[i] = i over the pairs; the edge list of graph_device.h over the wedges: one that is not used joins k to itself
__global__ __launch_bounds__(256) void k_gp_sc_cc(const uint32_t *kl, const uint8_t *on, uint32_t n_wedges, uint32_t n_pairs,
                                                  uint32_t *ea, uint32_t *eb, uint32_t *parent) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_pairs) parent[i] = i;
  if (i >= n_wedges) return;
  ea[i] = kl[2 * (size_t)i];
  eb[i] = on[i] ? kl[2 * (size_t)i + 1] : kl[2 * (size_t)i];
}

// ---- a step: trial, cost, decision, commit ---------------------------------------------------------------------------

// kind 1: Rn = R Cayley(x); kind 2: Cn = C + x; kind 3: the same on one value per node
__global__ __launch_bounds__(256) void k_gp_trial(GpDev D, int kind) {
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= D.n) return;
  const bool active = gp_active(D, v);
  if (kind == 3) {
    D.Cn[v] = active ? D.C[v] + D.x[v] : D.C[v];
    return;
  }
  const double *x = D.x + 3 * (size_t)v;
  if (kind == 2) {
#pragma unroll
    for (int i = 0; i < 3; ++i) D.Cn[3 * (size_t)v + i] = active ? D.C[3 * (size_t)v + i] + x[i] : D.C[3 * (size_t)v + i];
    return;
  }
  double R[9], Rn[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) Rn[i] = R[i] = D.R[9 * (size_t)v + i];
  if (active) {
    const double xx = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2], f = 2.0 / (1.0 + xx);
    const double K[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    double M[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        M[3 * i + j] = (i == j ? 1.0 : 0.0) + f * (K[3 * i + j] + (x[i] * x[j] - (i == j ? xx : 0.0)));
    gp_mul(R, false, M, Rn);
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) D.Rn[9 * (size_t)v + i] = Rn[i];
}

// per view over the pairs to a larger neighbour: the cost at the trial point and the model decrease
__global__ __launch_bounds__(256) void k_gp_cost(GpDev D, int kind) {
  __shared__ double sh[4];
  uint32_t v = 0;
  bool wave = false;
  double cost = 0.0, model = 0.0;
  if (gp_pick(D, &v, &wave) && D.inc[v]) {
    const uint8_t *on = kind == 2 ? D.etr : D.erot;
    double acc[2];
    gp_gather(D, v, wave, acc, [&](uint32_t t, double(&a)[2]) {
      const uint32_t k = D.adj_pe[t] & ~kDirBit;
      if (!on[k] || D.adj_nbr[t] <= v) return;
      a[0] += D.rho[k];
      a[1] += D.mterm[k];
    });
    if (gp_owner(wave)) {
      cost = acc[0];
      model = acc[1];
    }
  }
  cost = gp_block_sum(cost, sh);
  model = gp_block_sum(model, sh);
  if (threadIdx.x == 0) {
    D.part[blockIdx.x] = cost;
    D.part[D.n_part + blockIdx.x] = model;
  }
}

// one workgroup.  kind 1: sfmloc.h "IRLS"; kind 2: "solver" and "stopping" of the joint block
__global__ __launch_bounds__(256) void k_gp_decide(GpDev D, int kind) {
  __shared__ double sh[4];
  const double cn = gp_sum(D.part, D.n_part, sh);
  const double model = gp_sum(D.part + D.n_part, D.n_part, sh);
  if (threadIdx.x != 0) return;
  GpState *st = D.st;
  const double c = st->cost;
  st->cost_new = cn;
  st->model = model;
  ++st->steps_tried;
  st->pcg_total += st->pcg_iter;
  if (st->zero_grad || !(c > 0.0)) {  // (nothing to do at a stationary point)
    st->take = 0;
    st->stop = 0;
    st->running = 0;
    return;
  }
  if (kind == 1) {
    const bool ok = isfinite(cn) && cn < c;
    st->take = ok;
    if (ok) {
      ++st->steps_accepted;
      st->cost = cn;
      if ((c - cn) <= st->ftol * c) {
        st->stop = 0;
        st->running = 0;
      }
    } else {
      st->stop = 2;
      st->running = 0;
    }
  } else {
    const bool ok = isfinite(cn) && isfinite(model) && model > 0.0 && cn < c && (c - cn) / model > 1e-3;
    st->take = ok;
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
      if (isfinite(model) && model > 0.0 && model <= st->ftol * c) {
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
  }
  if (st->running && st->steps_tried >= st->max_steps) {
    st->stop = 1;
    st->running = 0;
  }
}

__global__ __launch_bounds__(256) void k_gp_commit(GpDev D, int kind) {
  if (!D.st->take) return;
  const uint32_t v = blockIdx.x * 256 + threadIdx.x;
  if (v >= D.n) return;
  if (kind == 3) {
    D.C[v] = D.Cn[v];
  } else if (kind == 2) {
#pragma unroll
    for (int i = 0; i < 3; ++i) D.C[3 * (size_t)v + i] = D.Cn[3 * (size_t)v + i];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) D.R[9 * (size_t)v + i] = D.Rn[9 * (size_t)v + i];
  }
}

// ---- host ------------------------------------------------------------------------------------------------------------


// a launch of 256-thread blocks, counted
template <class... Ts, class... As>
int gp_launch(uint32_t *launches, void (*kernel)(Ts...), uint32_t grid, LaunchStream on, As &&...as) {
  ++*launches;
  return dev_launch(kernel, dim3(grid), dim3(256), 0, on, as...);
}

int gp_read_state(const GpDev &D, GpState *h, hipStream_t s) {
  SFM_RC(dev_download(h, D.st, 1, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

// the queued iterations of one solve; *h = the state record where it stopped
template <int KIND>
int gp_pcg(const GpDev &D, uint32_t max_pcg, hipStream_t s, uint32_t *launches, GpState *h) {
  const uint32_t gv = D.nb_view, ga = D.n_part;
  for (uint32_t it = 0; it < max_pcg; it += kPcgChunk) {
    for (uint32_t k = it; k < it + kPcgChunk && k < max_pcg; ++k) {
      SFM_RC(gp_launch(launches, k_gp_apply<KIND>, ga, s, D, k));
      SFM_RC(gp_launch(launches, k_gp_step1<KIND>, gv, s, D, k));
      SFM_RC(gp_launch(launches, k_gp_step2<KIND>, gv, s, D, k));
    }
    SFM_RC(gp_read_state(D, h, s));
    if (h->done_at != kNever) break;
  }
  return SFMLOC_OK;
}

// the events at the phase boundaries of a call
struct GpEvents {
  Event e[5];
  int mark(int i, hipStream_t s) {
    SFM_RC(e[i].ensure(kTimingEvent));
    SFM_HIP(hipEventRecord(e[i], s));
    return SFMLOC_OK;
  }
  int between(int i, double *ms) { return span(i, i + 1, ms); }
  int span(int i, int j, double *ms) {  // (after the stream has been synchronised)
    float f = 0.f;
    SFM_HIP(hipEventElapsedTime(&f, e[i], e[j]));
    *ms = f;
    return SFMLOC_OK;
  }
};

GpState gp_state0(const sfmloc_gposes_options &o) {
  GpState st;
  memset(&st, 0, sizeof st);
  st.lam = 1e-4;
  st.nu = 2.0;
  st.pcg_tol = o.pcg_tolerance;
  st.ftol = o.function_tolerance;
  st.max_pcg = o.max_pcg;
  st.max_steps = o.max_steps;
  st.running = 1;
  st.done_at = kNever;
  return st;
}

// sfmloc.h "Scaled global poses": "scale graph" and "scales", after the rotations.  On return the translation pairs
// (g->pairs[].used_t, *etr), the view component (g->in_comp, the report) and D.inc / D.etr / D.root / D.base are those of
// the centres; *none: no wedge is used, nothing follows.
int gp_scale_phase(GpDev &D, uint8_t *d_inc, DevBuf<double> &d_base, const GpScaleIn &sc, const uint32_t *pairs,
                   hipStream_t s, uint32_t *launches, Gposes *g, std::vector<uint8_t> *etr, bool *none) {
  sfmloc_gposes_report &rep = g->rep;
  sfmloc_gpscale_report &sr = g->srep;
  const size_t P = D.n_pairs, n = D.n, W = sc.n_wedges;
  const uint32_t launches0 = *launches;
  std::vector<uint8_t> on(W ? W : 1, 0);
  std::vector<double> y(W ? W : 1, 0.0);
  for (size_t w = 0; w < W; ++w) {
    const double q = sc.ratio[w];
    on[w] = g->pairs[sc.kl[2 * w]].used_t && g->pairs[sc.kl[2 * w + 1]].used_t && isfinite(q) && q > 0.0;
    if (on[w]) y[w] = log(q);
    sr.n_wedges_used += on[w];
  }
  DevBuf<uint32_t> d_kl;
  DevBuf<uint8_t> d_on;
  uint32_t first = 0, size = 0;
  if (sr.n_wedges_used) {
    DevBuf<uint32_t> d_ea, d_eb, d_parent, d_flag;
    SFM_RC(dev_upload(nullptr, d_kl, sc.kl, 2 * W, s));
    SFM_RC(dev_upload(nullptr, d_on, on.data(), W, s));
    SFM_RC(d_ea.alloc(nullptr, W));
    SFM_RC(d_eb.alloc(nullptr, W));
    SFM_RC(d_parent.alloc(nullptr, P));
    SFM_RC(d_flag.alloc(nullptr, 1));
    const uint32_t gw = (uint32_t)((W + 255) / 256), gn = (uint32_t)((P + 255) / 256);
    SFM_RC(gp_launch(launches, k_gp_sc_cc, gw > gn ? gw : gn, s, d_kl, d_on, (uint32_t)W, (uint32_t)P, d_ea, d_eb,
                     d_parent));
    for (;;) {
      SFM_RC(d_flag.zero(1, s));
      SFM_RC(gp_launch(launches, k_graph_hook, gw, s, d_ea, d_eb, (uint32_t)W, d_parent, d_flag));
      SFM_RC(gp_launch(launches, k_graph_jump, gn, s, d_parent, (uint32_t)P));
      uint32_t changed = 0;
      SFM_RC(d_flag.download(&changed, 1, s));
      SFM_HIP(hipStreamSynchronize(s));
      if (!changed) break;
    }
    std::vector<uint32_t> label(P);
    SFM_RC(d_parent.download(label.data(), P, s));
    SFM_HIP(hipStreamSynchronize(s));
    gposes_host::pick_component(label, &first, &size);
    etr->assign(P, 0);
    if (size >= 2)
      for (size_t k = 0; k < P; ++k) (*etr)[k] = label[k] == first;
  }
  g->in_comp.assign(n, 0);
  rep.n_translation_pairs = rep.n_component_views = rep.root = 0;
  if (size < 2) {
    for (size_t k = 0; k < P; ++k) g->pairs[k].used_t = 0;
    sr.launches = *launches - launches0;
    *none = true;
    return SFMLOC_OK;
  }
  for (size_t k = 0; k < P; ++k) {
    g->pairs[k].used_t = (*etr)[k];
    if ((*etr)[k]) g->in_comp[pairs[2 * k]] = g->in_comp[pairs[2 * k + 1]] = 1;
  }
  uint32_t root = 0;
  for (size_t v = n; v-- > 0;)
    if (g->in_comp[v]) {
      ++rep.n_component_views;
      root = (uint32_t)v;
    }
  rep.root = root;
  rep.n_translation_pairs = sr.n_scaled_pairs = size;
  sr.n_scaled_views = rep.n_component_views;
  sr.first_pair = first;

  // "scales": the GpDev whose views are the pairs and whose pairs are the wedges
  for (size_t w = 0; w < W; ++w) on[w] = on[w] && (*etr)[sc.kl[2 * w]];
  wscales_host::ScaleGraph sg;
  wscales_host::scale_adjacency((uint32_t)P, sc.kl, on.data(), (uint32_t)W, &sg);
  GpDev S;
  memset(&S, 0, sizeof S);
  S.n = (uint32_t)P;
  S.n_pairs = (uint32_t)W;
  S.nb_view = (uint32_t)((P + 255) / 256);
  S.n_heavy = (uint32_t)sg.heavy.size();
  S.n_part = S.nb_view + (S.n_heavy + 3) / 4;
  S.root = first;
  DevBuf<uint32_t> d_off, d_nbr, d_pe, d_heavy;
  DevBuf<uint8_t> d_sinc;
  DevBuf<double> d_y, d_ev, d_ew, d_rho, d_res, d_mterm, d_diag, d_x, d_r, d_z, d_p, d_q, d_xs, d_xn, d_part;
  SFM_RC(dev_upload(nullptr, d_off, sg.off.data(), P + 1, s));
  SFM_RC(dev_upload(nullptr, d_nbr, sg.nbr.data(), sg.nbr.size(), s));
  SFM_RC(dev_upload(nullptr, d_pe, sg.pe.data(), sg.pe.size(), s));
  SFM_RC(dev_upload(nullptr, d_heavy, sg.heavy.data(), sg.heavy.size(), s, 1));
  SFM_RC(dev_upload(nullptr, d_on, on.data(), W, s));
  SFM_RC(dev_upload(nullptr, d_sinc, etr->data(), P, s));
  SFM_RC(dev_upload(nullptr, d_y, y.data(), W, s));
  for (DevBuf<double> *b : {std::addressof(d_ev), std::addressof(d_ew), std::addressof(d_rho), std::addressof(d_res),
                            std::addressof(d_mterm)})
    SFM_RC(b->alloc(nullptr, W));
  for (DevBuf<double> *b : {std::addressof(d_diag), std::addressof(d_x), std::addressof(d_r), std::addressof(d_z),
                            std::addressof(d_p), std::addressof(d_q), std::addressof(d_xs), std::addressof(d_xn)})
    SFM_RC(b->alloc(nullptr, P));
  SFM_RC(d_part.alloc(nullptr, 3 * (size_t)S.n_part));
  SFM_RC(d_xs.zero(P, s));
  SFM_RC(d_xn.zero(P, s));
  SFM_RC(d_mterm.zero(W, s));
  S.adj_off = d_off, S.adj_nbr = d_nbr, S.adj_pe = d_pe, S.heavy = d_heavy, S.pairs = d_kl, S.inc = d_sinc, S.erot = d_on;
  S.C = d_xs, S.Cn = d_xn, S.ev = d_ev, S.ew = d_ew, S.rho = d_rho, S.res = d_res, S.mterm = d_mterm, S.diag = d_diag;
  S.x = d_x, S.r = d_r, S.z = d_z, S.p = d_p, S.q = d_q, S.part = d_part, S.st = D.st;
  sfmloc_gposes_options o{};
  o.function_tolerance = sc.opt.function_tolerance;
  o.pcg_tolerance = sc.opt.pcg_tolerance;
  o.max_steps = sc.opt.max_steps;
  o.max_pcg = sc.opt.max_pcg;
  GpState h = gp_state0(o);
  SFM_RC(dev_upload(S.st, &h, 1, s));
  SFM_HIP(hipStreamSynchronize(s));  // (h is reused below)
  const uint32_t ge = (uint32_t)((W + 255) / 256), gv = S.nb_view, ga = S.n_part;
  const double delta = sc.opt.scale_delta;
  while (h.running) {
    SFM_RC(gp_launch(launches, k_gp_sc_edges, ge, s, S, d_xs, d_y, delta, 0));
    SFM_RC(gp_launch(launches, k_gp_setup<3>, ga, s, S));
    SFM_RC(gp_launch(launches, k_gp_begin, 1, s, S, 1));
    SFM_RC(gp_pcg<3>(S, sc.opt.max_pcg, s, launches, &h));
    SFM_RC(gp_launch(launches, k_gp_trial, gv, s, S, 3));
    SFM_RC(gp_launch(launches, k_gp_sc_edges, ge, s, S, d_xn, d_y, delta, 1));
    SFM_RC(gp_launch(launches, k_gp_cost, ga, s, S, 1));
    SFM_RC(gp_launch(launches, k_gp_decide, 1, s, S, 1));
    SFM_RC(gp_launch(launches, k_gp_commit, gv, s, S, 3));
    SFM_RC(gp_read_state(S, &h, s));
  }
  SFM_RC(gp_launch(launches, k_gp_sc_edges, ge, s, S, d_xs, d_y, delta, 0));  // the weights at the result
  std::vector<double> x(P), ew(W);
  SFM_RC(d_xs.download(x.data(), P, s));
  SFM_RC(d_ew.download(ew.data(), W, s));
  SFM_HIP(hipStreamSynchronize(s));
  std::vector<double> bx;
  for (size_t k = 0; k < P; ++k)
    if ((*etr)[k]) bx.push_back(exp(x[k]));
  const double med = wscales_host::lower_median(bx);
  for (size_t k = 0; k < P; ++k) g->base[k] = (*etr)[k] ? exp(x[k]) / med : 0.0;
  for (size_t w = 0; w < W; ++w) g->wedge_w[w] = on[w] ? ew[w] : 0.0;
  sr.steps_tried = h.steps_tried;
  sr.steps_accepted = h.steps_accepted;
  sr.pcg_total = h.pcg_total;
  sr.stop = h.stop;
  sr.cost_initial = h.cost0;
  sr.cost_final = h.cost;
  sr.launches = *launches - launches0;
  // "centres": what the translation kernels read
  SFM_RC(dev_upload(nullptr, d_base, g->base.data(), P, s));
  SFM_RC(dev_upload(d_inc, g->in_comp.data(), n, s));
  SFM_RC(dev_upload(D.etr, etr->data(), P, s));
  SFM_HIP(hipStreamSynchronize(s));
  D.base = d_base;
  D.root = root;
  return SFMLOC_OK;
}

int gposes_device(uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R, const double *rel_t,
                  const uint8_t *use_t, const sfmloc_gposes_options &opt, const gposes_host::Adjacency &adj,
                  const GpScaleIn *sc, hipStream_t s, Gposes *g) {
  sfmloc_gposes_report &rep = g->rep;
  uint32_t *launches = &rep.launches;
  const size_t n = n_views, P = n_pairs;
  GpEvents ev;
  SFM_RC(ev.mark(0, s));
  std::vector<uint8_t> use(P, 1);
  if (use_t)
    for (size_t k = 0; k < P; ++k) use[k] = use_t[k] ? 1 : 0;
  DevBuf<uint32_t> d_off, d_nbr, d_pe, d_heavy, d_pairs, d_ntri, d_nok, d_ea, d_eb, d_parent, d_flag;
  DevBuf<double> d_relR, d_relt;
  DevBuf<uint8_t> d_use, d_inc, d_erot, d_etr;
  SFM_RC(dev_upload(nullptr, d_off, adj.off.data(), n + 1, s));
  SFM_RC(dev_upload(nullptr, d_nbr, adj.nbr.data(), 2 * P, s));
  SFM_RC(dev_upload(nullptr, d_pe, adj.pe.data(), 2 * P, s));
  SFM_RC(dev_upload(nullptr, d_heavy, adj.heavy.data(), adj.heavy.size(), s, 1));
  SFM_RC(dev_upload(nullptr, d_pairs, pairs, 2 * P, s));
  SFM_RC(dev_upload(nullptr, d_relR, rel_R, 9 * P, s));
  SFM_RC(dev_upload(nullptr, d_relt, rel_t, 3 * P, s));
  SFM_RC(dev_upload(nullptr, d_use, use.data(), P, s));
  SFM_RC(d_ntri.alloc(nullptr, P));
  SFM_RC(d_nok.alloc(nullptr, P));
  SFM_RC(d_ea.alloc(nullptr, P));
  SFM_RC(d_eb.alloc(nullptr, P));
  SFM_RC(d_parent.alloc(nullptr, n));
  SFM_RC(d_flag.alloc(nullptr, 1));
  SFM_RC(d_inc.alloc(nullptr, n));
  SFM_RC(d_erot.alloc(nullptr, P));
  SFM_RC(d_etr.alloc(nullptr, P));
  GpDev D;
  memset(&D, 0, sizeof D);
  D.n = n_views;
  D.n_pairs = n_pairs;
  D.nb_view = (n_views + 255) / 256;
  D.n_heavy = (uint32_t)adj.heavy.size();
  D.n_part = D.nb_view + (D.n_heavy + 3) / 4;
  D.adj_off = d_off;
  D.adj_nbr = d_nbr;
  D.adj_pe = d_pe;
  D.heavy = d_heavy;
  D.pairs = d_pairs;
  D.relR = d_relR;
  D.relt = d_relt;
  D.use_t = d_use;
  D.inc = d_inc;
  D.ntri = d_ntri;
  D.nok = d_nok;
  D.erot = d_erot;
  D.etr = d_etr;
  const uint32_t gp = (n_pairs + 255) / 256, gv = D.nb_view, ga = D.n_part;
  const uint32_t gboth = ((n_pairs > n_views ? n_pairs : n_views) + 255) / 256;

  // sfmloc.h "triplets"
  const double thr = 1.0 + 2.0 * cos(opt.triplet_angle_deg * (M_PI / 180.0));
  SFM_RC(gp_launch(launches, k_gp_triplets, (n_pairs + 3) / 4, s, D, thr));
  // sfmloc.h "component"
  SFM_RC(gp_launch(launches, k_gp_cc_edges, gboth, s, D, d_ea, d_eb, d_parent));
  for (;;) {
    SFM_RC(d_flag.zero(1, s));
    SFM_RC(gp_launch(launches, k_graph_hook, gp, s, d_ea, d_eb, n_pairs, d_parent, d_flag));
    SFM_RC(gp_launch(launches, k_graph_jump, gv, s, d_parent, n_views));
    uint32_t changed = 0;
    SFM_RC(d_flag.download(&changed, 1, s));
    SFM_HIP(hipStreamSynchronize(s));
    if (!changed) break;
  }
  std::vector<uint32_t> label(n), ntri(P), nok(P);
  SFM_RC(d_parent.download(label.data(), n, s));
  SFM_RC(d_ntri.download(ntri.data(), P, s));
  SFM_RC(d_nok.download(nok.data(), P, s));
  SFM_HIP(hipStreamSynchronize(s));
  uint32_t root = 0, size = 0;
  gposes_host::pick_component(label, &root, &size);
  uint64_t t_all = 0, t_ok = 0;
  for (size_t k = 0; k < P; ++k) {
    sfmloc_gposes_pair &o = g->pairs[k];
    o.n_triplets = ntri[k];
    o.n_triplets_ok = nok[k];
    o.kept = nok[k] > 0;
    t_all += ntri[k];
    t_ok += nok[k];
    rep.n_pairs_kept += o.kept;
  }
  rep.n_triplets = (uint32_t)(t_all / 3);  // (every triangle is met from its three pairs)
  rep.n_triplets_ok = (uint32_t)(t_ok / 3);
  if (size < 2) return SFMLOC_OK;  // no triplet passes: an empty component
  rep.n_component_views = size;
  rep.root = root;
  for (size_t v = 0; v < n; ++v) g->in_comp[v] = label[v] == root;
  for (size_t k = 0; k < P; ++k) {
    const bool rot = g->pairs[k].kept && g->in_comp[pairs[2 * k]] && g->in_comp[pairs[2 * k + 1]];
    g->pairs[k].used_t = rot && use[k];
    rep.n_rotation_pairs += rot;
    rep.n_translation_pairs += g->pairs[k].used_t;
  }
  D.root = root;
  SFM_RC(ev.mark(1, s));
  SFM_RC(d_inc.upload(g->in_comp.data(), n, s));
  SFM_RC(gp_launch(launches, k_gp_flags, gp, s, D));

  DevBuf<double> d_R, d_Rn, d_C, d_Cn, d_dir, d_ev, d_W, d_ew, d_rho, d_res, d_mterm, d_diag, d_Minv, d_x, d_r, d_z, d_p,
      d_q, d_part;
  DevBuf<GpState> d_st;
  SFM_RC(d_R.alloc(nullptr, 9 * n));
  SFM_RC(d_Rn.alloc(nullptr, 9 * n));
  SFM_RC(d_C.alloc(nullptr, 3 * n));
  SFM_RC(d_Cn.alloc(nullptr, 3 * n));
  SFM_RC(d_dir.alloc(nullptr, 3 * P));
  SFM_RC(d_ev.alloc(nullptr, 3 * P));
  SFM_RC(d_W.alloc(nullptr, 9 * P));
  SFM_RC(d_ew.alloc(nullptr, P));
  SFM_RC(d_rho.alloc(nullptr, P));
  SFM_RC(d_res.alloc(nullptr, P));
  SFM_RC(d_mterm.alloc(nullptr, P));
  SFM_RC(d_diag.alloc(nullptr, 9 * n));
  SFM_RC(d_Minv.alloc(nullptr, 9 * n));
  SFM_RC(d_x.alloc(nullptr, 9 * n));
  SFM_RC(d_r.alloc(nullptr, 9 * n));
  SFM_RC(d_z.alloc(nullptr, 9 * n));
  SFM_RC(d_p.alloc(nullptr, 9 * n));
  SFM_RC(d_q.alloc(nullptr, 9 * n));
  SFM_RC(d_part.alloc(nullptr, 3 * (size_t)D.n_part));
  SFM_RC(d_st.alloc(nullptr, 1));
  SFM_RC(d_mterm.zero(P, s));
  D.R = d_R, D.Rn = d_Rn, D.C = d_C, D.Cn = d_Cn, D.dir = d_dir, D.ev = d_ev, D.W = d_W, D.ew = d_ew, D.rho = d_rho;
  D.res = d_res, D.mterm = d_mterm, D.diag = d_diag, D.Minv = d_Minv, D.x = d_x, D.r = d_r, D.z = d_z, D.p = d_p, D.q = d_q;
  D.part = d_part, D.st = d_st;
  GpState h = gp_state0(opt), h0 = h;

  // sfmloc.h "chordal"
  SFM_RC(d_st.upload(&h0, 1, s));
  SFM_RC(gp_launch(launches, k_gp_setup<0>, ga, s, D));
  SFM_RC(gp_launch(launches, k_gp_begin, 1, s, D, 0));
  SFM_RC(gp_pcg<0>(D, opt.max_pcg, s, launches, &h));
  rep.chordal_pcg = h.pcg_iter;
  rep.chordal_stop = h.pcg_stop;
  rep.chordal_residual = h.rr0 > 0.0 ? sqrt(h.rr / h.rr0) : 0.0;
  SFM_RC(gp_launch(launches, k_gp_project, gv, s, D));

  // sfmloc.h "IRLS"
  const double rdelta = opt.rotation_delta > 0.0 ? opt.rotation_delta : tan(opt.triplet_angle_deg * (M_PI / 180.0) / 6.0);
  SFM_RC(d_st.upload(&h0, 1, s));
  h = h0;
  while (h.running) {
    SFM_RC(gp_launch(launches, k_gp_rot_edges, gp, s, D, d_R, rdelta, 0));
    SFM_RC(gp_launch(launches, k_gp_setup<1>, ga, s, D));
    SFM_RC(gp_launch(launches, k_gp_begin, 1, s, D, 1));
    SFM_RC(gp_pcg<1>(D, opt.max_pcg, s, launches, &h));
    SFM_RC(gp_launch(launches, k_gp_trial, gv, s, D, 1));
    SFM_RC(gp_launch(launches, k_gp_rot_edges, gp, s, D, d_Rn, rdelta, 1));
    SFM_RC(gp_launch(launches, k_gp_cost, ga, s, D, 1));
    SFM_RC(gp_launch(launches, k_gp_decide, 1, s, D, 1));
    SFM_RC(gp_launch(launches, k_gp_commit, gv, s, D, 1));
    SFM_RC(gp_read_state(D, &h, s));
    if (h.steps_tried == 1) rep.chordal_cost = h.model;  // (at the first step's start: the projected chordal solution)
  }
  SFM_RC(gp_launch(launches, k_gp_rot_edges, gp, s, D, d_R, rdelta, 0));  // the residuals at the result
  std::vector<double> res(P);
  SFM_RC(d_res.download(res.data(), P, s));
  SFM_HIP(hipStreamSynchronize(s));
  for (size_t k = 0; k < P; ++k) g->pairs[k].rot_residual = res[k];
  rep.rot_steps_tried = h.steps_tried;
  rep.rot_steps_accepted = h.steps_accepted;
  rep.rot_pcg_total = h.pcg_total;
  rep.rot_stop = h.stop;
  rep.rot_cost_initial = h.cost0;
  rep.rot_cost_final = h.cost;

  // sfmloc.h "translation"
  SFM_RC(ev.mark(2, s));
  DevBuf<double> d_base;
  std::vector<uint8_t> etr_scaled;
  if (sc) {
    bool none = false;
    SFM_RC(gp_scale_phase(D, d_inc.get(), d_base, *sc, pairs, s, launches, g, &etr_scaled, &none));
    if (none) return SFMLOC_OK;
    SFM_RC(ev.mark(4, s));
  }
  SFM_RC(gp_launch(launches, k_gp_dirs, gp, s, D));
  SFM_RC(d_st.upload(&h0, 1, s));
  h = h0;
  while (h.running) {
    SFM_RC(gp_launch(launches, k_gp_tr_edges, gp, s, D, d_C, opt.translation_delta, 0));
    SFM_RC(gp_launch(launches, k_gp_setup<2>, ga, s, D));
    SFM_RC(gp_launch(launches, k_gp_begin, 1, s, D, 1));
    SFM_RC(gp_pcg<2>(D, opt.max_pcg, s, launches, &h));
    SFM_RC(gp_launch(launches, k_gp_trial, gv, s, D, 2));
    SFM_RC(gp_launch(launches, k_gp_tr_edges, gp, s, D, d_Cn, opt.translation_delta, 1));
    SFM_RC(gp_launch(launches, k_gp_cost, ga, s, D, 2));
    SFM_RC(gp_launch(launches, k_gp_decide, 1, s, D, 2));
    SFM_RC(gp_launch(launches, k_gp_commit, gv, s, D, 2));
    SFM_RC(gp_read_state(D, &h, s));
  }
  SFM_RC(gp_launch(launches, k_gp_tr_edges, gp, s, D, d_C, opt.translation_delta, 0));
  SFM_RC(d_res.download(res.data(), P, s));
  SFM_RC(d_R.download(g->R.data(), 9 * n, s));
  SFM_RC(d_C.download(g->C.data(), 3 * n, s));
  SFM_RC(ev.mark(3, s));
  SFM_HIP(hipStreamSynchronize(s));
  SFM_RC(ev.between(0, &rep.graph_ms));
  SFM_RC(ev.between(1, &rep.rotation_ms));
  if (sc) {
    SFM_RC(ev.span(2, 4, &g->srep.scale_ms));
    SFM_RC(ev.span(4, 3, &rep.translation_ms));
    g->srep.centre_ms = rep.translation_ms;
    for (size_t v = 0; v < n; ++v)
      if (!g->in_comp[v])
        for (int i = 0; i < 9; ++i) g->R[9 * v + i] = 0.0;
  } else {
    SFM_RC(ev.between(2, &rep.translation_ms));
  }
  for (size_t k = 0; k < P; ++k) g->pairs[k].trans_residual = res[k];
  rep.trans_steps_tried = h.steps_tried;
  rep.trans_steps_accepted = h.steps_accepted;
  rep.trans_pcg_total = h.pcg_total;
  rep.trans_stop = h.stop;
  rep.trans_cost_initial = h.cost0;
  rep.trans_cost_final = h.cost;
  return SFMLOC_OK;
}

int gposes_impl(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R,
                const double *rel_t, const uint8_t *use_t, const sfmloc_gposes_options &opt, const GpScaleIn *sc, Gposes *g) {
  gposes_host::Adjacency adj;
  std::string err;
  int rc = gposes_host::check(n_views, pairs, n_pairs, rel_R, rel_t, &adj, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  if (sc) {
    rc = wscales_host::check_wedges(pairs, n_pairs, sc->kl, sc->ratio, sc->n_wedges, &err);
    SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
    SFM_CHECK(sc->opt.scale_delta > 0.0 && sc->opt.function_tolerance >= 0.0 && sc->opt.pcg_tolerance >= 0.0, SFMLOC_EINVAL,
              "sfmloc_global_poses_scaled: scale_delta or a tolerance is out of range");
    SFM_CHECK(sc->opt.max_pcg >= 1 && sc->opt.max_pcg <= (1u << 30), SFMLOC_EINVAL,
              "sfmloc_global_poses_scaled: max_pcg = %u", sc->opt.max_pcg);
  }
  SFM_CHECK(opt.triplet_angle_deg > 0.0 && opt.triplet_angle_deg < 180.0, SFMLOC_EINVAL,
            "sfmloc_global_poses: triplet_angle_deg must lie in (0, 180)");
  SFM_CHECK(opt.translation_delta > 0.0 && opt.function_tolerance >= 0.0 && opt.pcg_tolerance >= 0.0 &&
                opt.rotation_delta == opt.rotation_delta,
            SFMLOC_EINVAL, "sfmloc_global_poses: a tolerance or delta is out of range");
  SFM_CHECK(opt.max_pcg >= 1 && opt.max_pcg <= (1u << 30), SFMLOC_EINVAL, "sfmloc_global_poses: max_pcg = %u", opt.max_pcg);
  g->n_views = n_views;
  g->in_comp.assign(n_views, 0);
  g->R.assign(9 * (size_t)n_views, 0.0);
  g->C.assign(3 * (size_t)n_views, 0.0);
  g->pairs.assign(n_pairs, sfmloc_gposes_pair{});
  g->rep.n_views = n_views;
  g->rep.n_pairs = n_pairs;
  g->base.assign(n_pairs, 0.0);
  g->wedge_w.assign(sc ? sc->n_wedges : 0, 0.0);
  g->srep.n_wedges = sc ? sc->n_wedges : 0;
  SFM_RC(timed_call(device, &g_gposes_last_ms, n_pairs != 0 && n_views != 0, [&](hipStream_t s) {
    return gposes_device(n_views, pairs, n_pairs, rel_R, rel_t, use_t, opt, adj, sc, s, g);
  }));
  g->rep.device_ms = g_gposes_last_ms;
  if (!g->rep.n_component_views) {  // (what the device wrote for a component that does not exist)
    g->R.assign(9 * (size_t)n_views, 0.0);
    g->C.assign(3 * (size_t)n_views, 0.0);
  }
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_gposes_default_options(sfmloc_gposes_options *o) {
  if (!o) return;
  o->triplet_angle_deg = 5.0;
  o->rotation_delta = 0.0;
  o->translation_delta = 0.05;
  o->function_tolerance = 1e-6;
  o->pcg_tolerance = 1e-6;
  o->max_steps = 50;
  o->max_pcg = 20000;
}

void sfmloc_gpscale_default_options(sfmloc_gpscale_options *o) {
  if (!o) return;
  o->scale_delta = 0.1;
  o->function_tolerance = 1e-6;
  o->pcg_tolerance = 1e-6;
  o->max_steps = 50;
  o->max_pcg = 20000;
}

static int gposes_call(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R,
                       const double *rel_t, const uint8_t *use_t, const sfmloc_gposes_options *opt, const GpScaleIn *sc,
                       sfmloc_gposes **out) {
  const sfmloc_gposes_options o = options_or(opt, sfmloc_gposes_default_options);
  return make_handle<Gposes>("sfmloc_global_poses", out, [&](Gposes *g) {
    return gposes_impl(device, n_views, pairs, n_pairs, rel_R, rel_t, use_t, o, sc, g);
  });
}

int sfmloc_global_poses(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R,
                        const double *rel_t, const uint8_t *use_t, const sfmloc_gposes_options *opt, sfmloc_gposes **out) {
  return gposes_call(device, n_views, pairs, n_pairs, rel_R, rel_t, use_t, opt, nullptr, out);
}

int sfmloc_global_poses_scaled(int device, uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R,
                               const double *rel_t, const uint8_t *use_t, const sfmloc_gposes_options *opt,
                               const uint32_t *wedge_kl, const double *wedge_ratio, uint32_t n_wedges,
                               const sfmloc_gpscale_options *sopt, sfmloc_gposes **out) {
  GpScaleIn sc{wedge_kl, wedge_ratio, n_wedges, {}};
  if (sopt) sc.opt = *sopt;
  else sfmloc_gpscale_default_options(&sc.opt);
  return gposes_call(device, n_views, pairs, n_pairs, rel_R, rel_t, use_t, opt, &sc, out);
}

int sfmloc_gpscale_baselines(const sfmloc_gposes *gg, double *b) {
  SFM_CHECK(gg, SFMLOC_EINVAL, "sfmloc_gpscale_baselines: null handle");
  const Gposes *g = reinterpret_cast<const Gposes *>(gg);
  SFM_CHECK(b || g->base.empty(), SFMLOC_EINVAL, "sfmloc_gpscale_baselines: null argument");
  if (!g->base.empty()) memcpy(b, g->base.data(), g->base.size() * sizeof(double));
  return SFMLOC_OK;
}

int sfmloc_gpscale_weights(const sfmloc_gposes *gg, double *w) {
  SFM_CHECK(gg, SFMLOC_EINVAL, "sfmloc_gpscale_weights: null handle");
  const Gposes *g = reinterpret_cast<const Gposes *>(gg);
  SFM_CHECK(w || g->wedge_w.empty(), SFMLOC_EINVAL, "sfmloc_gpscale_weights: null argument");
  if (!g->wedge_w.empty()) memcpy(w, g->wedge_w.data(), g->wedge_w.size() * sizeof(double));
  return SFMLOC_OK;
}

int sfmloc_gpscale_report_read(const sfmloc_gposes *gg, sfmloc_gpscale_report *rep) {
  SFM_CHECK(gg && rep, SFMLOC_EINVAL, "sfmloc_gpscale_report_read: null argument");
  *rep = reinterpret_cast<const Gposes *>(gg)->srep;
  return SFMLOC_OK;
}

int sfmloc_gposes_views(const sfmloc_gposes *gg, uint8_t *in_component, double *R, double *C) {
  SFM_CHECK(gg, SFMLOC_EINVAL, "sfmloc_gposes_views: null handle");
  const Gposes *g = reinterpret_cast<const Gposes *>(gg);
  if (in_component && g->n_views) memcpy(in_component, g->in_comp.data(), g->in_comp.size());
  if (R && g->n_views) memcpy(R, g->R.data(), g->R.size() * sizeof(double));
  if (C && g->n_views) memcpy(C, g->C.data(), g->C.size() * sizeof(double));
  return SFMLOC_OK;
}

int sfmloc_gposes_pairs(const sfmloc_gposes *gg, sfmloc_gposes_pair *out) {
  SFM_CHECK(gg, SFMLOC_EINVAL, "sfmloc_gposes_pairs: null handle");
  const Gposes *g = reinterpret_cast<const Gposes *>(gg);
  SFM_CHECK(out || g->pairs.empty(), SFMLOC_EINVAL, "sfmloc_gposes_pairs: null argument");
  if (!g->pairs.empty()) memcpy(out, g->pairs.data(), g->pairs.size() * sizeof(sfmloc_gposes_pair));
  return SFMLOC_OK;
}

int sfmloc_gposes_report_read(const sfmloc_gposes *gg, sfmloc_gposes_report *rep) {
  SFM_CHECK(gg && rep, SFMLOC_EINVAL, "sfmloc_gposes_report_read: null argument");
  *rep = reinterpret_cast<const Gposes *>(gg)->rep;
  return SFMLOC_OK;
}

void sfmloc_gposes_destroy(sfmloc_gposes *g) { delete reinterpret_cast<Gposes *>(g); }

double sfmloc_gposes_last_ms(void) { return g_gposes_last_ms; }

}  // extern "C"
