// sfmloc_merge: the device half of mergeSfM.mergeModel (hulo_sfm/mergeSfM.py) -- the RANSAC over 3D-3D matches, the
// nearest-other-point median of the threshold functions and the map transform.  The semantics, the readings chosen and
// the order of every sum are stated in include/sfmloc.h ("sfmloc_merge"); tests/merge_np.py restates the arithmetic in
// NumPy and the GPU tests compare bits.
//
//   rounds    one lane per round: ac_sample<4>, a 4-point model in registers (12 doubles), then all n matches in tiles
//             staged in LDS as structure-of-arrays f64 (every lane reads the same address: broadcasts).  The lane's key
//             (count << 32 | 0xFFFFFFFF - round) is reduced over the wave and one integer atomicMax per wave goes to
//             global memory: the largest count wins, the lowest round on ties, whatever the launch geometry.
//   winner    the winning round's model again through the same code (same bits), then the inlier list by an ordered
//             compaction (ballots and wave counts: no atomic decides a position).
//   fit       the final model on the inliers: 256 strided partial sums and a pairwise tree, one workgroup.
//   median    all pairs in tiles, one lane per point; the median by a radix select on the bit patterns (integer
//             histograms).
// Solvers use + - * / sqrt only, with fixed iteration counts; the library is built with -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "geom_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint32_t kMergeBlock = 256;       // lanes (= rounds) per workgroup of the round kernel
constexpr uint32_t kMergeTile = 512;        // matches per LDS tile (48 B each), less when the device's LDS is smaller
constexpr uint32_t kMergeLaunchRounds = 1u << 20;  // rounds per launch when the caller leaves the choice (0)
constexpr uint32_t kMergeMaxN = 1u << 24;
constexpr uint32_t kNnTile = 1024;          // points per LDS tile of the all-pairs kernel (24 KB)

thread_local double g_merge_last_ms = 0.0;

// ---- solvers (sfmloc.h "jacobi", "similarity", "affine") ----------------------------------------------------------------

// (the cyclic Jacobi of sfmloc.h "jacobi" is geom::jacobi_fixed, geom_device.h: kJacobiSweeps sweeps)
using geom::jacobi_fixed;

__device__ __forceinline__ bool finite12(const double *m) {
  bool f = true;
#pragma unroll
  for (int i = 0; i < 12; ++i) f = f && geom::is_finite(m[i]);
  return f;
}

// Horn's closed form from the centred moments: S[i][j] = sum b0_i a0_j, saa = sum |a0|^2, sbb = sum |b0|^2 and the means.
// M = [s R | ma - s R mb], row major 3 x 4.
__device__ __forceinline__ bool solve_similarity(const double (&ma)[3], const double (&mb)[3], const double (&S)[3][3],
                                                 double saa, double sbb, double *M) {
  double N[4][4], V[4][4];
  N[0][0] = (S[0][0] + S[1][1]) + S[2][2];
  N[0][1] = S[1][2] - S[2][1];
  N[0][2] = S[2][0] - S[0][2];
  N[0][3] = S[0][1] - S[1][0];
  N[1][1] = (S[0][0] - S[1][1]) - S[2][2];
  N[1][2] = S[0][1] + S[1][0];
  N[1][3] = S[2][0] + S[0][2];
  N[2][2] = (S[1][1] - S[0][0]) - S[2][2];
  N[2][3] = S[1][2] + S[2][1];
  N[3][3] = (S[2][2] - S[0][0]) - S[1][1];
#pragma unroll
  for (int i = 1; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) N[i][j] = N[j][i];
  jacobi_fixed<4>(N, V);
  double best = N[0][0], q0 = V[0][0], q1 = V[1][0], q2 = V[2][0], q3 = V[3][0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {  // the largest eigenvalue, the first on ties
    const bool take = N[i][i] > best;
    best = take ? N[i][i] : best;
    q0 = take ? V[0][i] : q0;
    q1 = take ? V[1][i] : q1;
    q2 = take ? V[2][i] : q2;
    q3 = take ? V[3][i] : q3;
  }
  const double nq = sqrt(((q0 * q0 + q1 * q1) + q2 * q2) + q3 * q3);
  const double w = q0 / nq, x = q1 / nq, y = q2 / nq, z = q3 / nq;
  double R[3][3];
  R[0][0] = 1.0 - 2.0 * (y * y + z * z);
  R[0][1] = 2.0 * (x * y - w * z);
  R[0][2] = 2.0 * (x * z + w * y);
  R[1][0] = 2.0 * (x * y + w * z);
  R[1][1] = 1.0 - 2.0 * (x * x + z * z);
  R[1][2] = 2.0 * (y * z - w * x);
  R[2][0] = 2.0 * (x * z - w * y);
  R[2][1] = 2.0 * (y * z + w * x);
  R[2][2] = 1.0 - 2.0 * (x * x + y * y);
  const double sc = sqrt(saa / sbb);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double m0 = sc * R[i][0], m1 = sc * R[i][1], m2 = sc * R[i][2];
    M[4 * i] = m0;
    M[4 * i + 1] = m1;
    M[4 * i + 2] = m2;
    M[4 * i + 3] = ma[i] - ((m0 * mb[0] + m1 * mb[1]) + m2 * mb[2]);
  }
  return finite12(M);
}

// G X = H (4 x 4, three right-hand sides) by Gaussian elimination with partial pivoting: in column k the rows below are
// compared with row k in order and swapped when strictly larger in magnitude.  A zero pivot: false.
__device__ __forceinline__ bool gauss4(double (&G)[4][4], double (&H)[4][3], double (&X)[4][3]) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
#pragma unroll
    for (int r = k + 1; r < 4; ++r) {
      const bool sw = geom::dabs(G[r][k]) > geom::dabs(G[k][k]);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const double a = G[k][j], b = G[r][j];
        G[k][j] = sw ? b : a;
        G[r][j] = sw ? a : b;
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double a = H[k][c], b = H[r][c];
        H[k][c] = sw ? b : a;
        H[r][c] = sw ? a : b;
      }
    }
    const double piv = G[k][k];
    ok = ok && piv != 0.0;
#pragma unroll
    for (int r = k + 1; r < 4; ++r) {
      const double f = G[r][k] / piv;
#pragma unroll
      for (int j = k + 1; j < 4; ++j) G[r][j] = G[r][j] - f * G[k][j];
#pragma unroll
      for (int c = 0; c < 3; ++c) H[r][c] = H[r][c] - f * H[k][c];
    }
  }
#pragma unroll
  for (int k = 3; k >= 0; --k)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double acc = H[k][c];
#pragma unroll
      for (int j = k + 1; j < 4; ++j) acc = acc - G[k][j] * X[j][c];
      X[k][c] = acc / G[k][k];
    }
  return ok;
}

// s[0] / s[-1] of M[:, :3] < svd_ratio, the singular values as square roots of the eigenvalues of L^T L
__device__ __forceinline__ bool ratio_ok(const double *M, double svd_ratio) {
  double Cm[3][3], V[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = i; j < 3; ++j) {
      Cm[i][j] = (M[i] * M[j] + M[4 + i] * M[4 + j]) + M[8 + i] * M[8 + j];
      Cm[j][i] = Cm[i][j];
    }
  jacobi_fixed<3>(Cm, V);
  double emax = Cm[0][0], emin = Cm[0][0];
#pragma unroll
  for (int i = 1; i < 3; ++i) {
    emax = Cm[i][i] > emax ? Cm[i][i] : emax;
    emin = Cm[i][i] < emin ? Cm[i][i] : emin;
  }
  return sqrt(emax) / sqrt(emin) < svd_ratio;  // (a NaN or infinite ratio fails)
}

__device__ __forceinline__ void affine_from_X(const double (&X)[4][3], double *M) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) M[4 * i + j] = X[j][i];
}

// the model of one round: 4 distinct matches by ac_sample<4>, then the 4-point fit (sums over the sample in order)
template <int MODEL>
__device__ __forceinline__ bool round_model(const double *__restrict__ A, const double *__restrict__ B, uint32_t n,
                                            uint64_t seed, uint32_t stream, uint32_t round, double svd_ratio, double *M) {
  int32_t s[4];
  geom::ac_sample<4>(nullptr, (int)n, seed, geom::STAGE_MERGE, stream, round, s);
  double a[4][3], b[4][3];
  bool fin = true;
#pragma unroll
  for (int p = 0; p < 4; ++p)
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      a[p][c] = A[3 * (size_t)s[p] + c];
      b[p][c] = B[3 * (size_t)s[p] + c];
      fin = fin && geom::is_finite(a[p][c]) && geom::is_finite(b[p][c]);
    }
  bool ok;
  if (MODEL == SFMLOC_MERGE_AFFINE) {
    double G[4][4], H[4][3], X[4][3];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      G[p][0] = b[p][0];
      G[p][1] = b[p][1];
      G[p][2] = b[p][2];
      G[p][3] = 1.0;
      H[p][0] = a[p][0];
      H[p][1] = a[p][1];
      H[p][2] = a[p][2];
    }
    ok = gauss4(G, H, X);
    affine_from_X(X, M);
    ok = ok && finite12(M) && ratio_ok(M, svd_ratio);
  } else {
    double ma[3], mb[3], S[3][3], saa = 0.0, sbb = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ma[c] = (((a[0][c] + a[1][c]) + a[2][c]) + a[3][c]) / 4.0;
      mb[c] = (((b[0][c] + b[1][c]) + b[2][c]) + b[3][c]) / 4.0;
    }
#pragma unroll
    for (int p = 0; p < 4; ++p)
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        a[p][c] = a[p][c] - ma[c];
        b[p][c] = b[p][c] - mb[c];
      }
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        S[i][j] = ((b[0][i] * a[0][j] + b[1][i] * a[1][j]) + b[2][i] * a[2][j]) + b[3][i] * a[3][j];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      saa = saa + ((a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2]);
      sbb = sbb + ((b[p][0] * b[p][0] + b[p][1] * b[p][1]) + b[p][2] * b[p][2]);
    }
    ok = solve_similarity(ma, mb, S, saa, sbb, M);
  }
  return ok && fin;
}

// sfmloc.h "inlier": sqrt((dx dx + dy dy) + dz dz) < thres, d_i = (((m_i0 x0 + m_i1 x1) + m_i2 x2) + t_i) - a_i
__device__ __forceinline__ bool is_inlier(const double *M, double x0, double x1, double x2, double a0, double a1, double a2,
                                          double thres) {
  const double dx = (((M[0] * x0 + M[1] * x1) + M[2] * x2) + M[3]) - a0;
  const double dy = (((M[4] * x0 + M[5] * x1) + M[6] * x2) + M[7]) - a1;
  const double dz = (((M[8] * x0 + M[9] * x1) + M[10] * x2) + M[11]) - a2;
  return sqrt((dx * dx + dy * dy) + dz * dz) < thres;
}

// ---- kernels --------------------------------------------------------------------------------------------------------------

template <int MODEL>
__global__ __launch_bounds__(kMergeBlock) void k_merge_rounds(const double *__restrict__ A, const double *__restrict__ B,
                                                              uint32_t n, double thres, double svd_ratio, uint64_t seed,
                                                              uint32_t stream, uint32_t round0, uint32_t n_rounds,
                                                              uint32_t tile, unsigned long long *__restrict__ best) {
  extern __shared__ double sm[];  // [6][tile]: B x y z, A x y z
  const uint32_t local = blockIdx.x * kMergeBlock + threadIdx.x;
  const bool live = local < n_rounds;
  const uint32_t round = round0 + (live ? local : 0u);
  double M[12];
  bool ok = round_model<MODEL>(A, B, n, seed, stream, round, svd_ratio, M);
  ok = ok && live;
  uint32_t count = 0;
  for (uint32_t base = 0; base < n; base += tile) {
    const uint32_t m = n - base < tile ? n - base : tile;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < 3 * m; k += kMergeBlock) {  // (coalesced: element k of the [m][3] slabs)
      const uint32_t p = k / 3, c = k - 3 * p;
      sm[c * tile + p] = B[3 * (size_t)base + k];
      sm[(3 + c) * tile + p] = A[3 * (size_t)base + k];
    }
    __syncthreads();
    for (uint32_t j = 0; j < m; ++j)
      count += is_inlier(M, sm[j], sm[tile + j], sm[2 * tile + j], sm[3 * tile + j], sm[4 * tile + j], sm[5 * tile + j],
                         thres)
                   ? 1u
                   : 0u;
  }
  unsigned long long key = (ok && count > 0) ? (((unsigned long long)count << 32) | (unsigned long long)(0xFFFFFFFFu - round))
                                             : 0ull;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned long long o = __shfl_xor(key, off, 64);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0 && key != 0ull) atomicMax(best, key);
}

// the winning round's model again (same code, same bits) -> Mwin[12], info = {has winner, round, count}
template <int MODEL>
__global__ void k_merge_winner(const double *__restrict__ A, const double *__restrict__ B, uint32_t n, double svd_ratio,
                               uint64_t seed, uint32_t stream, const unsigned long long *__restrict__ best,
                               double *__restrict__ Mwin, uint32_t *__restrict__ info) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const unsigned long long key = *best;
  double M[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) M[i] = 0.0;
  uint32_t round = 0, count = 0, has = 0;
  if (key != 0ull) {
    round = 0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFull);
    count = (uint32_t)(key >> 32);
    has = 1;
    round_model<MODEL>(A, B, n, seed, stream, round, svd_ratio, M);
  }
  for (int i = 0; i < 12; ++i) Mwin[i] = M[i];
  info[0] = has;
  info[1] = round;
  info[2] = count;
}

// inlier mask of a model and the ascending index list: one workgroup walks the matches 1024 at a time, a match's place
// is the running total + the inliers of the lower lanes of its wave + the earlier waves' counts
__global__ __launch_bounds__(1024) void k_merge_inliers(const double *__restrict__ A, const double *__restrict__ B, uint32_t n,
                                                        const double *__restrict__ Mdev, const uint32_t *__restrict__ has,
                                                        double thres, uint32_t *__restrict__ idx, uint32_t *__restrict__ n_out) {
  __shared__ uint32_t wc[16];
  __shared__ uint32_t total;
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (has && *has == 0) {
    if (t == 0) *n_out = 0;
    return;
  }
  double M[12];
  for (int i = 0; i < 12; ++i) M[i] = Mdev[i];
  if (t == 0) total = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t i = base + t;
    bool in = false;
    if (i < n)
      in = is_inlier(M, B[3 * (size_t)i], B[3 * (size_t)i + 1], B[3 * (size_t)i + 2], A[3 * (size_t)i], A[3 * (size_t)i + 1],
                     A[3 * (size_t)i + 2], thres);
    const unsigned long long bal = __ballot(in);
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    if (lane == 0) wc[w] = (uint32_t)__popcll(bal);
    __syncthreads();
    uint32_t r = total + (uint32_t)__popcll(bal & below);
    for (uint32_t ww = 0; ww < w; ++ww) r += wc[ww];
    if (in) idx[r] = i;
    __syncthreads();
    if (t == 0) {
      uint32_t s = 0;
      for (int ww = 0; ww < 16; ++ww) s += wc[ww];
      total += s;
    }
    __syncthreads();
  }
  if (t == 0) *n_out = total;
}

// sums of K quantities over the workgroup: 256 strided partials per quantity, then a pairwise tree (128, 64, ... 1)
template <int K>
__device__ __forceinline__ void block_sums(double (&part)[K], double *lds) {
  const uint32_t t = threadIdx.x;
#pragma unroll 1
  for (int q = 0; q < K; ++q) {
    double v = 0.0;
#pragma unroll
    for (int k = 0; k < K; ++k) v = k == q ? part[k] : v;
    lds[t] = v;
    __syncthreads();
    for (uint32_t s = 128; s > 0; s >>= 1) {
      if (t < s) lds[t] = lds[t] + lds[t + s];
      __syncthreads();
    }
    v = lds[0];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) part[k] = k == q ? v : part[k];
  }
}

// the final model on the inlier set (sfmloc.h "final fit"): out[0..11] = M, ok[0] = 1 when a finite model exists
template <int MODEL>
__global__ __launch_bounds__(256) void k_merge_fit(const double *__restrict__ A, const double *__restrict__ B,
                                                   const uint32_t *__restrict__ idx, uint32_t m, double *__restrict__ out,
                                                   uint32_t *__restrict__ okp) {
  __shared__ double lds[256];
  const uint32_t t = threadIdx.x;
  double M[12];
  bool ok;
  if (MODEL == SFMLOC_MERGE_AFFINE) {
    double p[21];
#pragma unroll
    for (int k = 0; k < 21; ++k) p[k] = 0.0;
    for (uint32_t i = t; i < m; i += 256) {
      const size_t o = 3 * (size_t)idx[i];
      const double b0 = B[o], b1 = B[o + 1], b2 = B[o + 2], a0 = A[o], a1 = A[o + 1], a2 = A[o + 2];
      p[0] = p[0] + b0 * b0;
      p[1] = p[1] + b0 * b1;
      p[2] = p[2] + b0 * b2;
      p[3] = p[3] + b0;
      p[4] = p[4] + b1 * b1;
      p[5] = p[5] + b1 * b2;
      p[6] = p[6] + b1;
      p[7] = p[7] + b2 * b2;
      p[8] = p[8] + b2;
      p[9] = p[9] + b0 * a0;
      p[10] = p[10] + b0 * a1;
      p[11] = p[11] + b0 * a2;
      p[12] = p[12] + b1 * a0;
      p[13] = p[13] + b1 * a1;
      p[14] = p[14] + b1 * a2;
      p[15] = p[15] + b2 * a0;
      p[16] = p[16] + b2 * a1;
      p[17] = p[17] + b2 * a2;
      p[18] = p[18] + a0;
      p[19] = p[19] + a1;
      p[20] = p[20] + a2;
    }
    block_sums<21>(p, lds);
    double G[4][4], H[4][3], X[4][3];
    G[0][0] = p[0];
    G[0][1] = G[1][0] = p[1];
    G[0][2] = G[2][0] = p[2];
    G[0][3] = G[3][0] = p[3];
    G[1][1] = p[4];
    G[1][2] = G[2][1] = p[5];
    G[1][3] = G[3][1] = p[6];
    G[2][2] = p[7];
    G[2][3] = G[3][2] = p[8];
    G[3][3] = (double)m;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < 3; ++c) H[j][c] = p[9 + 3 * j + c];
    ok = gauss4(G, H, X);
    affine_from_X(X, M);
    ok = ok && finite12(M);
  } else {
    double p[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) p[k] = 0.0;
    for (uint32_t i = t; i < m; i += 256) {
      const size_t o = 3 * (size_t)idx[i];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        p[c] = p[c] + A[o + c];
        p[3 + c] = p[3 + c] + B[o + c];
      }
    }
    block_sums<6>(p, lds);
    double ma[3], mb[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ma[c] = p[c] / (double)m;
      mb[c] = p[3 + c] / (double)m;
    }
    double r[11];
#pragma unroll
    for (int k = 0; k < 11; ++k) r[k] = 0.0;
    for (uint32_t i = t; i < m; i += 256) {
      const size_t o = 3 * (size_t)idx[i];
      const double a0 = A[o] - ma[0], a1 = A[o + 1] - ma[1], a2 = A[o + 2] - ma[2];
      const double b0 = B[o] - mb[0], b1 = B[o + 1] - mb[1], b2 = B[o + 2] - mb[2];
      r[0] = r[0] + b0 * a0;
      r[1] = r[1] + b0 * a1;
      r[2] = r[2] + b0 * a2;
      r[3] = r[3] + b1 * a0;
      r[4] = r[4] + b1 * a1;
      r[5] = r[5] + b1 * a2;
      r[6] = r[6] + b2 * a0;
      r[7] = r[7] + b2 * a1;
      r[8] = r[8] + b2 * a2;
      r[9] = r[9] + ((a0 * a0 + a1 * a1) + a2 * a2);
      r[10] = r[10] + ((b0 * b0 + b1 * b1) + b2 * b2);
    }
    block_sums<11>(r, lds);
    double S[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) S[i][j] = r[3 * i + j];
    ok = solve_similarity(ma, mb, S, r[9], r[10], M);
  }
  if (t == 0) {
    for (int i = 0; i < 12; ++i) out[i] = ok ? M[i] : 0.0;
    *okp = ok ? 1u : 0u;
  }
}

// nearest other point: lane i keeps min over j != i of (dx dx + dy dy) + dz dz, one square root at the end
__global__ __launch_bounds__(256) void k_merge_nn(const double *__restrict__ X, uint32_t n, double *__restrict__ dist) {
  __shared__ double sx[kNnTile], sy[kNnTile], sz[kNnTile];
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const bool live = i < n;
  const double x = live ? X[3 * (size_t)i] : 0.0, y = live ? X[3 * (size_t)i + 1] : 0.0, z = live ? X[3 * (size_t)i + 2] : 0.0;
  double best = geom::pos_inf();
  for (uint32_t base = 0; base < n; base += kNnTile) {
    const uint32_t m = n - base < kNnTile ? n - base : kNnTile;
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < m; k += 256) {
      sx[k] = X[3 * (size_t)(base + k)];
      sy[k] = X[3 * (size_t)(base + k) + 1];
      sz[k] = X[3 * (size_t)(base + k) + 2];
    }
    __syncthreads();
    for (uint32_t j = 0; j < m; ++j) {
      const double dx = x - sx[j], dy = y - sy[j], dz = z - sz[j];
      const double d2 = (dx * dx + dy * dy) + dz * dz;
      best = (base + j != i && d2 < best) ? d2 : best;
    }
  }
  if (live) dist[i] = sqrt(best);
}

// radix select: histogram of the byte at `shift` over the values whose higher bits equal `prefix`
__global__ __launch_bounds__(256) void k_merge_hist(const uint64_t *__restrict__ v, uint32_t n, uint64_t prefix, int shift,
                                                    uint32_t *__restrict__ hist) {
  __shared__ uint32_t h[256];
  h[threadIdx.x] = 0;
  __syncthreads();
  for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const uint64_t u = v[i];
    const bool match = shift == 56 || (u >> (shift + 8)) == (prefix >> (shift + 8));
    if (match) atomicAdd(&h[(u >> shift) & 255u], 1u);  // (counts: the same whatever the order)
  }
  __syncthreads();
  if (h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], h[threadIdx.x]);
}

// M applied to nR rotations (M[:, :3] R) and nX points (M[:, :3] X + M[:, 3]), in place
struct Mat34 {
  double m[12];
};
__global__ __launch_bounds__(256) void k_merge_transform(Mat34 T, double *__restrict__ R, uint32_t nR, double *__restrict__ X,
                                                         uint32_t nX) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const double *M = T.m;
  if (i < nR) {
    double r[9], o[9];
    for (int k = 0; k < 9; ++k) r[k] = R[9 * (size_t)i + k];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b) o[3 * a + b] = (M[4 * a] * r[b] + M[4 * a + 1] * r[3 + b]) + M[4 * a + 2] * r[6 + b];
    for (int k = 0; k < 9; ++k) R[9 * (size_t)i + k] = o[k];
  } else if (i - nR < nX) {
    const size_t p = 3 * (size_t)(i - nR);
    const double x0 = X[p], x1 = X[p + 1], x2 = X[p + 2];
    X[p] = ((M[0] * x0 + M[1] * x1) + M[2] * x2) + M[3];
    X[p + 1] = ((M[4] * x0 + M[5] * x1) + M[6] * x2) + M[7];
    X[p + 2] = ((M[8] * x0 + M[9] * x1) + M[10] * x2) + M[11];
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------

sfmloc_merge_params merge_params(const sfmloc_merge_params *params) {
  sfmloc_merge_params p;
  if (params) p = *params;
  else sfmloc_merge_default_params(&p);
  return p;
}

int launch_inliers(CallScope *d, const double *dA, const double *dB, uint32_t n, const double *dM, const uint32_t *d_has,
                   double thres, uint32_t *d_idx, uint32_t *d_n) {
  return dev_launch(k_merge_inliers, dim3(1), dim3(1024), 0, d->s, dA, dB, n, dM, d_has, thres, d_idx, d_n);
}

template <int MODEL>
int ransac_impl(CallScope *d, const sfmloc_merge_params &p, const double *A, const double *B, uint32_t n, double thres,
                uint64_t rounds, double svd_ratio, uint32_t stream, sfmloc_merge_result *out, uint32_t *inliers,
                uint32_t cap) {
  int lds = 0;
  SFM_HIP(hipDeviceGetAttribute(&lds, hipDeviceAttributeMaxSharedMemoryPerBlock, p.device));
  uint32_t tile = std::min<uint32_t>(kMergeTile, (uint32_t)lds / 48u);
  SFM_CHECK(tile >= 64, SFMLOC_EHIP, "sfmloc_merge_ransac: the device reports %d bytes of LDS per workgroup", lds);
  tile &= ~63u;
  DevBuf<double> dA, dB, dM, dMf;
  DevBuf<unsigned long long> d_best;
  DevBuf<uint32_t> d_info, d_idx, d_n, d_ok;
  int rc;
#define MRG_TRY(x)     \
  do {                 \
    rc = (x);          \
    if (rc) return rc; \
  } while (0)
  MRG_TRY(dev_upload(nullptr, dA, A, 3 * (size_t)n, d->s));
  MRG_TRY(dev_upload(nullptr, dB, B, 3 * (size_t)n, d->s));
  MRG_TRY(dM.alloc(nullptr, 12));
  MRG_TRY(dMf.alloc(nullptr, 12));
  MRG_TRY(d_best.alloc(nullptr, 1));
  MRG_TRY(d_info.alloc(nullptr, 3));
  MRG_TRY(d_idx.alloc(nullptr, n));
  MRG_TRY(d_n.alloc(nullptr, 1));
  MRG_TRY(d_ok.alloc(nullptr, 1));
  SFM_RC(d_best.zero(1, d->s));
  MRG_TRY(d->time_begin());
  const uint64_t per = p.rounds_per_launch ? p.rounds_per_launch : kMergeLaunchRounds;
  for (uint64_t r0 = 0; r0 < rounds; r0 += per) {
    const uint32_t m = (uint32_t)std::min<uint64_t>(per, rounds - r0);
    SFM_RC(dev_launch(HIP_KERNEL_NAME(k_merge_rounds<MODEL>), dim3((m + kMergeBlock - 1) / kMergeBlock),
                      dim3(kMergeBlock), 6 * tile * sizeof(double), d->s, dA, dB, n, thres, svd_ratio, (uint64_t)p.seed,
                      stream, (uint32_t)r0, m, tile, d_best));
  }
  SFM_RC(dev_launch(HIP_KERNEL_NAME(k_merge_winner<MODEL>), dim3(1), dim3(64), 0, d->s, dA, dB, n, svd_ratio,
                    (uint64_t)p.seed, stream, d_best, dM, d_info));
  MRG_TRY(launch_inliers(d, dA, dB, n, dM, d_info, thres, d_idx, d_n));
  uint32_t info[3] = {0, 0, 0}, n_inl = 0;
  SFM_RC(d_info.download(info, 3, d->s));
  SFM_RC(d_n.download(&n_inl, 1, d->s));
  SFM_HIP(hipStreamSynchronize(d->s));
  out->round = info[1];
  out->count = info[2];
  out->n_inliers = n_inl;
  SFM_CHECK(!info[0] || n_inl == info[2], SFMLOC_EHIP,
            "sfmloc_merge_ransac: the winner's model gives %u inliers where its round counted %u", n_inl, info[2]);
  if (info[0] && n_inl >= 4) {
    SFM_RC(dev_launch(HIP_KERNEL_NAME(k_merge_fit<MODEL>), dim3(1), dim3(256), 0, d->s, dA, dB, d_idx, n_inl, dMf,
                      d_ok));
    uint32_t ok = 0;
    SFM_RC(dMf.download(out->M, 12, d->s));
    SFM_RC(d_ok.download(&ok, 1, d->s));
    SFM_HIP(hipStreamSynchronize(d->s));
    out->has_model = ok;
  }
  MRG_TRY(d->time_end());
  SFM_CHECK(!inliers || cap >= n_inl, SFMLOC_ECAP, "sfmloc_merge_ransac: %u entries, %u inliers", cap, n_inl);
  if (inliers && n_inl) SFM_RC(d_idx.read(inliers, n_inl, d->s));
#undef MRG_TRY
  return SFMLOC_OK;
}

bool all_finite(const double *x, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

// the k-th smallest (0-based) of n positive doubles as bit patterns: 8 passes over one byte each
int radix_select(CallScope *d, const uint64_t *dv, uint32_t n, uint32_t k, uint32_t *d_hist, uint64_t *out) {
  uint64_t prefix = 0;
  uint32_t h[256];
  const uint32_t blocks = std::min<uint32_t>((n + 255) / 256, 1024);
  for (int shift = 56; shift >= 0; shift -= 8) {
    SFM_RC(dev_zero(d_hist, 256, d->s));
    SFM_RC(dev_launch(k_merge_hist, dim3(blocks), dim3(256), 0, d->s, dv, n, prefix, shift, d_hist));
    SFM_RC(dev_download(h, d_hist, 256, d->s));
    SFM_HIP(hipStreamSynchronize(d->s));
    uint32_t b = 0;
    while (b < 255 && k >= h[b]) k -= h[b++];
    prefix |= (uint64_t)b << shift;
  }
  *out = prefix;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_merge_default_params(sfmloc_merge_params *p) {
  if (!p) return;
  sfmloc_params q;
  sfmloc_default_params(&q);
  memset(p, 0, sizeof *p);
  p->seed = q.seed;
  p->device = 0;
  p->rounds_per_launch = 0;
  p->profile = 0;
}

double sfmloc_merge_last_ms(void) { return g_merge_last_ms; }

int sfmloc_merge_ransac(const double *A, const double *B, uint64_t n, double thres, uint64_t rounds, double svd_ratio,
                        int model, uint32_t stream, const sfmloc_merge_params *params, sfmloc_merge_result *out,
                        uint32_t *inliers, uint32_t cap) {
  SFM_CHECK(out, SFMLOC_EINVAL, "sfmloc_merge_ransac: null result");
  memset(out, 0, sizeof *out);
  SFM_CHECK(model == SFMLOC_MERGE_SIMILARITY || model == SFMLOC_MERGE_AFFINE, SFMLOC_EINVAL,
            "sfmloc_merge_ransac: model %d (0 similarity, 1 affine)", model);
  SFM_CHECK(n <= kMergeMaxN, SFMLOC_ECAP, "sfmloc_merge_ransac: %llu matches (at most 2^24)", (unsigned long long)n);
  SFM_CHECK(rounds < (1ull << 32), SFMLOC_ECAP, "sfmloc_merge_ransac: %llu rounds (fewer than 2^32)",
            (unsigned long long)rounds);
  if (n < 4 || rounds == 0) return SFMLOC_OK;  // no sample of 4: no model
  SFM_CHECK(A && B, SFMLOC_EINVAL, "sfmloc_merge_ransac: null points");
  const sfmloc_merge_params p = merge_params(params);
  CallScope d;  // (before the buffers: destroyed after them)
  int rc;
  if ((rc = CallScope::use_device(p.device)) || (rc = d.open(p.profile, &g_merge_last_ms))) return rc;
  return model == SFMLOC_MERGE_AFFINE
             ? ransac_impl<SFMLOC_MERGE_AFFINE>(&d, p, A, B, (uint32_t)n, thres, rounds, svd_ratio, stream, out, inliers, cap)
             : ransac_impl<SFMLOC_MERGE_SIMILARITY>(&d, p, A, B, (uint32_t)n, thres, rounds, svd_ratio, stream, out, inliers,
                                                    cap);
}

int sfmloc_merge_inliers(const double *A, const double *B, uint64_t n, const double *M, double thres,
                         const sfmloc_merge_params *params, uint32_t *idx, uint32_t cap, uint32_t *n_out) {
  SFM_CHECK(n_out && M, SFMLOC_EINVAL, "sfmloc_merge_inliers: null argument");
  *n_out = 0;
  SFM_CHECK(n <= kMergeMaxN, SFMLOC_ECAP, "sfmloc_merge_inliers: %llu matches (at most 2^24)", (unsigned long long)n);
  if (n == 0) return SFMLOC_OK;
  SFM_CHECK(A && B, SFMLOC_EINVAL, "sfmloc_merge_inliers: null points");
  const sfmloc_merge_params p = merge_params(params);
  CallScope d;  // (before the buffers: destroyed after them)
  int rc;
  if ((rc = CallScope::use_device(p.device)) || (rc = d.open(p.profile, &g_merge_last_ms))) return rc;
  DevBuf<double> dA, dB, dM;
  DevBuf<uint32_t> d_idx, d_n;
  if ((rc = dev_upload(nullptr, dA, A, 3 * (size_t)n, d.s)) || (rc = dev_upload(nullptr, dB, B, 3 * (size_t)n, d.s)) ||
      (rc = dev_upload(nullptr, dM, M, 12, d.s)) || (rc = d_idx.alloc(nullptr, n)) || (rc = d_n.alloc(nullptr, 1)))
    return rc;
  if ((rc = d.time_begin())) return rc;
  rc = launch_inliers(&d, dA, dB, (uint32_t)n, dM, nullptr, thres, d_idx, d_n);
  if (rc) return rc;
  if ((rc = d.time_end())) return rc;
  SFM_RC(d_n.download(n_out, 1, d.s));
  SFM_HIP(hipStreamSynchronize(d.s));
  SFM_CHECK(!idx || cap >= *n_out, SFMLOC_ECAP, "sfmloc_merge_inliers: %u entries, %u inliers", cap, *n_out);
  if (idx && *n_out) SFM_RC(d_idx.read(idx, *n_out, d.s));
  return SFMLOC_OK;
}

int sfmloc_merge_median_nn(const double *X, uint64_t n, const sfmloc_merge_params *params, double *median) {
  SFM_CHECK(median, SFMLOC_EINVAL, "sfmloc_merge_median_nn: null result");
  *median = 0.0;
  SFM_CHECK(n <= kMergeMaxN, SFMLOC_ECAP, "sfmloc_merge_median_nn: %llu points (at most 2^24)", (unsigned long long)n);
  if (n < 2) return SFMLOC_OK;
  SFM_CHECK(X, SFMLOC_EINVAL, "sfmloc_merge_median_nn: null points");
  SFM_CHECK(all_finite(X, 3 * (size_t)n), SFMLOC_EINVAL, "sfmloc_merge_median_nn: a coordinate is not finite");
  const sfmloc_merge_params p = merge_params(params);
  CallScope d;  // (before the buffers: destroyed after them)
  int rc;
  if ((rc = CallScope::use_device(p.device)) || (rc = d.open(p.profile, &g_merge_last_ms))) return rc;
  DevBuf<double> dX, d_dist;
  DevBuf<uint32_t> d_hist;
  if ((rc = dev_upload(nullptr, dX, X, 3 * (size_t)n, d.s)) || (rc = d_dist.alloc(nullptr, n)) ||
      (rc = d_hist.alloc(nullptr, 256)))
    return rc;
  if ((rc = d.time_begin())) return rc;
  SFM_RC(dev_launch(k_merge_nn, dim3(((uint32_t)n + 255) / 256), dim3(256), 0, d.s, dX, (uint32_t)n, d_dist));
  // (distances are >= 0 and finite or +inf on overflow: they order as their bit patterns)
  uint64_t lo = 0, hi = 0;
  const uint32_t k_hi = (uint32_t)(n / 2);
  if ((rc = radix_select(&d, reinterpret_cast<const uint64_t *>(d_dist.get()), (uint32_t)n, k_hi, d_hist, &hi))) return rc;
  lo = hi;
  if (n % 2 == 0 &&
      (rc = radix_select(&d, reinterpret_cast<const uint64_t *>(d_dist.get()), (uint32_t)n, k_hi - 1, d_hist, &lo)))
    return rc;
  if ((rc = d.time_end())) return rc;
  double dlo, dhi;
  memcpy(&dlo, &lo, 8);
  memcpy(&dhi, &hi, 8);
  *median = n % 2 ? dhi : (dlo + dhi) / 2.0;
  return SFMLOC_OK;
}

int sfmloc_merge_transform(const double *M, double *R, uint64_t nR, double *X, uint64_t nX,
                           const sfmloc_merge_params *params) {
  SFM_CHECK(M, SFMLOC_EINVAL, "sfmloc_merge_transform: null matrix");
  SFM_CHECK(nR <= kMergeMaxN && nX <= kMergeMaxN, SFMLOC_ECAP, "sfmloc_merge_transform: at most 2^24 rotations and points");
  SFM_CHECK((nR == 0 || R) && (nX == 0 || X), SFMLOC_EINVAL, "sfmloc_merge_transform: null array");
  if (nR + nX == 0) return SFMLOC_OK;
  const sfmloc_merge_params p = merge_params(params);
  CallScope d;  // (before the buffers: destroyed after them)
  int rc;
  if ((rc = CallScope::use_device(p.device)) || (rc = d.open(p.profile, &g_merge_last_ms))) return rc;
  DevBuf<double> dR, dX;  // (either may be empty and still has an address)
  if ((rc = dev_upload(nullptr, dR, (const double *)R, 9 * (size_t)nR, d.s, 1)) ||
      (rc = dev_upload(nullptr, dX, (const double *)X, 3 * (size_t)nX, d.s, 1)))
    return rc;
  Mat34 T;
  memcpy(T.m, M, sizeof T.m);
  if ((rc = d.time_begin())) return rc;
  SFM_RC(dev_launch(k_merge_transform, dim3((uint32_t)((nR + nX + 255) / 256)), dim3(256), 0, d.s, T, dR, (uint32_t)nR,
                    dX, (uint32_t)nX));
  if ((rc = d.time_end())) return rc;
  if (nR) SFM_RC(dR.download(R, 9 * (size_t)nR, d.s));
  if (nX) SFM_RC(dX.download(X, 3 * (size_t)nX, d.s));
  SFM_HIP(hipStreamSynchronize(d.s));
  return SFMLOC_OK;
}

}  // extern "C"
