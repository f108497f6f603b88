// sfmloc_bowtrain: the vocabulary training of TrainBoW (TrainBoW/src/TrainBoW.cpp) on the device.
//
//   sampling    getRandomTrainFeatures (TrainBoW.cpp:95-131): the dense descriptors of a drawn image (the sfmloc_imgbow
//               front end: resize + gray + min-max, M-LDB at the 300 x 300 grid) and a gather of the drawn rows into the
//               resident sample; no descriptor crosses PCIe.
//   PCA         cv::PCA (PcaWrapper.cpp:31-46): first and second moments in f64 per chunk of rows, chunks added in order
//               (integer rows: exact, independent of launch shape), eigen-decomposition on the host (cyclic Jacobi).
//   projection  PcaWrapper::calcPcaProject with bow.hip's device arithmetic (bof_device.h).
//   k-means     cv::kmeans as BoFSpatialPyramids::trainKMeans calls it (BoFSpatialPyramids.cpp:95-106): k-means++ seeding,
//               Lloyd steps, the empty-cluster rule, best of the attempts.  The arithmetic is stated in include/sfmloc.h.
// No float atomics anywhere: every sum has one fixed order (sequential per chunk of kTbChunk rows, chunks in order).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <cfloat>
#include <new>
#include <vector>

#include "bof_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint32_t kTbChunk = 1024;  // rows per fixed-order partial sum
constexpr int kTbMaxDim = 64;
constexpr int kTbMomSlots = 9;       // moments per thread: (64 + 64 * 65 / 2) / 256 rounded up
constexpr int kTbTile = 64;          // rows per LDS tile of the moments kernel

// ---- cv::RNG restated (the multiply-with-carry generator of OpenCV's core) ----
inline uint32_t rng_next(uint64_t *s) {
  *s = (uint64_t)(uint32_t)*s * 4164903690ull + (*s >> 32);
  return (uint32_t)*s;
}
inline float rng_uniform01(uint64_t *s) { return (float)rng_next(s) * 2.3283064365386962890625e-10f; }
inline double rng_double(uint64_t *s) {
  const uint32_t t = rng_next(s);
  const uint64_t lo = rng_next(s);
  return (double)(((uint64_t)t << 32) | lo) * 5.4210108624275221700372640043497e-20;
}

// descriptor bytes (rows of 64, the first dim used) at the drawn indices -> f32 rows of the sample
__global__ __launch_bounds__(256) void k_tb_gather8(const uint8_t *__restrict__ desc8, const uint32_t *__restrict__ idx,
                                                    uint32_t n_pick, uint32_t dim, float *__restrict__ out) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n_pick * dim) return;
  const uint32_t j = e / dim, i = e - j * dim;
  out[e] = (float)desc8[(size_t)idx[j] * 64 + i];
}

// f32 rows at the given indices (k-means++ centres)
__global__ __launch_bounds__(256) void k_tb_gather_rows(const float *__restrict__ x, const int32_t *__restrict__ idx,
                                                        uint32_t n, uint32_t dim, float *__restrict__ out) {
  const uint32_t e = blockIdx.x * 256 + threadIdx.x;
  if (e >= n * dim) return;
  const uint32_t j = e / dim, i = e - j * dim;
  out[e] = x[(size_t)idx[j] * dim + i];
}

// moments of one chunk: output o < dim is sum x_o, o >= dim the upper-triangle pair (i <= j, row major) sum x_i x_j.
// Each thread owns up to kTbMomSlots outputs and walks the chunk's rows in order (f64; the products of integer rows
// 0..255 and their sums are exact).
__global__ __launch_bounds__(256) void k_tb_moments(const float *__restrict__ x, uint32_t n, uint32_t dim,
                                                    double *__restrict__ part /*[chunks][n_out]*/) {
  __shared__ float tile[kTbTile * kTbMaxDim];
  const uint32_t n_out = dim + dim * (dim + 1) / 2;
  const uint32_t r0 = blockIdx.x * kTbChunk, r1 = min(n, r0 + kTbChunk);
  int oi[kTbMomSlots], oj[kTbMomSlots];
  double acc[kTbMomSlots];
#pragma unroll
  for (int s = 0; s < kTbMomSlots; ++s) {
    const uint32_t o = threadIdx.x + 256u * s;
    acc[s] = 0.0;
    oi[s] = -1;
    oj[s] = -1;
    if (o < dim) {
      oi[s] = (int)o;
    } else if (o < n_out) {
      uint32_t p = o - dim, i = 0;
      while (p >= dim - i) {
        p -= dim - i;
        ++i;
      }
      oi[s] = (int)i;
      oj[s] = (int)(i + p);
    }
  }
  for (uint32_t t0 = r0; t0 < r1; t0 += kTbTile) {
    const uint32_t rows = min((uint32_t)kTbTile, r1 - t0);
    __syncthreads();
    for (uint32_t e = threadIdx.x; e < rows * dim; e += 256) tile[e] = x[(size_t)t0 * dim + e];
    __syncthreads();
#pragma unroll
    for (int s = 0; s < kTbMomSlots; ++s) {
      if (oi[s] < 0) continue;
      double a = acc[s];
      if (oj[s] < 0) {
        for (uint32_t r = 0; r < rows; ++r) a = a + (double)tile[r * dim + oi[s]];
      } else {
        for (uint32_t r = 0; r < rows; ++r) {
          const double p = (double)tile[r * dim + oi[s]] * (double)tile[r * dim + oj[s]];
          a = a + p;
        }
      }
      acc[s] = a;
    }
  }
#pragma unroll
  for (int s = 0; s < kTbMomSlots; ++s) {
    const uint32_t o = threadIdx.x + 256u * s;
    if (o < n_out) part[(size_t)blockIdx.x * n_out + o] = acc[s];
  }
}

// column sums of [rows x cols] f64 partials, rows in order
__global__ __launch_bounds__(256) void k_tb_colsum(const double *__restrict__ part, uint32_t rows, uint32_t cols,
                                                   double *__restrict__ out) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
  for (uint32_t r = 0; r < rows; ++r) s = s + part[(size_t)r * cols + c];
  out[c] = s;
}

// the sample -> PCA space (PcaWrapper::calcPcaProject): one thread per (row, component)
__global__ __launch_bounds__(256) void k_tb_project(const float *__restrict__ x, uint32_t n, int in_dim,
                                                    const float *__restrict__ mean, const float *__restrict__ evec,
                                                    const float *__restrict__ eval, int n_pca, float *__restrict__ y) {
  const uint64_t e = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (uint64_t)n * n_pca) return;
  const uint32_t r = (uint32_t)(e / n_pca), d = (uint32_t)(e - (uint64_t)r * n_pca);
  y[e] = bof_pca_component(x + (size_t)r * in_dim, mean, evec + (size_t)d * in_dim, in_dim, eval[d]);
}

// squared distance of a row held in registers to a centre (LDS or global), the stated f32 chain
template <int DMAX>
__device__ __forceinline__ float tb_dist(const float (&x)[DMAX], const float *c, int dim) {
  float s = 0.0f;
#pragma unroll
  for (int d = 0; d < DMAX; ++d) {
    if (d < dim) {
      const float t = x[d] - c[d];
      const float t2 = t * t;
      s = s + t2;
    }
  }
  return s;
}

template <int DMAX>
__device__ __forceinline__ void tb_load_row(float (&x)[DMAX], const float *__restrict__ row, int dim) {
#pragma unroll
  for (int d = 0; d < DMAX; ++d) x[d] = d < dim ? row[d] : 0.0f;
}

// k-means++: out[i] = min(dist(x_i, x_ci), prev[i]) (prev == NULL: the distance alone)
template <int DMAX>
__global__ __launch_bounds__(256) void k_tb_pp_dist(const float *__restrict__ x, uint32_t n, int dim,
                                                    const int32_t *__restrict__ d_ci, int32_t ci_host,
                                                    const float *__restrict__ prev, float *__restrict__ out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int32_t ci = d_ci ? *d_ci : ci_host;
  float xi[DMAX];
  tb_load_row<DMAX>(xi, x + (size_t)i * dim, dim);
  float d = tb_dist<DMAX>(xi, x + (size_t)ci * dim, dim);
  if (prev) {
    const float p = prev[i];
    d = p < d ? p : d;  // std::min(d, p)
  }
  out[i] = d;
}

// f64 sum of each chunk of kTbChunk f32 values, sequential; one thread per chunk
__global__ __launch_bounds__(256) void k_tb_chunk_sum(const float *__restrict__ v, uint32_t n, double *__restrict__ part) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  const uint32_t r0 = c * kTbChunk;
  if (r0 >= n) return;
  const uint32_t r1 = min(n, r0 + kTbChunk);
  double s = 0.0;
  for (uint32_t r = r0; r < r1; ++r) s = s + (double)v[r];
  part[c] = s;
}

struct PpPick {
  double total;
  int32_t ci;
  int32_t pad;
};

// one thread: total = the chunk partials in order; with u >= 0 also the draw: the first i with R_i >= u * total
__global__ void k_tb_pp_pick(const double *__restrict__ part, uint32_t n_chunks, const float *__restrict__ v, uint32_t n,
                             double u, PpPick *__restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  double total = 0.0;
  for (uint32_t c = 0; c < n_chunks; ++c) total = total + part[c];
  int32_t ci = (int32_t)n - 1;
  if (u >= 0.0) {
    const double target = u * total;
    double before = 0.0;
    for (uint32_t c = 0; c < n_chunks; ++c) {
      const double end = before + part[c];
      if (end >= target) {
        const uint32_t r0 = c * kTbChunk, r1 = min(n, r0 + kTbChunk);
        double q = 0.0;
        for (uint32_t r = r0; r < r1; ++r) {
          q = q + (double)v[r];
          if (before + q >= target) {
            ci = (int32_t)r;
            break;
          }
        }
        break;
      }
      before = end;
    }
  }
  out->total = total;
  out->ci = ci;
}

// assignment: nearest centre (ties to the lower index) and its distance; centres in LDS
template <int DMAX>
__global__ __launch_bounds__(256) void k_tb_assign(const float *__restrict__ x, uint32_t n, int dim,
                                                   const float *__restrict__ centers, int K, int32_t *__restrict__ labels,
                                                   float *__restrict__ mind) {
  extern __shared__ float s_cen[];  // [K][dim]
  for (int e = threadIdx.x; e < K * dim; e += 256) s_cen[e] = centers[e];
  __syncthreads();
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float xi[DMAX];
  tb_load_row<DMAX>(xi, x + (size_t)i * dim, dim);
  int best = 0;
  float bestd = INFINITY;
  for (int k = 0; k < K; ++k) {
    const float d = tb_dist<DMAX>(xi, s_cen + (size_t)k * dim, dim);
    if (d < bestd) {
      bestd = d;
      best = k;
    }
  }
  labels[i] = best;
  mind[i] = bestd;
}

// per-chunk centre sums: one wave, lane = dimension, the chunk's rows in order; counts by lane 0
__global__ __launch_bounds__(64) void k_tb_csum_part(const float *__restrict__ x, uint32_t n, int dim,
                                                     const int32_t *__restrict__ labels, int K,
                                                     double *__restrict__ part_sum /*[chunks][K][dim]*/,
                                                     uint32_t *__restrict__ part_cnt /*[chunks][K]*/) {
  extern __shared__ double s_acc[];  // [K][dim], then K u32 counts
  uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_acc + (size_t)K * dim);
  const int lane = threadIdx.x;
  for (int e = lane; e < K * dim; e += 64) s_acc[e] = 0.0;
  for (int e = lane; e < K; e += 64) s_cnt[e] = 0u;
  __syncthreads();
  const uint32_t r0 = blockIdx.x * kTbChunk, r1 = min(n, r0 + kTbChunk);
  for (uint32_t r = r0; r < r1; ++r) {
    const int k = labels[r];
    if (lane < dim) s_acc[(size_t)k * dim + lane] = s_acc[(size_t)k * dim + lane] + (double)x[(size_t)r * dim + lane];
    if (lane == 0) s_cnt[k] += 1u;
  }
  __syncthreads();
  for (int e = lane; e < K * dim; e += 64) part_sum[(size_t)blockIdx.x * K * dim + e] = s_acc[e];
  for (int e = lane; e < K; e += 64) part_cnt[(size_t)blockIdx.x * K + e] = s_cnt[e];
}

__global__ __launch_bounds__(256) void k_tb_cnt_sum(const uint32_t *__restrict__ part, uint32_t rows, int K,
                                                    uint32_t *__restrict__ out) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= K) return;
  uint32_t s = 0;
  for (uint32_t r = 0; r < rows; ++r) s += part[(size_t)r * K + k];
  out[k] = s;
}

// the empty-cluster rule, clusters in index order (one 1024-thread workgroup): the biggest cluster (first on ties),
// its farthest point from its centre (the last on ties) becomes a one-point cluster
constexpr int kTbEmptyThreads = 1024;
template <int DMAX>
__global__ __launch_bounds__(1024) void k_tb_empty(const float *__restrict__ x, uint32_t n, int dim, int K,
                                                   int32_t *__restrict__ labels, double *__restrict__ sum,
                                                   uint32_t *__restrict__ cnt) {
  __shared__ float s_base[kTbMaxDim];
  __shared__ float s_bd[kTbEmptyThreads];
  __shared__ int32_t s_bi[kTbEmptyThreads];
  __shared__ int s_maxk;
  const int tid = threadIdx.x;
  for (int k = 0; k < K; ++k) {
    if (cnt[k] != 0) continue;  // (uniform: every thread reads the same value; written only below, behind barriers)
    if (tid == 0) {
      int mk = 0;
      for (int k1 = 1; k1 < K; ++k1)
        if (cnt[mk] < cnt[k1]) mk = k1;
      s_maxk = mk;
    }
    __syncthreads();
    const int mk = s_maxk;
    if (tid < dim) s_base[tid] = (float)(sum[(size_t)mk * dim + tid] / (double)cnt[mk]);
    __syncthreads();
    float bd = -1.0f;
    int32_t bi = -1;
    const uint32_t per = (n + kTbEmptyThreads - 1) / kTbEmptyThreads;
    const uint32_t lo = min(n, (uint32_t)tid * per), hi = min(n, lo + per);
    for (uint32_t i = lo; i < hi; ++i) {
      if (labels[i] != mk) continue;
      float xi[DMAX];
      tb_load_row<DMAX>(xi, x + (size_t)i * dim, dim);
      const float d = tb_dist<DMAX>(xi, s_base, dim);
      if (bd <= d) {
        bd = d;
        bi = (int32_t)i;
      }
    }
    s_bd[tid] = bd;
    s_bi[tid] = bi;
    __syncthreads();
    for (int stride = kTbEmptyThreads / 2; stride >= 1; stride >>= 1) {
      if (tid < stride) {
        const float od = s_bd[tid + stride];
        const int32_t oi = s_bi[tid + stride];
        if (oi >= 0 && (s_bi[tid] < 0 || od > s_bd[tid] || (od == s_bd[tid] && oi > s_bi[tid]))) {
          s_bd[tid] = od;
          s_bi[tid] = oi;
        }
      }
      __syncthreads();
    }
    const int32_t far = s_bi[0];  // (the biggest cluster is not empty: far >= 0)
    if (tid < dim && far >= 0) {
      const double v = (double)x[(size_t)far * dim + tid];
      sum[(size_t)mk * dim + tid] = sum[(size_t)mk * dim + tid] - v;
      sum[(size_t)k * dim + tid] = sum[(size_t)k * dim + tid] + v;
    }
    __syncthreads();
    if (tid == 0 && far >= 0) {
      cnt[mk] -= 1u;
      cnt[k] += 1u;
      labels[far] = k;
    }
    __syncthreads();
    __threadfence_block();
  }
}

// centres = f32(sum / count); squared shift against the old centres in f64; the largest shift (one workgroup)
__global__ __launch_bounds__(1024) void k_tb_divide(const double *__restrict__ sum, const uint32_t *__restrict__ cnt, int K,
                                                    int dim, const float *__restrict__ old_c, float *__restrict__ new_c,
                                                    double *__restrict__ max_shift) {
  __shared__ double s_m[1024];
  double m = 0.0;
  for (int k = threadIdx.x; k < K; k += 1024) {
    double sh = 0.0;
    for (int d = 0; d < dim; ++d) {
      const float c = (float)(sum[(size_t)k * dim + d] / (double)cnt[k]);
      new_c[(size_t)k * dim + d] = c;
      const double t = (double)c - (double)old_c[(size_t)k * dim + d];
      sh = sh + t * t;
    }
    m = sh > m ? sh : m;
  }
  s_m[threadIdx.x] = m;
  __syncthreads();
  for (int stride = 512; stride >= 1; stride >>= 1) {
    if ((int)threadIdx.x < stride) s_m[threadIdx.x] = s_m[threadIdx.x + stride] > s_m[threadIdx.x] ? s_m[threadIdx.x + stride] : s_m[threadIdx.x];
    __syncthreads();
  }
  if (threadIdx.x == 0) *max_shift = s_m[0];
}

// ---- host: cyclic Jacobi on a symmetric f64 matrix (row major, n x n) ----
void jacobi_eigen(std::vector<double> a, int n, std::vector<double> *vals, std::vector<double> *vecs /*rows*/) {
  std::vector<double> v((size_t)n * n, 0.0);
  for (int i = 0; i < n; ++i) v[(size_t)i * n + i] = 1.0;
  for (int sweep = 0; sweep < 100; ++sweep) {
    double off = 0.0, diag = 0.0;
    for (int i = 0; i < n; ++i) {
      diag += a[(size_t)i * n + i] * a[(size_t)i * n + i];
      for (int j = i + 1; j < n; ++j) off += a[(size_t)i * n + j] * a[(size_t)i * n + j];
    }
    if (off == 0.0 || off <= 1e-36 * diag) break;
    for (int p = 0; p < n; ++p)
      for (int q = p + 1; q < n; ++q) {
        const double apq = a[(size_t)p * n + q];
        if (apq == 0.0) continue;
        const double app = a[(size_t)p * n + p], aqq = a[(size_t)q * n + q];
        const double theta = (aqq - app) / (2.0 * apq);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        for (int k = 0; k < n; ++k) {  // A <- A J (columns p, q)
          const double akp = a[(size_t)k * n + p], akq = a[(size_t)k * n + q];
          a[(size_t)k * n + p] = c * akp - s * akq;
          a[(size_t)k * n + q] = s * akp + c * akq;
        }
        for (int k = 0; k < n; ++k) {  // A <- J^T A (rows p, q)
          const double apk = a[(size_t)p * n + k], aqk = a[(size_t)q * n + k];
          a[(size_t)p * n + k] = c * apk - s * aqk;
          a[(size_t)q * n + k] = s * apk + c * aqk;
        }
        a[(size_t)p * n + q] = a[(size_t)q * n + p] = 0.0;
        for (int k = 0; k < n; ++k) {  // V <- V J (eigenvectors as columns)
          const double vkp = v[(size_t)k * n + p], vkq = v[(size_t)k * n + q];
          v[(size_t)k * n + p] = c * vkp - s * vkq;
          v[(size_t)k * n + q] = s * vkp + c * vkq;
        }
      }
  }
  std::vector<int> order(n);
  for (int i = 0; i < n; ++i) order[i] = i;
  std::stable_sort(order.begin(), order.end(), [&](int x, int y) { return a[(size_t)x * n + x] > a[(size_t)y * n + y]; });
  vals->assign(n, 0.0);
  vecs->assign((size_t)n * n, 0.0);
  for (int r = 0; r < n; ++r) {
    const int c = order[r];
    (*vals)[r] = a[(size_t)c * n + c];
    int big = 0;  // sign rule: the largest-magnitude component positive (the first such on ties)
    for (int k = 1; k < n; ++k)
      if (fabs(v[(size_t)k * n + c]) > fabs(v[(size_t)big * n + c])) big = k;
    const double sg = v[(size_t)big * n + c] < 0 ? -1.0 : 1.0;
    for (int k = 0; k < n; ++k) (*vecs)[(size_t)r * n + k] = sg * v[(size_t)k * n + c];
  }
}

}  // namespace

struct BowTrain {
  int device = 0;
  uint32_t dim0 = 0, dim = 0, cap = 0, n = 0;
  hipStream_t s = nullptr;  // the extractor's own non-blocking stream: every call of the trainer queues on it
  sfmloc_akaze *ak = nullptr;
  DenseGrayPlan plan;
  bool plan_ok = false;
  DevBuf<float> d_grid;
  uint32_t n_grid = 0;
  DevBuf<uint8_t> d_src;
  std::vector<uint8_t> last_img;  // the image whose descriptors akaze_desc_dev holds
  uint32_t last_w = 0, last_h = 0, last_c = 0;
  DevBuf<uint32_t> d_idx;
  DevBuf<float> d_x, d_y;  // the sample [cap x dim0] and the projection target
  // PCA
  bool pca_ok = false;
  std::vector<double> mean, cov, evec, eval;
  DevBuf<double> d_part, d_mom;
  DevBuf<float> d_pmean, d_pevec, d_peval;  // the projection's model: allocated together (sfmloc_bowtrain_project)
};

namespace {
int tb_part(BowTrain *t, size_t doubles) {
  if (t->d_part.bytes() >= doubles * sizeof(double)) return SFMLOC_OK;
  SFM_HIP(hipStreamSynchronize(t->s));
  return t->d_part.alloc(nullptr, doubles);
}

uint32_t tb_chunks(uint32_t n) { return (n + kTbChunk - 1) / kTbChunk; }

int tb_moments(BowTrain *t) {
  if (t->pca_ok) return SFMLOC_OK;
  const uint32_t n = t->n, dim = t->dim;
  SFM_CHECK(n >= 1, SFMLOC_EINVAL, "sfmloc_bowtrain_pca: empty sample");
  const uint32_t n_out = dim + dim * (dim + 1) / 2, chunks = tb_chunks(n);
  int rc = tb_part(t, (size_t)chunks * n_out);
  if (rc) return rc;
  if (!t->d_mom && (rc = t->d_mom.alloc(nullptr, (size_t)(kTbMaxDim + kTbMaxDim * (kTbMaxDim + 1) / 2)))) return rc;
  SFM_RC(dev_launch(k_tb_moments, dim3(chunks), dim3(256), 0, t->s, t->d_x, n, dim, t->d_part));
  SFM_RC(dev_launch(k_tb_colsum, dim3((n_out + 255) / 256), dim3(256), 0, t->s, t->d_part, chunks, n_out, t->d_mom));
  std::vector<double> mom(n_out);
  SFM_RC(t->d_mom.download(mom.data(), n_out, t->s));
  SFM_HIP(hipStreamSynchronize(t->s));
  const double N = (double)n;
  t->mean.assign(dim, 0.0);
  t->cov.assign((size_t)dim * dim, 0.0);
  for (uint32_t i = 0; i < dim; ++i) t->mean[i] = mom[i] / N;
  uint32_t o = dim;
  for (uint32_t i = 0; i < dim; ++i)
    for (uint32_t j = i; j < dim; ++j, ++o) {
      const double mm = t->mean[i] * t->mean[j];
      const double c = (mom[o] - N * mm) / N;
      t->cov[(size_t)i * dim + j] = t->cov[(size_t)j * dim + i] = c;
    }
  jacobi_eigen(t->cov, (int)dim, &t->eval, &t->evec);
  t->pca_ok = true;
  return SFMLOC_OK;
}

struct KmWork {
  DevBuf<float> dist[3];
  DevBuf<double> dpart[3];
  DevBuf<PpPick> d_pick;
  DevBuf<int32_t> d_ids, d_labels, d_best_labels;
  DevBuf<float> d_mind, d_best_mind, d_cen[2], d_best_cen;
  DevBuf<double> d_psum, d_sum, d_shift;
  DevBuf<uint32_t> d_pcnt, d_cnt;
};

template <int DMAX>
int tb_kmeans(BowTrain *t, uint32_t K, uint32_t attempts, uint32_t max_iter, double eps, uint64_t seed, float *centers,
              int32_t *labels, float *min_dist, double *compactness, uint32_t *iterations) {
  const uint32_t n = t->n, dim = t->dim, chunks = tb_chunks(n);
  const hipStream_t s = t->s;
  const dim3 g_rows((n + 255) / 256), g_chunks((chunks + 255) / 256);
  KmWork w;
  int rc = SFMLOC_OK;
  for (int i = 0; i < 3 && !rc; ++i) {
    rc = w.dist[i].alloc(nullptr, n);
    if (!rc) rc = w.dpart[i].alloc(nullptr, chunks);
  }
  if (!rc) rc = w.d_pick.alloc(nullptr, 2);
  if (!rc) rc = w.d_ids.alloc(nullptr, K);
  if (!rc) rc = w.d_labels.alloc(nullptr, n);
  if (!rc) rc = w.d_best_labels.alloc(nullptr, n);
  if (!rc) rc = w.d_mind.alloc(nullptr, n);
  if (!rc) rc = w.d_best_mind.alloc(nullptr, n);
  for (int i = 0; i < 2 && !rc; ++i) rc = w.d_cen[i].alloc(nullptr, (size_t)K * dim);
  if (!rc) rc = w.d_best_cen.alloc(nullptr, (size_t)K * dim);
  if (!rc) rc = w.d_psum.alloc(nullptr, (size_t)chunks * K * dim);
  if (!rc) rc = w.d_sum.alloc(nullptr, (size_t)K * dim);
  if (!rc) rc = w.d_shift.alloc(nullptr, 1);
  if (!rc) rc = w.d_pcnt.alloc(nullptr, (size_t)chunks * K);
  if (!rc) rc = w.d_cnt.alloc(nullptr, K);
  if (rc) return rc;
  uint64_t rng = seed ? seed : 0xffffffffull;
  const double e = eps > 0 ? eps : 0.0, eps2 = e * e;
  const uint32_t iter_end = std::max(max_iter, 2u);
  const size_t lds_assign = (size_t)K * dim * sizeof(float);
  const size_t lds_csum = (size_t)K * dim * sizeof(double) + (size_t)K * sizeof(uint32_t);
  // (lds_csum: up to 64 KB -- 49 KB for the reference's K = 100 x 61 --, above the default limit of a launch)
  uint32_t n_iter = 0;
  double best = DBL_MAX;
  std::vector<int32_t> ids(K);
  for (uint32_t a = 0; a < attempts; ++a) {
    int cur = 0;  // d_cen[cur]: the current centres
    double max_shift = DBL_MAX, compact = 0.0;
    for (uint32_t iter = 0;;) {
      if (iter == 0) {
        // generateCentersPP: dist = d(x, x_c0); per centre three trials, the one of the smallest potential is kept
        int di = 0, ti = 1, t2 = 2;
        ids[0] = (int32_t)(rng_next(&rng) % n);
        SFM_RC(dev_launch(k_tb_pp_dist<DMAX>, g_rows, dim3(256), 0, s, t->d_x, n, (int)dim, nullptr, ids[0], nullptr,
                          w.dist[di]));
        SFM_RC(dev_launch(k_tb_chunk_sum, g_chunks, dim3(256), 0, s, w.dist[di], n, w.dpart[di]));
        double sum0 = 0.0;
        {
          SFM_RC(dev_launch(k_tb_pp_pick, dim3(1), dim3(64), 0, s, w.dpart[di], chunks, w.dist[di], n, -1.0,
                            w.d_pick + 1));
          PpPick p{};
          SFM_RC(w.d_pick.download(&p, 1, s, 1));
          SFM_HIP(hipStreamSynchronize(s));
          sum0 = p.total;
        }
        for (uint32_t k = 1; k < K; ++k) {
          double best_sum = DBL_MAX;
          int32_t best_c = -1;
          for (int trial = 0; trial < 3; ++trial) {
            const double u = rng_double(&rng);
            // the draw on dist (slot 0), the trial's potential on min(dist, d(x, x_ci)) (slot 1)
            SFM_RC(dev_launch(k_tb_pp_pick, dim3(1), dim3(64), 0, s, w.dpart[di], chunks, w.dist[di], n, u, w.d_pick));
            SFM_RC(dev_launch(k_tb_pp_dist<DMAX>, g_rows, dim3(256), 0, s, t->d_x, n, (int)dim, &w.d_pick.get()->ci, 0,
                              w.dist[di], w.dist[t2]));
            SFM_RC(dev_launch(k_tb_chunk_sum, g_chunks, dim3(256), 0, s, w.dist[t2], n, w.dpart[t2]));
            SFM_RC(dev_launch(k_tb_pp_pick, dim3(1), dim3(64), 0, s, w.dpart[t2], chunks, w.dist[t2], n, -1.0,
                              w.d_pick + 1));
            PpPick p[2];
            SFM_RC(w.d_pick.download(p, 2, s));
            SFM_HIP(hipStreamSynchronize(s));
            if (p[1].total < best_sum) {
              best_sum = p[1].total;
              best_c = p[0].ci;
              std::swap(ti, t2);
            }
          }
          SFM_CHECK(best_c >= 0, SFMLOC_EINVAL, "sfmloc_bowtrain_kmeans: can't update cluster center (huge or NaN values)");
          ids[k] = best_c;
          sum0 = best_sum;
          std::swap(di, ti);
        }
        (void)sum0;
        SFM_RC(w.d_ids.upload(ids.data(), K, s));
        SFM_RC(dev_launch(k_tb_gather_rows, dim3((K * dim + 255) / 256), dim3(256), 0, s, t->d_x, w.d_ids, K, dim,
                          w.d_cen[cur]));
        SFM_HIP(hipStreamSynchronize(s));  // (ids is read by the copy above)
      } else {
        // centres from the labels: per-chunk f64 sums, chunks in order, the empty-cluster rule, the division
        SFM_RC(dev_launch(k_tb_csum_part, dim3(chunks), dim3(64), lds_csum, s, t->d_x, n, (int)dim, w.d_labels, (int)K,
                          w.d_psum, w.d_pcnt));
        SFM_RC(dev_launch(k_tb_colsum, dim3((K * dim + 255) / 256), dim3(256), 0, s, w.d_psum, chunks, K * dim,
                          w.d_sum));
        SFM_RC(dev_launch(k_tb_cnt_sum, dim3((K + 255) / 256), dim3(256), 0, s, w.d_pcnt, chunks, (int)K, w.d_cnt));
        SFM_RC(dev_launch(k_tb_empty<DMAX>, dim3(1), dim3(kTbEmptyThreads), 0, s, t->d_x, n, (int)dim, (int)K,
                          w.d_labels, w.d_sum, w.d_cnt));
        SFM_RC(dev_launch(k_tb_divide, dim3(1), dim3(1024), 0, s, w.d_sum, w.d_cnt, (int)K, (int)dim, w.d_cen[cur],
                          w.d_cen[cur ^ 1], w.d_shift));
        cur ^= 1;
        SFM_RC(w.d_shift.download(&max_shift, 1, s));
        SFM_HIP(hipStreamSynchronize(s));
      }
      if (++iter == iter_end || max_shift <= eps2) break;
      ++n_iter;  // (one more assignment: the Lloyd iterations of all attempts)
      SFM_RC(dev_launch(k_tb_assign<DMAX>, g_rows, dim3(256), lds_assign, s, t->d_x, n, (int)dim, w.d_cen[cur], (int)K,
                        w.d_labels, w.d_mind));
    }
    // compactness: the min distances of the last assignment, chunked f64 sum
    SFM_RC(dev_launch(k_tb_chunk_sum, g_chunks, dim3(256), 0, s, w.d_mind, n, w.dpart[0]));
    SFM_RC(dev_launch(k_tb_pp_pick, dim3(1), dim3(64), 0, s, w.dpart[0], chunks, w.d_mind, n, -1.0, w.d_pick + 1));
    PpPick p{};
    SFM_RC(w.d_pick.download(&p, 1, s, 1));
    SFM_HIP(hipStreamSynchronize(s));
    compact = p.total;
    if (compact < best) {
      best = compact;
      SFM_RC(w.d_best_cen.copy_from(w.d_cen[cur], (size_t)K * dim, s));
      SFM_RC(w.d_best_labels.copy_from(w.d_labels, n, s));
      SFM_RC(w.d_best_mind.copy_from(w.d_mind, n, s));
    }
  }
  SFM_RC(w.d_best_cen.download(centers, (size_t)K * dim, s));
  if (labels) SFM_RC(w.d_best_labels.download(labels, n, s));
  if (min_dist) SFM_RC(w.d_best_mind.download(min_dist, n, s));
  SFM_HIP(hipStreamSynchronize(s));
  if (compactness) *compactness = best;
  if (iterations) *iterations = n_iter;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_bowtrain_destroy(sfmloc_bowtrain *p) {
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  if (!t) return;
  hipSetDevice(t->device);
  if (t->s) (void)hipStreamSynchronize(t->s);
  sfmloc_akaze *ak = t->ak;
  delete t;  // (its buffers go before the extractor's stream, which is the trainer's)
  if (ak) sfmloc_akaze_destroy(ak);
}

int sfmloc_bowtrain_create(int device, uint32_t dim, uint32_t cap_rows, sfmloc_bowtrain **out) {
  SFM_CHECK(out, SFMLOC_EINVAL, "sfmloc_bowtrain_create: null argument");
  *out = nullptr;
  SFM_CHECK(dim >= 1 && dim <= (uint32_t)kTbMaxDim && cap_rows >= 1 && cap_rows <= (1u << 26), SFMLOC_EINVAL,
            "sfmloc_bowtrain_create: dim %u (1..%d), cap_rows %u", dim, kTbMaxDim, cap_rows);
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) SFM_CHECK(false, SFMLOC_ENODEV, "no HIP device");
  SFM_HIP(hipSetDevice(device));
  BowTrain *t = new (std::nothrow) BowTrain();
  SFM_CHECK(t, SFMLOC_ENOMEM, "out of host memory");
  t->device = device;
  t->dim0 = t->dim = dim;
  t->cap = cap_rows;
  // the dense extractor of DenseLocalFeatureWrapper (cv::AKAZE::create() defaults, DenseLocalFeatureWrapper.cpp:42) and
  // its grid (DenseFeatureDetector.cpp:44-69); its own non-blocking stream is the trainer's
  const int size = 300;
  int rc = sfmloc_akaze_create(device, size, size, 4, 4, 0.001f, &t->ak);
  std::vector<float> grid;
  if (!rc) {
    try {
      dense_grid_build(size, &grid, nullptr);  // (imgbow.hip: the query chain's grid)
    } catch (const std::bad_alloc &) {
      sfmloc_bowtrain_destroy(reinterpret_cast<sfmloc_bowtrain *>(t));
      SFM_CHECK(false, SFMLOC_ENOMEM, "sfmloc_bowtrain_create: out of host memory");
    }
    t->n_grid = (uint32_t)(grid.size() / 4);
    t->s = akaze_stream_now(reinterpret_cast<Akaze *>(t->ak));
    rc = dev_upload(nullptr, t->d_grid, grid.data(), grid.size(), t->s);
    if (!rc) rc = t->d_x.alloc(nullptr, (size_t)cap_rows * dim);
    if (!rc) rc = t->d_y.alloc(nullptr, (size_t)cap_rows * dim);
    const hipError_t he = rc ? hipSuccess : hipStreamSynchronize(t->s);
    if (he != hipSuccess) {
      set_error("sfmloc_bowtrain_create: %s", hipGetErrorString(he));
      rc = he == hipErrorOutOfMemory ? SFMLOC_ENOMEM : SFMLOC_EHIP;
    }
  }
  if (rc) {
    sfmloc_bowtrain_destroy(reinterpret_cast<sfmloc_bowtrain *>(t));
    return rc;
  }
  *out = reinterpret_cast<sfmloc_bowtrain *>(t);
  return SFMLOC_OK;
}

int sfmloc_bowtrain_reset(sfmloc_bowtrain *p) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_bowtrain_reset: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  t->n = 0;
  t->dim = t->dim0;
  t->pca_ok = false;
  return SFMLOC_OK;
}

int sfmloc_bowtrain_size(const sfmloc_bowtrain *p, uint32_t *n, uint32_t *dim) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_bowtrain_size: null argument");
  const BowTrain *t = reinterpret_cast<const BowTrain *>(p);
  if (n) *n = t->n;
  if (dim) *dim = t->dim;
  return SFMLOC_OK;
}

int sfmloc_bowtrain_add_rows(sfmloc_bowtrain *p, const float *rows, uint32_t n) {
  SFM_CHECK(p && (rows || n == 0), SFMLOC_EINVAL, "sfmloc_bowtrain_add_rows: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_CHECK(t->dim == t->dim0, SFMLOC_EINVAL, "sfmloc_bowtrain_add_rows: the sample is projected (reset first)");
  SFM_CHECK((uint64_t)t->n + n <= t->cap, SFMLOC_ECAP, "sfmloc_bowtrain_add_rows: %u + %u rows > capacity %u", t->n, n, t->cap);
  if (n == 0) return SFMLOC_OK;
  SFM_HIP(hipSetDevice(t->device));
  SFM_RC(dev_upload(t->d_x + (size_t)t->n * t->dim, rows, (size_t)n * t->dim, t->s));
  SFM_HIP(hipStreamSynchronize(t->s));  // (the caller's rows may go once this returns)
  t->n += n;
  t->pca_ok = false;
  return SFMLOC_OK;
}

int sfmloc_bowtrain_add_image(sfmloc_bowtrain *p, const uint8_t *bgr, uint32_t w, uint32_t h, uint32_t channels,
                              uint32_t n_pick, uint64_t *rng_state) {
  SFM_CHECK(p && rng_state, SFMLOC_EINVAL, "sfmloc_bowtrain_add_image: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_CHECK(t->dim == t->dim0 && t->dim0 == 61, SFMLOC_EINVAL,
            "sfmloc_bowtrain_add_image: the dense rows are 61 M-LDB bytes (sample dim %u)", t->dim);
  SFM_CHECK((uint64_t)t->n + n_pick <= t->cap, SFMLOC_ECAP, "sfmloc_bowtrain_add_image: %u + %u rows > capacity %u", t->n,
            n_pick, t->cap);
  SFM_HIP(hipSetDevice(t->device));
  float *dst = t->d_x + (size_t)t->n * t->dim;
  if (!bgr) {  // no descriptors (TrainBoW.cpp:114-116): the rows stay zero, nothing is drawn
    if (n_pick) SFM_RC(dev_zero(dst, (size_t)n_pick * t->dim, t->s));
    t->n += n_pick;
    t->pca_ok = false;
    return SFMLOC_OK;
  }
  SFM_CHECK(w >= 1 && h >= 1 && w <= 16384 && h <= 16384 && (channels == 1 || channels == 3), SFMLOC_EINVAL,
            "sfmloc_bowtrain_add_image: image %ux%ux%u", w, h, channels);
  const size_t n_src = (size_t)w * h * channels;
  const bool cached = t->last_w == w && t->last_h == h && t->last_c == channels && t->last_img.size() == n_src &&
                      memcmp(t->last_img.data(), bgr, n_src) == 0;
  Akaze *a = reinterpret_cast<Akaze *>(t->ak);
  if (!cached) {
    if (!t->plan_ok || t->plan.w != (int)w || t->plan.h != (int)h || t->plan.channels != (int)channels) {
      SFM_HIP(hipStreamSynchronize(t->s));
      if (t->plan_ok) dense_gray_plan_destroy(&t->plan);
      t->plan_ok = false;
      t->plan = DenseGrayPlan();
      int rc = dense_gray_plan_create(&t->plan, (int)w, (int)h, (int)channels, 300);
      if (rc) return rc;
      t->plan_ok = true;
    }
    if (t->d_src.bytes() < n_src) {
      SFM_HIP(hipStreamSynchronize(t->s));
      const int rc = t->d_src.alloc(nullptr, n_src);
      if (rc) return rc;
    }
    t->last_w = 0;  // (invalid until the extraction is queued)
    SFM_RC(t->d_src.upload(bgr, n_src, t->s));
    int rc = dense_gray_enqueue(&t->plan, t->s, t->d_src, akaze_gray_dev(a));
    if (!rc) rc = akaze_compute_resident(a, t->d_grid, t->n_grid, 4);  // (the grid's four scales are levels 0 .. 3)
    if (rc) return rc;
    t->last_img.assign(bgr, bgr + n_src);
    t->last_w = w;
    t->last_h = h;
    t->last_c = channels;
  }
  if (n_pick == 0) return SFMLOC_OK;
  std::vector<uint32_t> idx(n_pick);
  const uint32_t rows = t->n_grid;
  for (uint32_t j = 0; j < n_pick; ++j) {  // int k = descriptors.rows * randFeature (TrainBoW.cpp:118-119), clamped
    const float r = rng_uniform01(rng_state);
    uint32_t k = (uint32_t)((float)rows * r);
    idx[j] = k < rows ? k : rows - 1;
  }
  if (t->d_idx.bytes() < (size_t)n_pick * sizeof(uint32_t)) {
    SFM_HIP(hipStreamSynchronize(t->s));
    const int rc = t->d_idx.alloc(nullptr, n_pick);
    if (rc) return rc;
  }
  SFM_RC(t->d_idx.upload(idx.data(), n_pick, t->s));
  SFM_RC(dev_launch(k_tb_gather8, dim3((n_pick * t->dim + 255) / 256), dim3(256), 0, t->s, akaze_desc_dev(a), t->d_idx,
                    n_pick, t->dim, dst));
  SFM_HIP(hipStreamSynchronize(t->s));  // (idx is a host vector; the image may be reused by the caller at once)
  t->n += n_pick;
  t->pca_ok = false;
  return SFMLOC_OK;
}

int sfmloc_bowtrain_read(sfmloc_bowtrain *p, float *rows, uint64_t cap_floats) {
  SFM_CHECK(p && rows, SFMLOC_EINVAL, "sfmloc_bowtrain_read: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  const uint64_t need = (uint64_t)t->n * t->dim;
  SFM_CHECK(cap_floats >= need, SFMLOC_ECAP, "sfmloc_bowtrain_read: %llu floats needed", (unsigned long long)need);
  SFM_HIP(hipSetDevice(t->device));
  if (need) SFM_RC(t->d_x.download(rows, need, t->s));
  SFM_HIP(hipStreamSynchronize(t->s));
  return SFMLOC_OK;
}

int sfmloc_bowtrain_pca64(sfmloc_bowtrain *p, double *mean, double *cov, double *eigvec, double *eigval) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_bowtrain_pca64: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_HIP(hipSetDevice(t->device));
  const int rc = tb_moments(t);
  if (rc) return rc;
  const size_t d = t->dim;
  if (mean) memcpy(mean, t->mean.data(), d * sizeof(double));
  if (cov) memcpy(cov, t->cov.data(), d * d * sizeof(double));
  if (eigvec) memcpy(eigvec, t->evec.data(), d * d * sizeof(double));
  if (eigval) memcpy(eigval, t->eval.data(), d * sizeof(double));
  return SFMLOC_OK;
}

int sfmloc_bowtrain_pca(sfmloc_bowtrain *p, float *mean, float *eigvec, float *eigval) {
  SFM_CHECK(p, SFMLOC_EINVAL, "sfmloc_bowtrain_pca: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_HIP(hipSetDevice(t->device));
  const int rc = tb_moments(t);
  if (rc) return rc;
  const size_t d = t->dim;
  for (size_t i = 0; i < d; ++i) {
    if (mean) mean[i] = (float)t->mean[i];
    if (eigval) eigval[i] = (float)t->eval[i];
  }
  if (eigvec)
    for (size_t i = 0; i < d * d; ++i) eigvec[i] = (float)t->evec[i];
  return SFMLOC_OK;
}

int sfmloc_bowtrain_project(sfmloc_bowtrain *p, const sfmloc_bof_desc *pca) {
  SFM_CHECK(p && pca && pca->pca_mean && pca->pca_eigvec && pca->pca_eigval, SFMLOC_EINVAL,
            "sfmloc_bowtrain_project: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_CHECK(pca->in_dim == (int)t->dim && pca->n_pca >= 1 && pca->n_pca <= pca->in_dim, SFMLOC_EINVAL,
            "sfmloc_bowtrain_project: in_dim %d (sample dim %u), n_pca %d", pca->in_dim, t->dim, pca->n_pca);
  SFM_HIP(hipSetDevice(t->device));
  const int in_dim = pca->in_dim, np = pca->n_pca;
  if (!t->d_pmean) {
    DevGroup g(nullptr);
    g.add(t->d_pmean, kTbMaxDim);
    g.add(t->d_pevec, kTbMaxDim * kTbMaxDim);
    g.add(t->d_peval, kTbMaxDim);
    if (!g.ok()) return g.rc();
    g.commit();
  }
  SFM_RC(t->d_pmean.upload(pca->pca_mean, in_dim, t->s));
  SFM_RC(t->d_pevec.upload(pca->pca_eigvec, (size_t)np * in_dim, t->s));
  SFM_RC(t->d_peval.upload(pca->pca_eigval, np, t->s));
  const uint64_t total = (uint64_t)t->n * np;
  if (total)
    SFM_RC(dev_launch(k_tb_project, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, t->s, t->d_x, t->n, in_dim,
                      t->d_pmean, t->d_pevec, t->d_peval, np, t->d_y));
  SFM_HIP(hipStreamSynchronize(t->s));  // (the model arrays are the caller's)
  std::swap(t->d_x, t->d_y);
  t->dim = (uint32_t)np;
  t->pca_ok = false;
  return SFMLOC_OK;
}

int sfmloc_bowtrain_kmeans(sfmloc_bowtrain *p, uint32_t K, uint32_t attempts, uint32_t max_iter, double eps,
                           uint64_t seed, float *centers, int32_t *labels, float *min_dist, double *compactness,
                           uint32_t *iterations) {
  SFM_CHECK(p && centers, SFMLOC_EINVAL, "sfmloc_bowtrain_kmeans: null argument");
  BowTrain *t = reinterpret_cast<BowTrain *>(p);
  SFM_CHECK(t->n >= 1 && K >= 1 && attempts >= 1, SFMLOC_EINVAL, "sfmloc_bowtrain_kmeans: %u rows, K %u, attempts %u", t->n,
            K, attempts);
  const uint32_t Kc = std::min(K, t->n);  // clusterCount = min(K, features.rows) (BoFSpatialPyramids.cpp:99)
  SFM_CHECK((size_t)Kc * t->dim * sizeof(double) + Kc * sizeof(uint32_t) <= 64 * 1024, SFMLOC_EINVAL,
            "sfmloc_bowtrain_kmeans: K %u x dim %u centres exceed the 64 KB workgroup memory of the centre sums", Kc, t->dim);
  SFM_HIP(hipSetDevice(t->device));
  if (t->dim <= 32) return tb_kmeans<32>(t, Kc, attempts, max_iter, eps, seed, centers, labels, min_dist, compactness, iterations);
  return tb_kmeans<64>(t, Kc, attempts, max_iter, eps, seed, centers, labels, min_dist, compactness, iterations);
}

}  // extern "C"
