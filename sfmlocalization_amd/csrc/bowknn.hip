// sfmloc_bow_knn: for every view the k views nearest to it in BoW space -- K8 (bow.hip) asked for all views at once.
// The semantics are stated in include/sfmloc.h ("All-views BoW k-NN"); tests/bowknn_np.py restates them over the C oracle
// and the GPU tests compare bits.
//
//   k_bowknn_dist    a tile of 16 query rows x 16 bank rows per workgroup of four waves.  The bank rows go through LDS in
//                    chunks of 256 elements (16 KB); every wave holds four query rows' elements of the round in registers
//                    (element lane + 64 r of the row, as the oracle's partial `lane` takes them) and sixty-four running
//                    partial sums, one per (query row, bank row) pair of its 4 x 16 sub-tile: each element of `bow` is
//                    read from global memory once per workgroup tile, and each LDS read feeds four pairs.
//                    The sixty-four partials of sixty-four pairs are then reduced across the sixty-four lanes TOGETHER:
//                    at stride 32 a lane keeps the 32 pairs of its own half and hands the other 32 to lane ^ 32, at stride
//                    16 it keeps 16 of those, ... -- 63 cross-lane steps for 64 pairs where a butterfly per pair takes 384.
//                    Lane p ends with pair p's sum, added up along the oracle's tree (partial[l] + partial[l ^ stride],
//                    strides 32 .. 1): float addition is commutative, so which partner holds the running sum changes no bit.
//                    A lane past the end of a row adds +0 to a sum that is never -0: the oracle's lane adds nothing.
//   k_bowknn_select  one workgroup of 1024 per query row over the row's n distances: BowTopkBody (bow_topk_device.h), the
//                    selection K8 uses, with k = count[i]; then the distances of the kept views and the padding.
// Entries of a row that are no candidates (|j - i| <= window) carry 0xFFFFFFFF, above +inf's 0x7F800000.
// -ffp-contract=off: subtract, multiply and add stay three roundings, as in the oracle.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "bow_topk_device.h"
#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint32_t kKnnMaxN = 1u << 22;
constexpr uint64_t kKnnMaxOut = 1ull << 32;          // n * k entries
constexpr uint64_t kKnnScratchEntries = 1ull << 26;  // the default rows_per_launch keeps the scratch at 256 MB
constexpr uint32_t kKnnMaxRows = 1u << 20;           // query rows of one pass
constexpr uint32_t kExcluded = 0xFFFFFFFFu;
constexpr uint32_t kInfBits = 0x7F800000u;

constexpr uint32_t kTile = 16;                    // query rows and bank rows of a workgroup's tile
constexpr uint32_t kWaveRows = 4;                 // query rows of a wave: 4 x 16 = the 64 pairs of its lanes
constexpr uint32_t kChunkRounds = 4;              // rounds of 64 elements staged at once
constexpr uint32_t kChunk = 64 * kChunkRounds;    // = the workgroup's 256 threads: one element of each bank row each

thread_local double g_bowknn_last_ms = 0.0;

// one step of the transposed reduction: in[2 H] -> out[H]; a lane whose `stride` bit is set keeps the upper half
template <int H>
__device__ __forceinline__ void fold(const float (&in)[2 * H], float (&out)[H], uint32_t lane) {
  const bool upper = (lane & (uint32_t)H) != 0;
#pragma unroll
  for (int q = 0; q < H; ++q) {
    const float keep = upper ? in[q + H] : in[q];
    const float send = upper ? in[q] : in[q + H];
    out[q] = keep + __shfl_xor(send, H, 64);
  }
}

// dist_bits[(i - row0) * n + j] for the query rows i in [row0, row0 + rows) and every j
__global__ __launch_bounds__(256) void k_bowknn_dist(const float *__restrict__ bow, uint32_t n, uint32_t dim, uint32_t row0,
                                                     uint32_t rows, uint32_t window, uint32_t *__restrict__ dist_bits) {
  __shared__ float s_bank[kTile][kChunk];
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const uint32_t b0 = blockIdx.x * kTile;
  const uint32_t row_end = row0 + rows;
  const uint32_t q0 = row0 + blockIdx.y * kTile + wave * kWaveRows;
  float acc[64];  // pair qi * 16 + bj
#pragma unroll
  for (int p = 0; p < 64; ++p) acc[p] = 0.0f;
  for (uint32_t c0 = 0; c0 < dim; c0 += kChunk) {
    __syncthreads();  // the chunk before this one has been read
#pragma unroll
    for (uint32_t u = 0; u < kTile; ++u) {
      const uint32_t j = b0 + u, col = c0 + tid;
      s_bank[u][tid] = (j < n && col < dim) ? bow[(size_t)j * dim + col] : 0.0f;
    }
    __syncthreads();
#pragma unroll
    for (uint32_t r = 0; r < kChunkRounds; ++r) {
      if (c0 + 64 * r >= dim) break;  // (the same for every lane)
      const uint32_t col = c0 + 64 * r + lane;
      float q[kWaveRows];
#pragma unroll
      for (uint32_t qi = 0; qi < kWaveRows; ++qi) {
        const uint32_t i = q0 + qi;
        q[qi] = (i < row_end && col < dim) ? bow[(size_t)i * dim + col] : 0.0f;
      }
#pragma unroll
      for (uint32_t bj = 0; bj < kTile; ++bj) {
        const float x = s_bank[bj][64 * r + lane];
#pragma unroll
        for (uint32_t qi = 0; qi < kWaveRows; ++qi) {
          const float d = x - q[qi];
          const float d2 = d * d;
          acc[qi * kTile + bj] = acc[qi * kTile + bj] + d2;
        }
      }
    }
  }
  float t32[32], t16[16], t8[8], t4[4], t2[2], t1[1];
  fold<32>(acc, t32, lane);
  fold<16>(t32, t16, lane);
  fold<8>(t16, t8, lane);
  fold<4>(t8, t4, lane);
  fold<2>(t4, t2, lane);
  fold<1>(t2, t1, lane);
  const uint32_t i = q0 + lane / kTile, j = b0 + lane % kTile;  // lane p holds pair p
  if (i < row_end && j < n) {
    const uint32_t apart = i > j ? i - j : j - i;
    dist_bits[(size_t)(i - row0) * n + j] = apart <= window ? kExcluded : __float_as_uint(t1[0]);
  }
}

// row r of the pass: the count[i] candidates smallest in (distance bits, index), ascending by index, their distances, and
// the padding up to k_out entries
__global__ __launch_bounds__(1024) void k_bowknn_select(const uint32_t *__restrict__ dist_bits, uint32_t n, uint32_t row0,
                                                        uint32_t k, uint32_t k_out, uint32_t window,
                                                        uint32_t *__restrict__ nbr, uint32_t *__restrict__ dist_out) {
  const uint32_t i = row0 + blockIdx.x;
  const uint32_t lo = i > window ? i - window : 0u, hi = min(i + window, n - 1);  // (window < n <= 2^22: no wrap)
  const uint32_t n_cand = n - (hi - lo + 1);
  const uint32_t cnt = min(k, n_cand);
  const uint32_t *row = dist_bits + (size_t)blockIdx.x * n;
  uint32_t *out = nbr + (size_t)blockIdx.x * k_out;
  uint32_t *dout = dist_out + (size_t)blockIdx.x * k_out;
  BowTopkBody::run(row, n, nullptr, cnt, out, ChainArgs{});
  __syncthreads();  // the selection (this workgroup's own global stores) is complete and visible to it
  for (uint32_t s = threadIdx.x; s < k_out; s += 1024) {
    if (s < cnt) {
      dout[s] = row[out[s]];
    } else {
      out[s] = kExcluded;
      dout[s] = kInfBits;
    }
  }
}

// |cand(i)| capped at k
inline uint32_t count_of(uint32_t i, uint32_t n, uint32_t window, uint32_t k) {
  const uint64_t lo = i > window ? i - window : 0u, hi = std::min<uint64_t>((uint64_t)i + window, n - 1);
  return (uint32_t)std::min<uint64_t>(k, n - (hi - lo + 1));
}

uint32_t default_rows(uint32_t n) {
  uint64_t rows = kKnnScratchEntries / n;  // >= 16 at n = 2^22
  if (rows > kTile) rows -= rows % kTile;  // (whole tiles: no pass ends on a partly used one but the last)
  return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(rows, 1), n);
}

int bowknn_impl(CallScope *d, const float *bow, uint32_t n, uint32_t dim, uint32_t k_out, const sfmloc_bowknn_options &o,
                std::vector<uint32_t> *h_nbr, std::vector<uint32_t> *h_dist) {
  // (at most 2^20 rows a pass: the distance grid's second dimension stays below 65 536 tiles)
  const uint32_t per = std::min(o.rows_per_launch ? std::min(o.rows_per_launch, n) : default_rows(n), kKnnMaxRows);
  DevBuf<float> d_bow;
  DevBuf<uint32_t> d_bits, d_nbr, d_dist;
  SFM_RC(dev_upload(nullptr, d_bow, bow, (size_t)n * dim, d->s));
  SFM_RC(d_bits.alloc(nullptr, (size_t)per * n));
  SFM_RC(d_nbr.alloc(nullptr, (size_t)per * k_out));
  SFM_RC(d_dist.alloc(nullptr, (size_t)per * k_out));
  SFM_RC(d->time_begin());
  for (uint32_t row0 = 0; row0 < n; row0 += per) {
    const uint32_t rows = std::min(per, n - row0);
    SFM_RC(dev_launch(k_bowknn_dist, dim3((n + kTile - 1) / kTile, (rows + kTile - 1) / kTile), dim3(256), 0, d->s, d_bow,
                      n, dim, row0, rows, o.window, d_bits));
    SFM_RC(dev_launch(k_bowknn_select, dim3(rows), dim3(1024), 0, d->s, d_bits, n, row0, o.k, k_out, o.window, d_nbr,
                      d_dist));
    SFM_RC(d_nbr.download(h_nbr->data() + (size_t)row0 * k_out, (size_t)rows * k_out, d->s));
    SFM_RC(d_dist.download(h_dist->data() + (size_t)row0 * k_out, (size_t)rows * k_out, d->s));
  }
  SFM_RC(d->time_end());
  SFM_HIP(hipStreamSynchronize(d->s));
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_bowknn_default_options(sfmloc_bowknn_options *o) {
  if (!o) return;
  o->k = 20;
  o->window = 0;
  o->rows_per_launch = 0;
  o->profile = 0;
}

double sfmloc_bowknn_last_ms(void) { return g_bowknn_last_ms; }

int sfmloc_bow_knn(int device, const float *bow, uint32_t n, uint32_t dim, const sfmloc_bowknn_options *opt, uint32_t *nbr,
                   float *dist, uint32_t *count) {
  sfmloc_bowknn_options o;
  if (opt) o = *opt;
  else sfmloc_bowknn_default_options(&o);
  SFM_CHECK(o.k != 0, SFMLOC_EINVAL, "sfmloc_bow_knn: k = 0 (at least 1)");
  SFM_CHECK(dim != 0, SFMLOC_EINVAL, "sfmloc_bow_knn: dim = 0 (at least 1)");
  SFM_CHECK(n <= kKnnMaxN, SFMLOC_ECAP, "sfmloc_bow_knn: %u views (at most 2^22)", n);
  SFM_CHECK((uint64_t)n * o.k <= kKnnMaxOut, SFMLOC_ECAP, "sfmloc_bow_knn: %u views x k = %u: more than 2^32 entries", n, o.k);
  SFM_CHECK(n == 0 || (bow && nbr && dist && count), SFMLOC_EINVAL, "sfmloc_bow_knn: null array");
  for (uint32_t i = 0; i < n; ++i) {
    const float *row = bow + (size_t)i * dim;
    for (uint32_t c = 0; c < dim; ++c)
      SFM_CHECK(std::isfinite(row[c]), SFMLOC_EINVAL, "sfmloc_bow_knn: row %u has a non-finite value", i);
  }
  g_bowknn_last_ms = 0.0;
  const size_t k = o.k;
  if (n < 2 || o.window >= n - 1) {  // no row has a candidate: nothing to launch
    for (size_t e = 0; e < (size_t)n * k; ++e) {
      nbr[e] = kExcluded;
      dist[e] = INFINITY;
    }
    for (uint32_t i = 0; i < n; ++i) count[i] = 0;
    return SFMLOC_OK;
  }
  const uint32_t k_out = (uint32_t)std::min<size_t>(k, n - 1);  // no row keeps more: what the device arrays hold per row
  std::vector<uint32_t> h_nbr, h_dist;
  try {
    h_nbr.resize((size_t)n * k_out);
    h_dist.resize((size_t)n * k_out);
  } catch (const std::bad_alloc &) {
    SFM_CHECK(false, SFMLOC_ENOMEM, "sfmloc_bow_knn: out of host memory for %u x %u results", n, k_out);
  }
  {
    CallScope d;
    int rc;
    if ((rc = CallScope::use_device(device)) || (rc = d.open(o.profile != 0, &g_bowknn_last_ms))) return rc;
    if ((rc = bowknn_impl(&d, bow, n, dim, k_out, o, &h_nbr, &h_dist))) return rc;
  }
  // nothing of the caller's is written before every step has succeeded
  for (uint32_t i = 0; i < n; ++i) {
    memcpy(nbr + i * k, h_nbr.data() + (size_t)i * k_out, (size_t)k_out * sizeof(uint32_t));
    memcpy(dist + i * k, h_dist.data() + (size_t)i * k_out, (size_t)k_out * sizeof(uint32_t));
    for (size_t s = k_out; s < k; ++s) {
      nbr[i * k + s] = kExcluded;
      dist[i * k + s] = INFINITY;
    }
    count[i] = count_of(i, n, o.window, o.k);
  }
  return SFMLOC_OK;
}

}  // extern "C"
