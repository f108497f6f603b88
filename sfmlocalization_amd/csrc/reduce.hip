// sfmloc_reduce_points: the device half of reduceClosePointsKDTree (PyEvaluateAccuracy/src/
// localizeGlobalCoordinateRefPoint.py:81-118) -- landmarks closer than `thres` in world coordinates folded into the one of
// lowest index.  The semantics, the readings chosen and the arithmetic are stated in include/sfmloc.h
// ("sfmloc_reduce_points"); tests/globalcoord_np.py restates them over an all-pairs matrix and the GPU tests compare bits.
//
//   global    G = A [X; 1] as k_merge_transform computes it, and the bounding box by integer min / max of the order-
//             preserving bit patterns (exact, so the order of the atomics does not matter).
//   grid      cells of edge h = thres (1 + 2^-10) over the box (the margin keeps a pair with d < thres within one cell
//             of each other whatever the rounding of the cell index).  A cell's 63-bit key is hashed into a power-of-two
//             table of buckets: count / scan / scatter.  The order inside a bucket is whatever the atomics gave; nothing
//             below depends on it (counts, ranks, and lists that are sorted before they are used).
//   close     one lane per point walks its 27 cells twice: a count, then a fill of the row (j > i, d < thres).  A point
//             with more than knn points within thres (itself included) keeps a candidate only if fewer than knn
//             candidates precede it in (distance bits, index).  Rows are then rank-sorted by (distance bits, index).
//   resolve   the transpose of the rows (who lists me), then passes: a point is decided in pass p when every point that
//             lists it was decided in a pass before p (stamps, so a pass never sees its own writes); keeper iff none of
//             them is a keeper, else owned by the smallest keeper.
//   order     per keeper the owned entries of its row in row order, placed by a scan of the counts.
// Every sum of integers here is a count; every float is computed by exactly one expression.  -ffp-contract=off.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr uint64_t kReduceMaxN = 1ull << 24;
constexpr double kReduceMaxCells = 2097152.0;   // 2^21 per axis: three coordinates in one 63-bit key
constexpr uint64_t kReduceMaxPairs = 1ull << 28;
constexpr double kCellMargin = 1.0009765625;    // 1 + 2^-10
constexpr uint32_t kScanItems = 8;              // elements per lane of the scan kernels
constexpr uint32_t kScanChunk = 256 * kScanItems;
constexpr uint32_t kResolvePasses = 8;          // passes per host check when the caller leaves the choice (0)
constexpr uint32_t kNone = 0xFFFFFFFFu;

thread_local double g_reduce_last_ms = 0.0;

struct Mat34 {
  double m[12];
};
struct Grid {
  double lo[3];
  double h;
  uint32_t nc[3];
  uint32_t mask;  // buckets - 1
};

__device__ __forceinline__ uint64_t ordered_bits(double x) {  // a < b  <=>  ordered_bits(a) < ordered_bits(b)
  const uint64_t u = (uint64_t)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

__device__ __forceinline__ uint32_t bucket_of(uint64_t key, uint32_t mask) {  // splitmix64 finaliser
  key ^= key >> 30;
  key *= 0xBF58476D1CE4E5B9ull;
  key ^= key >> 27;
  key *= 0x94D049BB133111EBull;
  key ^= key >> 31;
  return (uint32_t)key & mask;
}

__device__ __forceinline__ uint64_t cell_key(uint32_t cx, uint32_t cy, uint32_t cz) {
  return (uint64_t)cx | ((uint64_t)cy << 21) | ((uint64_t)cz << 42);
}

__device__ __forceinline__ double dist3(double ax, double ay, double az, double bx, double by, double bz) {
  const double dx = ax - bx, dy = ay - by, dz = az - bz;
  return sqrt((dx * dx + dy * dy) + dz * dz);
}

// (distance bits, index) order; distances are >= +0 and finite or +inf, so their bit patterns order as they do
__device__ __forceinline__ bool key_less(uint64_t da, uint32_t ia, uint64_t db, uint32_t ib) {
  return da < db || (da == db && ia < ib);
}

// ---- kernels --------------------------------------------------------------------------------------------------------------

// G = A [X; 1]; box[0..2] = min, box[3..5] = max of the ordered bit patterns
__global__ __launch_bounds__(256) void k_reduce_global(Mat34 T, const double *__restrict__ X, uint32_t n,
                                                       double *__restrict__ G, unsigned long long *__restrict__ box) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  const double *M = T.m;
  unsigned long long lo[3] = {~0ull, ~0ull, ~0ull}, hi[3] = {0ull, 0ull, 0ull};
  if (i < n) {
    const size_t p = 3 * (size_t)i;
    const double x0 = X[p], x1 = X[p + 1], x2 = X[p + 2];
    double g[3];
    g[0] = ((M[0] * x0 + M[1] * x1) + M[2] * x2) + M[3];
    g[1] = ((M[4] * x0 + M[5] * x1) + M[6] * x2) + M[7];
    g[2] = ((M[8] * x0 + M[9] * x1) + M[10] * x2) + M[11];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      G[p + c] = g[c];
      lo[c] = hi[c] = ordered_bits(g[c]);
    }
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned long long a = __shfl_xor(lo[c], off, 64), b = __shfl_xor(hi[c], off, 64);
      lo[c] = a < lo[c] ? a : lo[c];
      hi[c] = b > hi[c] ? b : hi[c];
    }
  }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      atomicMin(&box[c], lo[c]);
      atomicMax(&box[3 + c], hi[c]);
    }
  }
}

__device__ __forceinline__ uint32_t cell_coord(double g, double lo, double h, uint32_t nc) {
  const double q = (g - lo) / h;  // >= 0: lo is the minimum of the same values
  const uint32_t c = (uint32_t)q;
  return c < nc ? c : nc - 1;
}

// a point's cell key and the size of its bucket
__global__ __launch_bounds__(256) void k_reduce_cell(Grid gr, const double *__restrict__ G, uint32_t n,
                                                     uint64_t *__restrict__ key, uint32_t *__restrict__ count) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const size_t p = 3 * (size_t)i;
  const uint64_t k = cell_key(cell_coord(G[p], gr.lo[0], gr.h, gr.nc[0]), cell_coord(G[p + 1], gr.lo[1], gr.h, gr.nc[1]),
                              cell_coord(G[p + 2], gr.lo[2], gr.h, gr.nc[2]));
  key[i] = k;
  atomicAdd(&count[bucket_of(k, gr.mask)], 1u);  // (a count: the same whatever the order)
}

// exclusive scan, level 1: each workgroup scans kScanChunk elements in place and leaves their sum in sums[block]
__global__ __launch_bounds__(256) void k_reduce_scan_chunk(uint32_t *__restrict__ v, uint32_t n, uint32_t *__restrict__ sums) {
  __shared__ uint32_t part[256];
  const uint32_t t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * kScanChunk + (size_t)t * kScanItems;
  uint32_t x[kScanItems], s = 0;
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; ++k) {
    x[k] = base + k < n ? v[base + k] : 0u;
    s += x[k];
  }
  part[t] = s;
  __syncthreads();
  for (uint32_t off = 1; off < 256; off <<= 1) {
    const uint32_t a = t >= off ? part[t - off] : 0u;
    __syncthreads();
    part[t] += a;
    __syncthreads();
  }
  uint32_t run = part[t] - s;  // exclusive prefix of this lane's elements
#pragma unroll
  for (uint32_t k = 0; k < kScanItems; ++k) {
    if (base + k < n) v[base + k] = run;
    run += x[k];
  }
  if (t == 255) sums[blockIdx.x] = part[255];
}

__global__ __launch_bounds__(256) void k_reduce_scan_add(uint32_t *__restrict__ v, uint32_t n, const uint32_t *__restrict__ sums) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < n) v[i] += sums[i / kScanChunk];
}

// a point's place in its bucket; the sorted copies (coordinates, key, index) that the walks read
__global__ __launch_bounds__(256) void k_reduce_scatter(Grid gr, const double *__restrict__ G, const uint64_t *__restrict__ key,
                                                        uint32_t n, const uint32_t *__restrict__ start,
                                                        uint32_t *__restrict__ fill, double *__restrict__ sG,
                                                        uint64_t *__restrict__ skey, uint32_t *__restrict__ sidx) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  const uint32_t b = bucket_of(k, gr.mask);
  const uint32_t pos = start[b] + atomicAdd(&fill[b], 1u);  // (any order inside a bucket: see the header)
  sG[3 * (size_t)pos] = G[3 * (size_t)i];
  sG[3 * (size_t)pos + 1] = G[3 * (size_t)i + 1];
  sG[3 * (size_t)pos + 2] = G[3 * (size_t)i + 2];
  skey[pos] = k;
  sidx[pos] = i;
}

// f(j, distance bits) for every point j (i itself included) of the 27 cells around (cx, cy, cz) with d(i, j) < thres
template <class F>
__device__ __forceinline__ void for_each_within(const Grid &gr, const uint32_t *__restrict__ start,
                                                const double *__restrict__ sG, const uint64_t *__restrict__ skey,
                                                const uint32_t *__restrict__ sidx, uint64_t key, double gx, double gy,
                                                double gz, double thres, F f) {
  const uint32_t cx = (uint32_t)(key & 0x1FFFFFu), cy = (uint32_t)((key >> 21) & 0x1FFFFFu), cz = (uint32_t)(key >> 42);
  for (int dz = -1; dz <= 1; ++dz) {
    const uint32_t z = cz + (uint32_t)dz;  // (wraps below 0: then >= nc)
    if (z >= gr.nc[2]) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const uint32_t y = cy + (uint32_t)dy;
      if (y >= gr.nc[1]) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const uint32_t x = cx + (uint32_t)dx;
        if (x >= gr.nc[0]) continue;
        const uint64_t k = cell_key(x, y, z);
        const uint32_t b = bucket_of(k, gr.mask);
        const uint32_t e1 = start[b + 1];
        for (uint32_t e = start[b]; e < e1; ++e) {
          if (skey[e] != k) continue;  // (another cell of the same bucket)
          const double d = dist3(gx, gy, gz, sG[3 * (size_t)e], sG[3 * (size_t)e + 1], sG[3 * (size_t)e + 2]);
          if (d < thres) f(sidx[e], (uint64_t)__double_as_longlong(d));
        }
      }
    }
  }
}

// C(i): the row of point i.  FILL = false counts it into rowcnt[i]; FILL = true writes it (unsorted) at rowoff[i].
template <bool FILL>
__global__ __launch_bounds__(256) void k_reduce_rows(Grid gr, const double *__restrict__ G, const uint64_t *__restrict__ key,
                                                     uint32_t n, double thres, uint32_t knn,
                                                     const uint32_t *__restrict__ start, const double *__restrict__ sG,
                                                     const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
                                                     uint32_t *__restrict__ rowcnt, const uint32_t *__restrict__ rowoff,
                                                     uint32_t *__restrict__ col, uint64_t *__restrict__ dbits) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint64_t k = key[i];
  const double gx = G[3 * (size_t)i], gy = G[3 * (size_t)i + 1], gz = G[3 * (size_t)i + 2];
  uint32_t within = 0;  // points within thres, i included
  for_each_within(gr, start, sG, skey, sidx, k, gx, gy, gz, thres, [&](uint32_t, uint64_t) { ++within; });
  const bool capped = within > knn;  // N(i) is then the knn smallest of them by (distance bits, index)
  uint32_t m = 0;
  const uint32_t at = FILL ? rowoff[i] : 0u;
  for_each_within(gr, start, sG, skey, sidx, k, gx, gy, gz, thres, [&](uint32_t j, uint64_t dj) {
    if (j <= i) return;
    if (capped) {
      uint32_t before = 0;
      for_each_within(gr, start, sG, skey, sidx, k, gx, gy, gz, thres,
                      [&](uint32_t q, uint64_t dq) { before += key_less(dq, q, dj, j) ? 1u : 0u; });
      if (before >= knn) return;
    }
    if (FILL) {
      col[at + m] = j;
      dbits[at + m] = dj;
    }
    ++m;
  });
  if (!FILL) rowcnt[i] = m;
}

// rows into (distance bits, index) order: an entry's place is the number of entries of its row below it (keys are
// distinct: the indices are).  Counts how many rows list each point.
__global__ __launch_bounds__(256) void k_reduce_rowsort(uint32_t n, const uint32_t *__restrict__ rowoff,
                                                        const uint32_t *__restrict__ col_in, const uint64_t *__restrict__ d_in,
                                                        uint32_t *__restrict__ col, uint64_t *__restrict__ dbits,
                                                        uint32_t *__restrict__ indeg) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const uint32_t e0 = rowoff[i], e1 = rowoff[i + 1];
  for (uint32_t e = e0; e < e1; ++e) {
    const uint32_t j = col_in[e];
    const uint64_t dj = d_in[e];
    uint32_t r = 0;
    for (uint32_t q = e0; q < e1; ++q) r += key_less(d_in[q], col_in[q], dj, j) ? 1u : 0u;
    col[e0 + r] = j;
    dbits[e0 + r] = dj;
    atomicAdd(&indeg[j], 1u);
  }
}

// the transpose: rlist[roff[j] ..] = the points whose rows list j (any order: only a minimum is taken over it)
__global__ __launch_bounds__(256) void k_reduce_transpose(uint32_t n, const uint32_t *__restrict__ rowoff,
                                                          const uint32_t *__restrict__ col, const uint32_t *__restrict__ roff,
                                                          uint32_t *__restrict__ rfill, uint32_t *__restrict__ rlist) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  for (uint32_t e = rowoff[i]; e < rowoff[i + 1]; ++e) {
    const uint32_t j = col[e];
    rlist[roff[j] + atomicAdd(&rfill[j], 1u)] = i;
  }
}

// pass `pass` (from 1): an undecided point whose listers were all decided before this pass is decided now.
// stamp[i] = the pass that decided i (0 = undecided); a stamp written in this pass reads as undecided.
__global__ __launch_bounds__(256) void k_reduce_resolve(uint32_t n, uint32_t pass, const uint32_t *__restrict__ roff,
                                                        const uint32_t *__restrict__ rlist, const double *__restrict__ G,
                                                        uint32_t *stamp, uint32_t *owner, double *__restrict__ dist,
                                                        uint32_t *__restrict__ state /* {undecided, rounds} */) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n || stamp[i] != 0u) return;
  uint32_t keeper = kNone;
  for (uint32_t e = roff[i]; e < roff[i + 1]; ++e) {
    const uint32_t k = rlist[e];
    const uint32_t s = __hip_atomic_load(&stamp[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (s == 0u || s >= pass) return;
    if (owner[k] == k && k < keeper) keeper = k;  // (written in an earlier launch)
  }
  if (keeper == kNone) {
    owner[i] = i;
    dist[i] = 0.0;
  } else {
    owner[i] = keeper;
    dist[i] = dist3(G[3 * (size_t)keeper], G[3 * (size_t)keeper + 1], G[3 * (size_t)keeper + 2], G[3 * (size_t)i],
                    G[3 * (size_t)i + 1], G[3 * (size_t)i + 2]);
  }
  __hip_atomic_store(&stamp[i], pass, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicSub(&state[0], 1u);
  atomicMax(&state[1], pass);
}

// FILL = false: owned[i] = the entries of row i that i owns; FILL = true: they go to order[] from ooff[i], in row order
template <bool FILL>
__global__ __launch_bounds__(256) void k_reduce_order(uint32_t n, const uint32_t *__restrict__ rowoff,
                                                      const uint32_t *__restrict__ col, const uint32_t *__restrict__ owner,
                                                      uint32_t *__restrict__ owned, const uint32_t *__restrict__ ooff,
                                                      uint32_t *__restrict__ order) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  uint32_t m = 0;
  const uint32_t at = FILL ? ooff[i] : 0u;
  if (owner[i] == i)
    for (uint32_t e = rowoff[i]; e < rowoff[i + 1]; ++e) {
      const uint32_t j = col[e];
      if (owner[j] != i) continue;
      if (FILL) order[at + m] = j;
      ++m;
    }
  if (!FILL) owned[i] = m;
}

// ---- host ---------------------------------------------------------------------------------------------------------------

int zeros(CallScope *d, DevBuf<uint32_t> &b, size_t n) {
  const int rc = b.alloc(nullptr, n);
  if (rc) return rc;
  SFM_RC(b.zero(n, d->s));
  return SFMLOC_OK;
}

inline dim3 lanes(uint64_t n) { return dim3((uint32_t)((n + 255) / 256)); }

// v[0..n) becomes its exclusive prefix sums, in place (n <= 2^26: three levels of kScanChunk).  sums: the caller's, one
// array of partial sums per level, which the kernels read after this has returned
constexpr int kScanLevels = 3;
int scan_exclusive(CallScope *d, uint32_t *v, uint32_t n, DevBuf<uint32_t> *sums) {
  if (n == 0) return SFMLOC_OK;
  const uint32_t blocks = (n + kScanChunk - 1) / kScanChunk;
  const int rc = sums->alloc(nullptr, blocks);
  if (rc) return rc;
  SFM_RC(dev_launch(k_reduce_scan_chunk, dim3(blocks), dim3(256), 0, d->s, v, n, sums->get()));
  if (blocks > 1) {
    const int rc2 = scan_exclusive(d, *sums, blocks, sums + 1);
    if (rc2) return rc2;
    SFM_RC(dev_launch(k_reduce_scan_add, lanes(n), dim3(256), 0, d->s, v, n, sums->get()));
  }
  return SFMLOC_OK;
}

bool all_finite(const double *x, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!std::isfinite(x[i])) return false;
  return true;
}

double from_ordered(uint64_t u) {
  u = (u >> 63) ? (u & 0x7FFFFFFFFFFFFFFFull) : ~u;
  double x;
  memcpy(&x, &u, 8);
  return x;
}

int reduce_impl(CallScope *d, const sfmloc_merge_params &p, const double *X, uint32_t n, const Mat34 &T, double thres, uint32_t knn,
                uint32_t *owner, uint32_t *order, double *dist, sfmloc_reduce_result *out) {
  int rc;
#define RDC_TRY(x)     \
  do {                 \
    rc = (x);          \
    if (rc) return rc; \
  } while (0)
  DevBuf<double> dX, dG, dsG, d_dist;
  DevBuf<unsigned long long> d_box;
  DevBuf<uint64_t> d_key, d_skey, d_dtmp, d_dbits;
  DevBuf<uint32_t> d_start, d_fill, d_sidx, d_rowoff, d_ctmp, d_col, d_roff, d_rfill, d_rlist, d_stamp, d_owner, d_state,
      d_ooff, d_order, scan_tmp[4][kScanLevels];
  RDC_TRY(dev_upload(nullptr, dX, X, 3 * (size_t)n, d->s));
  RDC_TRY(dG.alloc(nullptr, 3 * (size_t)n));
  RDC_TRY(d_box.alloc(nullptr, 6));
  SFM_RC(d_box.fill(0xFF, 3, d->s));
  SFM_RC(d_box.zero(3, d->s, 3));
  RDC_TRY(d->time_begin());
  SFM_RC(dev_launch(k_reduce_global, lanes(n), dim3(256), 0, d->s, T, dX, n, dG, d_box));
  unsigned long long box[6];
  SFM_RC(d_box.download(box, 6, d->s));
  SFM_HIP(hipStreamSynchronize(d->s));

  Grid gr;
  gr.h = thres * kCellMargin;
  for (int c = 0; c < 3; ++c) {
    gr.lo[c] = from_ordered(box[c]);
    const double q = (from_ordered(box[3 + c]) - gr.lo[c]) / gr.h;
    SFM_CHECK(q < kReduceMaxCells, SFMLOC_ECAP,
              "sfmloc_reduce_points: axis %d spans %g cells of %g (at most 2^21; a non-finite world coordinate also ends here)",
              c, q, gr.h);
    gr.nc[c] = (uint32_t)q + 1u;
  }
  uint32_t buckets = 1024;
  while (buckets < n) buckets <<= 1;
  gr.mask = buckets - 1;

  RDC_TRY(d_key.alloc(nullptr, n));
  RDC_TRY(zeros(d, d_start, (size_t)buckets + 1));
  SFM_RC(dev_launch(k_reduce_cell, lanes(n), dim3(256), 0, d->s, gr, dG, n, d_key, d_start));
  RDC_TRY(scan_exclusive(d, d_start, buckets + 1, scan_tmp[0]));
  RDC_TRY(zeros(d, d_fill, buckets));
  RDC_TRY(dsG.alloc(nullptr, 3 * (size_t)n));
  RDC_TRY(d_skey.alloc(nullptr, n));
  RDC_TRY(d_sidx.alloc(nullptr, n));
  SFM_RC(dev_launch(k_reduce_scatter, lanes(n), dim3(256), 0, d->s, gr, dG, d_key, n, d_start, d_fill, dsG, d_skey,
                    d_sidx));

  RDC_TRY(zeros(d, d_rowoff, (size_t)n + 1));
  SFM_RC(dev_launch(HIP_KERNEL_NAME(k_reduce_rows<false>), lanes(n), dim3(256), 0, d->s, gr, dG, d_key, n, thres, knn,
                    d_start, dsG, d_skey, d_sidx, d_rowoff, nullptr, nullptr, nullptr));
  // (row counts sum to at most n (knn - 1) or n (n - 1) / 2: the total may pass 2^32, so it is added up here in 64 bits
  // before the 32-bit scan runs)
  std::vector<uint32_t> rowcnt(n);
  SFM_RC(d_rowoff.download(rowcnt.data(), n, d->s));
  SFM_HIP(hipStreamSynchronize(d->s));
  uint64_t n_pairs = 0;
  for (uint32_t i = 0; i < n; ++i) n_pairs += rowcnt[i];
  SFM_CHECK(n_pairs <= kReduceMaxPairs, SFMLOC_ECAP, "sfmloc_reduce_points: %llu close pairs (at most 2^28)",
            (unsigned long long)n_pairs);
  RDC_TRY(scan_exclusive(d, d_rowoff, n + 1, scan_tmp[1]));
  const size_t pairs1 = n_pairs ? n_pairs : 1;  // (no close pair: the arrays still have an address)
  RDC_TRY(d_ctmp.alloc(nullptr, pairs1));
  RDC_TRY(d_dtmp.alloc(nullptr, pairs1));
  RDC_TRY(d_col.alloc(nullptr, pairs1));
  RDC_TRY(d_dbits.alloc(nullptr, pairs1));
  SFM_RC(dev_launch(HIP_KERNEL_NAME(k_reduce_rows<true>), lanes(n), dim3(256), 0, d->s, gr, dG, d_key, n, thres, knn,
                    d_start, dsG, d_skey, d_sidx, nullptr, d_rowoff, d_ctmp, d_dtmp));
  RDC_TRY(zeros(d, d_roff, (size_t)n + 1));
  SFM_RC(dev_launch(k_reduce_rowsort, lanes(n), dim3(256), 0, d->s, n, d_rowoff, d_ctmp, d_dtmp, d_col, d_dbits,
                    d_roff));
  RDC_TRY(scan_exclusive(d, d_roff, n + 1, scan_tmp[2]));
  RDC_TRY(zeros(d, d_rfill, n));
  RDC_TRY(d_rlist.alloc(nullptr, pairs1));
  SFM_RC(dev_launch(k_reduce_transpose, lanes(n), dim3(256), 0, d->s, n, d_rowoff, d_col, d_roff, d_rfill, d_rlist));

  RDC_TRY(zeros(d, d_stamp, n));
  RDC_TRY(d_owner.alloc(nullptr, n));
  RDC_TRY(d_dist.alloc(nullptr, n));
  RDC_TRY(d_state.alloc(nullptr, 2));
  uint32_t state[2] = {n, 0};
  SFM_RC(d_state.upload(state, 2, d->s));
  const uint32_t per = p.rounds_per_launch ? p.rounds_per_launch : kResolvePasses;
  for (uint32_t pass = 1; state[0] != 0;) {  // each pass decides at least the smallest undecided index
    for (uint32_t k = 0; k < per; ++k, ++pass) {
      SFM_RC(dev_launch(k_reduce_resolve, lanes(n), dim3(256), 0, d->s, n, pass, d_roff, d_rlist, dG, d_stamp, d_owner,
                        d_dist, d_state));
    }
    SFM_RC(d_state.download(state, 2, d->s));
    SFM_HIP(hipStreamSynchronize(d->s));
    SFM_CHECK(pass <= n + per, SFMLOC_EHIP, "sfmloc_reduce_points: %u points undecided after %u passes", state[0], pass - 1);
  }

  RDC_TRY(zeros(d, d_ooff, (size_t)n + 1));
  RDC_TRY(d_order.alloc(nullptr, n));
  SFM_RC(d_order.fill(0xFF, n, d->s));
  SFM_RC(dev_launch(HIP_KERNEL_NAME(k_reduce_order<false>), lanes(n), dim3(256), 0, d->s, n, d_rowoff, d_col, d_owner,
                    d_ooff, nullptr, nullptr));
  RDC_TRY(scan_exclusive(d, d_ooff, n + 1, scan_tmp[3]));
  SFM_RC(dev_launch(HIP_KERNEL_NAME(k_reduce_order<true>), lanes(n), dim3(256), 0, d->s, n, d_rowoff, d_col, d_owner,
                    nullptr, d_ooff, d_order));
  RDC_TRY(d->time_end());
  // the outputs, into the call's own buffers first: nothing of the caller's is written before every step has succeeded
  std::vector<uint32_t> h_owner(n), h_order(n);
  std::vector<double> h_dist(n);
  uint32_t n_absorbed = 0;
  SFM_RC(d_owner.download(h_owner.data(), n, d->s));
  SFM_RC(d_order.download(h_order.data(), n, d->s));
  SFM_RC(d_dist.download(h_dist.data(), n, d->s));
  SFM_RC(d_ooff.download(&n_absorbed, 1, d->s, n));
  SFM_HIP(hipStreamSynchronize(d->s));
  memcpy(owner, h_owner.data(), (size_t)n * sizeof(uint32_t));
  memcpy(order, h_order.data(), (size_t)n * sizeof(uint32_t));
  memcpy(dist, h_dist.data(), (size_t)n * sizeof(double));
  out->n_keep = n - n_absorbed;
  out->n_absorbed = n_absorbed;
  out->n_pairs = n_pairs;
  out->rounds = state[1];
  out->reserved = 0;
#undef RDC_TRY
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

double sfmloc_reduce_last_ms(void) { return g_reduce_last_ms; }

int sfmloc_reduce_points(const double *X, uint64_t n, const double *A, double thres, uint32_t knn,
                         const sfmloc_merge_params *params, uint32_t *owner, uint32_t *order, double *dist,
                         sfmloc_reduce_result *out) {
  SFM_CHECK(out, SFMLOC_EINVAL, "sfmloc_reduce_points: null result");
  SFM_CHECK(n <= kReduceMaxN, SFMLOC_ECAP, "sfmloc_reduce_points: %llu points (at most 2^24)", (unsigned long long)n);
  SFM_CHECK(std::isfinite(thres) && thres > 0.0, SFMLOC_EINVAL, "sfmloc_reduce_points: threshold %g (finite and > 0)", thres);
  SFM_CHECK(n == 0 || (X && owner && order && dist), SFMLOC_EINVAL, "sfmloc_reduce_points: null array");
  SFM_CHECK(all_finite(X, 3 * (size_t)n), SFMLOC_EINVAL, "sfmloc_reduce_points: a coordinate is not finite");
  SFM_CHECK(!A || all_finite(A, 12), SFMLOC_EINVAL, "sfmloc_reduce_points: an entry of A is not finite");
  g_reduce_last_ms = 0.0;
  if (n < 2) {  // nothing to absorb (the reference's query fails on k = 1)
    if (n == 1) {
      owner[0] = 0;
      order[0] = kNone;
      dist[0] = 0.0;
    }
    memset(out, 0, sizeof *out);
    out->n_keep = n;
    return SFMLOC_OK;
  }
  Mat34 T = {{1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0}};
  if (A) memcpy(T.m, A, sizeof T.m);
  sfmloc_merge_params p;
  if (params) p = *params;
  else sfmloc_merge_default_params(&p);
  CallScope d;
  int rc;
  if ((rc = CallScope::use_device(p.device)) || (rc = d.open(p.profile, &g_reduce_last_ms))) return rc;
  return reduce_impl(&d, p, X, (uint32_t)n, T, thres, knn, owner, order, dist, out);
}

}  // extern "C"
