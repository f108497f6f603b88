// Stable LSD radix sort of (key, value) pairs of uint32_t on the device, 8 bits per pass: what adjust.hip's transpose
// (observations by view) and tracks.hip (nodes by component label) share.  Each pass is a per-block digit histogram, one
// exclusive scan over (digit, block) and a scatter whose rank inside the block comes from wave ballots -- no atomic
// decides a position, so two runs give the same order.  Everything is in the anonymous namespace: each translation unit
// compiles its own copy, no device symbol crosses one.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sfmloc_internal.h"

namespace sfmloc {
namespace {

constexpr int kRadixBlock = 1024;  // elements per block of a radix pass (16 waves)

// digit histogram of one block of kRadixBlock elements -> hist[digit * nb + block]
__global__ __launch_bounds__(kRadixBlock) void k_radix_hist(const uint32_t *__restrict__ key, uint32_t n, int shift,
                                                            uint32_t *__restrict__ hist, uint32_t nb) {
  __shared__ uint32_t h[256];
  for (int i = threadIdx.x; i < 256; i += kRadixBlock) h[i] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kRadixBlock + threadIdx.x;
  if (i < n) atomicAdd(&h[(key[i] >> shift) & 255u], 1u);  // (a count: the same whatever the order)
  __syncthreads();
  for (int d = threadIdx.x; d < 256; d += kRadixBlock) hist[(uint32_t)d * nb + blockIdx.x] = h[d];
}

// exclusive prefix sum of a[0..n) in place: one workgroup, chunks of 1024 in order
__global__ __launch_bounds__(1024) void k_scan_excl(uint32_t *__restrict__ a, uint32_t n) {
  __shared__ uint32_t s[1024];
  __shared__ uint32_t carry;
  const int t = threadIdx.x;
  if (t == 0) carry = 0;
  __syncthreads();
  for (uint32_t base = 0; base < n; base += 1024) {
    const uint32_t v = (base + t < n) ? a[base + t] : 0u;
    s[t] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      const uint32_t x = t >= off ? s[t - off] : 0u;
      __syncthreads();
      s[t] += x;
      __syncthreads();
    }
    if (base + t < n) a[base + t] = carry + s[t] - v;
    __syncthreads();
    if (t == 0) carry += s[1023];
    __syncthreads();
  }
}

// stable scatter: an element's place = its digit's offset for this block + the elements of the same digit before it in
// the block (its wave's lanes below it, from a ballot match over the digit's bits, then the earlier waves' counts)
__global__ __launch_bounds__(kRadixBlock) void k_radix_scatter(const uint32_t *__restrict__ kin,
                                                               const uint32_t *__restrict__ vin, uint32_t n, int shift,
                                                               const uint32_t *__restrict__ off, uint32_t nb,
                                                               uint32_t *__restrict__ kout, uint32_t *__restrict__ vout) {
  constexpr int kWaves = kRadixBlock / 64;
  __shared__ uint32_t wc[kWaves][257];  // (digit 256: the lanes past the end)
  for (int i = threadIdx.x; i < kWaves * 257; i += kRadixBlock) (&wc[0][0])[i] = 0;
  __syncthreads();
  const uint32_t i = blockIdx.x * kRadixBlock + threadIdx.x;
  const bool valid = i < n;
  const uint32_t d = valid ? ((kin[i] >> shift) & 255u) : 256u;
  unsigned long long mask = ~0ull;
  for (int b = 0; b < 9; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(bit);
    mask &= bit ? bb : ~bb;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  const uint32_t rank = (uint32_t)__popcll(mask & below);
  if ((mask & below) == 0ull) wc[w][d] = (uint32_t)__popcll(mask);  // the lowest lane of each digit group
  __syncthreads();
  if (!valid) return;
  uint32_t r = rank;
  for (int ww = 0; ww < w; ++ww) r += wc[ww][d];
  const uint32_t dst = off[d * nb + blockIdx.x] + r;
  kout[dst] = kin[i];
  vout[dst] = vin[i];
}

// the key bits a sort has to look at for keys 0..max_key
inline int radix_key_bits(uint32_t max_key) {
  int bits = 0;
  while (bits < 32 && (max_key >> bits) != 0) ++bits;
  return bits;
}

// entries of the histogram scratch a sort of n pairs needs
inline size_t radix_hist_entries(uint64_t n) { return 256 * (size_t)((n + kRadixBlock - 1) / kRadixBlock); }

// sorts n pairs by the low `bits` bits of the key, ping-ponging between (k0, v0) and the scratch pair (k1, v1); hist holds
// radix_hist_entries(n).  *in_scratch: the result ended in (k1, v1).
inline int radix_sort_pairs(uint32_t *k0, uint32_t *v0, uint32_t *k1, uint32_t *v1, uint32_t n, int bits, uint32_t *hist,
                            hipStream_t s, bool *in_scratch) {
  const uint32_t nb = (n + kRadixBlock - 1) / kRadixBlock;
  uint32_t *kin = k0, *vin = v0, *kout = k1, *vout = v1;
  for (int shift = 0; shift < bits && n > 0; shift += 8) {
    SFM_RC(dev_launch(k_radix_hist, dim3(nb), dim3(kRadixBlock), 0, s, kin, n, shift, hist, nb));
    SFM_RC(dev_launch(k_scan_excl, dim3(1), dim3(1024), 0, s, hist, 256u * nb));
    SFM_RC(dev_launch(k_radix_scatter, dim3(nb), dim3(kRadixBlock), 0, s, kin, vin, n, shift, hist, nb, kout, vout));
    uint32_t *t = kin;
    kin = kout;
    kout = t;
    t = vin;
    vin = vout;
    vout = t;
  }
  *in_scratch = kin != k0;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc
