// The exact top-k selection over float32 distance bits that K8 (bow.hip: k_bow_topk, one query's shortlist) and the
// all-views k-NN (bowknn.hip: k_bowknn_select, one workgroup per query row) share: one body, so both give the same
// selection for the same distances.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#include "chain_device.h"

namespace sfmloc {

// exclusive prefix sum of one value per thread over a 1024-thread workgroup (wave shuffles + one LDS hop); every
// thread also gets the grand total
__device__ __forceinline__ uint32_t block_exclusive_scan_1024(uint32_t v, uint32_t *wave_tot /*[16] LDS*/, uint32_t *total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  uint32_t inc = v;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t o = __shfl_up(inc, off, 64);
    if (lane >= (uint32_t)off) inc += o;
  }
  __syncthreads();  // wave_tot of an earlier call is no longer read
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  uint32_t before = 0, tot = 0;
#pragma unroll
  for (uint32_t w = 0; w < 16; ++w) {
    const uint32_t t = wave_tot[w];
    if (w < wave) before += t;
    tot += t;
  }
  *total = tot;
  return before + inc - v;
}

// One 1024-thread workgroup: exact k-th smallest distance by a 3-pass radix select on the float bits
// (11+11+10), then an order-preserving compaction of {dist < T} plus the first (k - #less) of {dist == T}.
// Every search over the histogram and every scan over the per-thread counts is a block-wide scan: the first version
// left them to thread 0 and spent 130 us on 10 000 views, most of it in those loops.
struct BowTopkBody {
  static constexpr int kGangThreads = 1024;
  static __device__ __forceinline__ void run(const uint32_t *__restrict__ dist_bits, uint32_t n,
                                           const uint32_t *__restrict__ cand, uint32_t k,
                                           uint32_t *__restrict__ out_sel, ChainArgs chain) {
    __shared__ uint32_t hist[2048];
    __shared__ uint32_t wave_tot[16];
    __shared__ uint32_t sh_prefix, sh_rank;
    const uint32_t tid = threadIdx.x;
    if (k > n) k = n;
    if (k == 0) return;  // (the launcher never chains an empty shortlist)
    const uint32_t k_sel = k;
    uint32_t prefix = 0, rank = k;  // the k-th smallest (1-based) within the elements matching `prefix`
    const int shifts[3] = {21, 10, 0};
    const uint32_t widths[3] = {11, 11, 10};
    // (up to kRegVals values per thread -- 16 384 views -- are fetched ONCE, side by side, and the three passes count from
    // registers: as a loop over global memory each pass was a chain of n / 1024 load -> LDS-atomic steps, ~6 us of a lone
    // query's 27 us in this kernel per pass)
    constexpr uint32_t kRegVals = 16;
    const bool in_regs = n <= kRegVals * 1024u;
    uint32_t xs[kRegVals];
    if (in_regs) {
#pragma unroll
      for (uint32_t u = 0; u < kRegVals; ++u) xs[u] = tid + 1024u * u < n ? dist_bits[tid + 1024u * u] : 0u;
    }
    for (int pass = 0; pass < 3; ++pass) {
      const uint32_t bins = 1u << widths[pass];
      for (uint32_t b = tid; b < bins; b += 1024) hist[b] = 0;
      __syncthreads();
      const uint32_t hi_shift = shifts[pass] + widths[pass];
      if (in_regs) {
#pragma unroll
        for (uint32_t u = 0; u < kRegVals; ++u) {
          const uint32_t x = xs[u];
          const bool match = (pass == 0) || ((x >> hi_shift) == (prefix >> hi_shift));
          if (tid + 1024u * u < n && match) atomicAdd(&hist[(x >> shifts[pass]) & (bins - 1)], 1u);
        }
      } else {
        for (uint32_t i = tid; i < n; i += 1024) {
          const uint32_t x = dist_bits[i];
          const bool match = (pass == 0) || ((x >> hi_shift) == (prefix >> hi_shift));
          if (match) atomicAdd(&hist[(x >> shifts[pass]) & (bins - 1)], 1u);
        }
      }
      __syncthreads();
      // the bin holding the rank-th element: thread t owns bins 2t, 2t+1 (1024 bins in the last pass: bin t, and 0)
      const uint32_t per = bins / 1024;  // 2 or 1
      const uint32_t h0 = hist[tid * per], h1 = per == 2 ? hist[tid * per + 1] : 0u;
      uint32_t total;
      const uint32_t before = block_exclusive_scan_1024(h0 + h1, wave_tot, &total);
      if (before < rank && rank <= before + h0 + h1) {  // exactly one thread (total >= rank by construction)
        const bool second = rank > before + h0;
        sh_prefix = prefix | ((tid * per + (second ? 1u : 0u)) << shifts[pass]);
        sh_rank = rank - before - (second ? h0 : 0u);
      }
      __syncthreads();
      prefix = sh_prefix;
      rank = sh_rank;
      __syncthreads();
    }
    const uint32_t T = prefix;  // bit pattern of the k-th smallest distance; `rank` of the equal ones are taken
    // contiguous chunk per thread keeps index order
    const uint32_t chunk = (n + 1023) / 1024;
    const uint32_t lo = min(n, tid * chunk), hi = min(n, lo + chunk);
    uint32_t c_eq = 0;
    for (uint32_t i = lo; i < hi; ++i) c_eq += (dist_bits[i] == T);
    uint32_t total;
    const uint32_t eq_before = block_exclusive_scan_1024(c_eq, wave_tot, &total);
    uint32_t c_sel = 0;
    {
      uint32_t e = eq_before;
      for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t x = dist_bits[i];
        if (x < T) ++c_sel;
        else if (x == T) {
          if (e < rank) ++c_sel;
          ++e;
        }
      }
    }
    uint32_t pos = block_exclusive_scan_1024(c_sel, wave_tot, &total);
    uint32_t e = eq_before;
    for (uint32_t i = lo; i < hi; ++i) {
      const uint32_t x = dist_bits[i];
      bool take = x < T;
      if (x == T) {
        take = e < rank;
        ++e;
      }
      if (take) out_sel[pos++] = cand ? cand[i] : i;
    }
    if (chain.keys_out) {  // sharded shortlist: the selection as (distance bits << 32 | global view id), padded
      __syncthreads();
      for (uint32_t i = tid; i < chain.k_out; i += 1024) {
        unsigned long long key = ~0ull;
        if (i < k_sel) {
          const uint32_t v = out_sel[i];
          key = ((unsigned long long)dist_bits[v] << 32) | (unsigned long long)chain.key_view_id[v];
        }
        chain.keys_out[i] = key;
      }
    }
    chain_after_shortlist(chain);  // the query's counters and the block list of the k views (chain_device.h)
  }
};

}  // namespace sfmloc
