// LAB -- would the matrix cores beat the popcount kernel at exact Hamming 2-NN?  The legs at the end
// (fp4 / screening) are what k_hamming_screen_mfma (hamming.hip) was decided on: profiles/k1mfma_lab.jsonl.
// Hamming(a, b) over the 486 valid bits = (486 - <a', b'>) / 2 with a', b' the bits as
// +-1 bytes (the query's padding bits as 0), so a 32 x 32 tile of distances is 16 x v_mfma_i32_32x32x32_i8 (K = 512)
// and the running top-2 per bank row works on the accumulators: lane (l & 31) holds the bank row's column, its 16
// registers are 16 query rows.  Per pair that leaves five VALU lane-ops -- key = ((486 << 15) | q) - (dot << 15)
// (shift + subtract), then the running top-2 (min, max, min) -- five lane-ops against 22 in k_hamming_screen.
//   functional: one wave per 32 bank rows, operands expanded from the bit rows in the kernel; (best, second) keys of every
//               bank row compared with the CPU's exact popcount top-2 (lower query index wins ties)
//   ceiling:    the same inner loop (16 MFMAs + the 48-instruction epilogue per 32 x 32 tile) on register operands, 1 / 2
//               / 4 waves per SIMD on every SIMD: pairs/s when operand delivery is free -- what a finished kernel could
//               at most reach; delivery (LDS-staged query tiles, a 2 x 2 register block per wave) is not written
//   fp4 functional: every distance of a 4 096 x 1 000 problem over all 512 stored bits through
//               v_mfma_scale_f32_32x32x64_f8f6f4 (e2m1 +-1, scales 2^0, operands by k1_mfma_expand.h) vs CPU popcount
//   screening ceiling: fp4 (8 MFMA per 32 x 32 tile) and int8 (16), the streamed operand read from LDS in bit form and
//               expanded per use (7 / 8 VALU per MFMA), two bank tiles per wave, epilogue = running maximum
//               (8 x v_max3 per tile): what a screening kernel could at most reach at 1 / 2 / 4 waves per SIMD.  The
//               fp4 leg runs twice: with the expansion's +1 constant as a literal (the compiler splits every and-or:
//               10 VALU per descriptor dword) and in a register as the product kernel holds it (7).  The int8 leg is
//               a RATE probe only: its streamed operand is 0 / 1 bytes, it does not compute Hamming distances.
// build: hipcc --offload-arch=gfx950 -O3 -o tools/mfma_hamming_lab tools/mfma_hamming_lab.hip ; run on the GPU box
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../sfmlocalization_amd/csrc/k1_mfma_expand.h"

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

// 4 bits -> 4 bytes: bit set -> +1, clear -> -1
__device__ __forceinline__ uint32_t pm1_bytes(uint32_t nib) {
  const uint32_t spread = ((nib & 0xFu) * 0x00204081u) & 0x01010101u;  // bit i -> byte i (0 / 1)
  return 0xFFFFFFFFu ^ (spread * 0xFEu);                               // 1 -> 0x01, 0 -> 0xFF
}
// 16 bits -> 16 bytes of +-1; valid: mask of the bits that count (others -> 0)
__device__ __forceinline__ v4i expand16(uint32_t bits16, uint32_t valid16) {
  v4i r;
  for (int g = 0; g < 4; ++g) {
    const uint32_t b = pm1_bytes(bits16 >> (4 * g));
    const uint32_t m = (((valid16 >> (4 * g)) & 0xFu) * 0x00204081u) & 0x01010101u;
    r[g] = (int)(b & (m * 0xFFu));
  }
  return r;
}

// running top-2 on the key: b1 = med3(b0, b1, key); b0 = min(b0, key)
__device__ __forceinline__ void push(uint32_t &b0, uint32_t &b1, uint32_t key) {
  const uint32_t lo = min(b0, key), hi = max(b0, key);
  b1 = min(b1, hi);
  b0 = lo;
}

// bank [n_bank x 16 dwords], query [n_q x 16 dwords] (rows of 64 bytes, padding zero) -> out[n_bank] = (best, second) keys
__global__ __launch_bounds__(64) void k_functional(const uint32_t *__restrict__ bank, const uint32_t *__restrict__ query,
                                                   int n_q, uint2 *__restrict__ out) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int brow = blockIdx.x * 32 + r;
  v4i B[16];
  for (int s = 0; s < 16; ++s) {
    const uint32_t w = bank[(size_t)brow * 16 + s];
    B[s] = expand16((w >> (16 * h)) & 0xFFFFu, 0xFFFFu);  // the bank's padding bits may be anything: the query's are 0
  }
  uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;
  for (int q0 = 0; q0 < n_q; q0 += 32) {
    v16i acc = {0};
    const int qrow = min(q0 + r, n_q - 1);
    for (int s = 0; s < 16; ++s) {
      const uint32_t w = query[(size_t)qrow * 16 + s];
      // valid bits: 486 = 15 dwords + 6 bits
      const uint32_t vmask = s < 15 ? 0xFFFFFFFFu : 0x3Fu;
      const v4i A = expand16((w >> (16 * h)) & 0xFFFFu, (vmask >> (16 * h)) & 0xFFFFu);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B[s], acc, 0, 0, 0);
    }
    for (int reg = 0; reg < 16; ++reg) {
      const int m = (reg & 3) + 8 * (reg >> 2) + 4 * h;  // the query row of this accumulator
      const int q = q0 + m;
      if (q < n_q) {
        const uint32_t key = (uint32_t)(((486 << 15) | q) - (acc[reg] << 15));
        push(b0, b1, key);
      }
    }
  }
  // lanes l and l + 32 hold the same bank row: merge
  const uint32_t o0 = __shfl_xor(b0, 32, 64), o1 = __shfl_xor(b1, 32, 64);
  push(b0, b1, o0);
  push(b0, b1, o1);
  if (h == 0) out[brow] = make_uint2(b0, b1);
}

// the inner loop on register operands: `tiles` 32 x 32 tiles per wave
template <int EPI>
__global__ __launch_bounds__(256) void k_ceiling(int tiles, uint32_t seed, uint2 *__restrict__ sink) {
  v4i A[4], B[4];
  for (int i = 0; i < 4; ++i)
    for (int g = 0; g < 4; ++g) {
      A[i][g] = (int)pm1_bytes(seed * 2654435761u + threadIdx.x * 97u + i * 13u + g);
      B[i][g] = (int)pm1_bytes(seed * 40503u + threadIdx.x * 31u + i * 7u + g);
    }
  uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;
  int qbase = (486 << 15);
  for (int t = 0; t < tiles; ++t) {
    v16i acc = {0};
#pragma unroll
    for (int s = 0; s < 16; ++s) acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(A[s & 3], B[(s >> 2) & 3], acc, 0, 0, 0);
    if (EPI) {
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const uint32_t key = (uint32_t)((qbase + reg) - (acc[reg] << 15));
        push(b0, b1, key);
      }
    } else {
      b0 ^= (uint32_t)acc[0];
    }
    qbase += 32;
    A[t & 3][0] ^= (int)b0 & 0x01010101;  // (keeps the loop from being hoisted; one VALU per tile)
  }
  if (b0 == 0x12345678u) sink[0] = make_uint2(b0, b1);
}


// ---- fp4 form -------------------------------------------------------------------------------------------------------
__device__ __forceinline__ v8i fp4_operand(uint32_t w, uint32_t all_plus_one = sfmloc::kE2m1AllPlusOne) {
  uint32_t e[4];
  sfmloc::k1_mfma_expand(w, e, all_plus_one);
  v8i r = {(int)e[0], (int)e[1], (int)e[2], (int)e[3], 0, 0, 0, 0};
  return r;
}
__device__ __forceinline__ v16f mfma_fp4(v8i a, v8i b, v16f c) {
  return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, 0x7F7F7F7F, 0, 0x7F7F7F7F);
}

// one wave per 32 bank rows; dist[bank row][query row] (n_q a multiple of 32) over all 512 bits
__global__ __launch_bounds__(64) void k_functional_fp4(const uint32_t *__restrict__ bank, const uint32_t *__restrict__ query,
                                                       int n_q, uint16_t *__restrict__ dist) {
  const int lane = threadIdx.x, r = lane & 31, h = lane >> 5;
  const int brow = blockIdx.x * 32 + r;
  v8i B[8];
  for (int s = 0; s < 8; ++s) B[s] = fp4_operand(bank[(size_t)brow * 16 + sfmloc::k1_mfma_dword_of_step(h, s)]);
  for (int q0 = 0; q0 < n_q; q0 += 32) {
    v16f acc = {0};
    for (int s = 0; s < 8; ++s)
      acc = mfma_fp4(fp4_operand(query[(size_t)(q0 + r) * 16 + sfmloc::k1_mfma_dword_of_step(h, s)]), B[s], acc);
    for (int reg = 0; reg < 16; ++reg) {
      const int m = (reg & 3) + 8 * (reg >> 2) + 4 * h;
      dist[(size_t)brow * n_q + q0 + m] = (uint16_t)sfmloc::k1_mfma_distance_of_dot((int)acc[reg]);
    }
  }
}

// FORM 0: fp4, 8 MFMA per tile; FORM 2: the same with the +1 constant in a register (as hamming.hip's
// k1_mfma_plus_one_reg); FORM 1: int8, 16 per tile (streamed operand as 0 / 1 bytes, shift + and per dword: the rate of
// that instruction mix, NOT a Hamming distance).
// The wave keeps two bank tiles in registers, reads the query tile's bits from LDS (plane layout: conflict free), expands
// them per use and keeps the running maximum of the dot products.
template <int FORM>
__global__ __launch_bounds__(256) void k_ceiling_screen(int tiles, uint32_t seed, float *__restrict__ sink) {
  __shared__ uint4 qs[4 * 512];  // [plane][row]
  for (int i = threadIdx.x; i < 4 * 512; i += 256) {
    const uint32_t x = (seed + i) * 2654435761u;
    qs[i] = make_uint4(x, x * 31u, x * 977u, x ^ 0x5bd1e995u);
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, r = lane & 31, h = lane >> 5;
  float best = -1024.f;
  int ibest = -1024;
  if (FORM == 0 || FORM == 2) {
    uint32_t plus_one = sfmloc::kE2m1AllPlusOne;
    if (FORM == 2) asm("v_mov_b32 %0, 0x22222222" : "=v"(plus_one));
    v8i B[2][8];
    for (int t = 0; t < 2; ++t)
      for (int s = 0; s < 8; ++s) B[t][s] = fp4_operand(seed * 40503u + threadIdx.x * 31u + t * 7u + s);
    for (int t = 0; t < tiles; ++t) {
      const int row = ((t * 32) & 511) + r;
      const uint4 a0 = qs[(2 * h) * 512 + row], a1 = qs[(2 * h + 1) * 512 + row];
      const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      v16f c0 = {0}, c1 = {0};
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const v8i A = fp4_operand(w[s], plus_one);
        c0 = mfma_fp4(A, B[0][s], c0);
        c1 = mfma_fp4(A, B[1][s], c1);
      }
#pragma unroll
      for (int i = 0; i < 16; i += 2) best = fmaxf(fmaxf(best, c0[i]), c0[i + 1]);
#pragma unroll
      for (int i = 0; i < 16; i += 2) best = fmaxf(fmaxf(best, c1[i]), c1[i + 1]);
    }
  } else {
    v4i B[2][16];
    for (int t = 0; t < 2; ++t)
      for (int s = 0; s < 16; ++s)
        for (int g = 0; g < 4; ++g) B[t][s][g] = (int)pm1_bytes(seed * 40503u + threadIdx.x * 31u + t * 7u + s * 5u + g);
    for (int t = 0; t < tiles; ++t) {
      const int row = ((t * 32) & 511) + r;
      const uint4 a0 = qs[(2 * h) * 512 + row], a1 = qs[(2 * h + 1) * 512 + row];
      const uint32_t w[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      v16i c0 = {0}, c1 = {0};
#pragma unroll
      for (int s = 0; s < 16; ++s) {  // descriptor dword s / 2, bits 8 i + j, j = 4 (s & 1) .. + 3 -> bytes 0 / 1
        v4i A;
#pragma unroll
        for (int g = 0; g < 4; ++g) A[g] = (int)((w[s >> 1] >> (4 * (s & 1) + g)) & 0x01010101u);
        c0 = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B[0][s], c0, 0, 0, 0);
        c1 = __builtin_amdgcn_mfma_i32_32x32x32_i8(A, B[1][s], c1, 0, 0, 0);
      }
#pragma unroll
      for (int i = 0; i < 16; i += 2) ibest = max(max(ibest, c0[i]), c0[i + 1]);
#pragma unroll
      for (int i = 0; i < 16; i += 2) ibest = max(max(ibest, c1[i]), c1[i + 1]);
    }
    best = (float)ibest;
  }
  if (best == 12345.f) sink[0] = best;
}

static uint32_t rnd(uint64_t &s) {
  s = s * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(s >> 33);
}

int main() {
  // ---- functional check ----
  const int n_bank = 4096, n_q = 1000;
  std::vector<uint32_t> bank((size_t)n_bank * 16), query((size_t)n_q * 16);
  uint64_t s = 7;
  auto fill = [&](std::vector<uint32_t> &v, int rows) {
    for (int i = 0; i < rows; ++i)
      for (int k = 0; k < 16; ++k) {
        uint32_t w = (rnd(s) << 16) ^ rnd(s);
        if (k == 15) w &= 0x3Fu;  // 486 valid bits
        v[(size_t)i * 16 + k] = w;
      }
  };
  fill(bank, n_bank);
  fill(query, n_q);
  for (int i = 0; i < n_bank; i += 7) {  // planted near-duplicates and exact ties
    const int j = (i * 31) % n_q;
    memcpy(&bank[(size_t)i * 16], &query[(size_t)j * 16], 64);
    bank[(size_t)i * 16 + (i % 15)] ^= (1u << (i % 29)) | (1u << ((i + 5) % 31));
    if (i % 21 == 0 && j + 1 < n_q) memcpy(&query[(size_t)(j + 1) * 16], &query[(size_t)j * 16], 64);  // a tie: lower index wins
  }
  uint32_t *d_bank, *d_query;
  uint2 *d_out;
  CK(hipMalloc(&d_bank, bank.size() * 4));
  CK(hipMalloc(&d_query, query.size() * 4));
  CK(hipMalloc(&d_out, n_bank * sizeof(uint2)));
  CK(hipMemcpy(d_bank, bank.data(), bank.size() * 4, hipMemcpyHostToDevice));
  CK(hipMemcpy(d_query, query.data(), query.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(k_functional, dim3(n_bank / 32), dim3(64), 0, 0, d_bank, d_query, n_q, d_out);
  CK(hipDeviceSynchronize());
  std::vector<uint2> out(n_bank);
  CK(hipMemcpy(out.data(), d_out, n_bank * sizeof(uint2), hipMemcpyDeviceToHost));
  int bad = 0;
  for (int i = 0; i < n_bank; ++i) {
    uint32_t b0 = 0xFFFFFFFFu, b1 = 0xFFFFFFFFu;
    for (int j = 0; j < n_q; ++j) {
      int d = 0;
      for (int k = 0; k < 16; ++k) d += __builtin_popcount(bank[(size_t)i * 16 + k] ^ query[(size_t)j * 16 + k]);
      const uint32_t key = ((uint32_t)d << 16) | (uint32_t)j;
      const uint32_t lo = key < b0 ? key : b0, hi = key < b0 ? b0 : key;
      b1 = hi < b1 ? hi : b1;
      b0 = lo;
    }
    if (out[i].x != b0 || out[i].y != b1) {
      if (bad < 5) printf("row %d: mfma (%08x, %08x) popcount (%08x, %08x)\n", i, out[i].x, out[i].y, b0, b1);
      ++bad;
    }
  }
  printf("{\"functional\": \"%d bank rows x %d query rows, top-2 keys by i8 MFMA vs popcount\", \"rows_differing\": %d}\n",
         n_bank, n_q, bad);
  // ---- ceiling ----
  hipDeviceProp_t prop;
  CK(hipGetDeviceProperties(&prop, 0));
  const int cus = prop.multiProcessorCount;
  uint2 *d_sink;
  CK(hipMalloc(&d_sink, 16));
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  for (int epi = 0; epi < 2; ++epi)
    for (int wps = 1; wps <= 4; wps *= 2) {
      const int tiles = 4000;
      const int blocks = cus * wps;  // 256 threads = 4 waves = one per SIMD; wps blocks per CU
      for (int rep = 0; rep < 2; ++rep) {
        CK(hipEventRecord(e0));
        if (epi)
          hipLaunchKernelGGL(k_ceiling<1>, dim3(blocks), dim3(256), 0, 0, tiles, 11u, d_sink);
        else
          hipLaunchKernelGGL(k_ceiling<0>, dim3(blocks), dim3(256), 0, 0, tiles, 11u, d_sink);
        CK(hipEventRecord(e1));
        CK(hipEventSynchronize(e1));
      }
      float ms = 0;
      CK(hipEventElapsedTime(&ms, e0, e1));
      const double pairs = (double)blocks * 4 * tiles * 1024.0;
      printf("{\"ceiling\": \"%s\", \"waves_per_simd\": %d, \"ms\": %.3f, \"tera_pairs_per_s\": %.3f, "
             "\"i8_tera_ops_per_s\": %.1f}\n",
             epi ? "16 MFMA + top-2 epilogue (3 VALU per pair) per 32x32 tile" : "16 MFMA per tile, no epilogue", wps, ms,
             pairs / (ms * 1e-3) / 1e12, pairs * 1024.0 / (ms * 1e-3) / 1e12);
    }
  // ---- fp4 functional: all 512 bits, every pair ----
  int bad4 = 0;
  {
    const int nq4 = 1024;  // 1 000 query rows + all-zero padding rows up to a multiple of 32
    std::vector<uint32_t> bank4((size_t)n_bank * 16), query4((size_t)nq4 * 16, 0u);
    uint64_t s4 = 11;
    for (auto &w : bank4) w = (rnd(s4) << 16) ^ rnd(s4);
    for (size_t i = 0; i < (size_t)n_q * 16; ++i) query4[i] = (rnd(s4) << 16) ^ rnd(s4);
    for (int i = 0; i < n_bank; i += 7) {  // near-duplicates, exact copies (distance 0), ties between query rows
      const int j = (i * 31) % n_q;
      memcpy(&bank4[(size_t)i * 16], &query4[(size_t)j * 16], 64);
      if (i % 3) bank4[(size_t)i * 16 + (i % 16)] ^= (1u << (i % 29)) | (1u << ((i + 5) % 31));
      if (i % 21 == 0 && j + 1 < n_q) memcpy(&query4[(size_t)(j + 1) * 16], &query4[(size_t)j * 16], 64);
    }
    for (int k = 0; k < 16; ++k) {  // the accumulator extremes: all ones against all zeros (512) and against itself (0)
      bank4[(size_t)5 * 16 + k] = 0xFFFFFFFFu, bank4[(size_t)6 * 16 + k] = 0u;
      query4[(size_t)3 * 16 + k] = 0u, query4[(size_t)4 * 16 + k] = 0xFFFFFFFFu;
    }
    uint32_t *d_b4, *d_q4;
    uint16_t *d_dist;
    CK(hipMalloc(&d_b4, bank4.size() * 4));
    CK(hipMalloc(&d_q4, query4.size() * 4));
    CK(hipMalloc(&d_dist, (size_t)n_bank * nq4 * 2));
    CK(hipMemcpy(d_b4, bank4.data(), bank4.size() * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(d_q4, query4.data(), query4.size() * 4, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_functional_fp4, dim3(n_bank / 32), dim3(64), 0, 0, d_b4, d_q4, nq4, d_dist);
    CK(hipDeviceSynchronize());
    std::vector<uint16_t> dist((size_t)n_bank * nq4);
    CK(hipMemcpy(dist.data(), d_dist, dist.size() * 2, hipMemcpyDeviceToHost));
    int dmin = 512, dmax = 0;
    for (int i = 0; i < n_bank; ++i)
      for (int j = 0; j < nq4; ++j) {
        int d = 0;
        for (int k = 0; k < 16; ++k) d += __builtin_popcount(bank4[(size_t)i * 16 + k] ^ query4[(size_t)j * 16 + k]);
        dmin = d < dmin ? d : dmin, dmax = d > dmax ? d : dmax;
        if (dist[(size_t)i * nq4 + j] != d) {
          if (bad4 < 5) printf("pair (%d, %d): fp4 mfma %d popcount %d\n", i, j, (int)dist[(size_t)i * nq4 + j], d);
          ++bad4;
        }
      }
    printf("{\"functional\": \"%d bank rows x %d query rows (%d of them all-zero padding), every distance over 512 bits by "
           "e2m1 MFMA vs popcount\", \"distance_range\": [%d, %d], \"pairs_differing\": %d}\n",
           n_bank, nq4, nq4 - n_q, dmin, dmax, bad4);
  }
  // ---- screening ceilings ----
  {
    float *d_fsink;
    CK(hipMalloc(&d_fsink, 16));
    for (int form = 0; form < 3; ++form)
      for (int wps = 1; wps <= 4; wps *= 2) {
        const int tiles = 4000, blocks = cus * wps;
        for (int rep = 0; rep < 3; ++rep) {
          CK(hipEventRecord(e0));
          if (form == 0)
            hipLaunchKernelGGL(k_ceiling_screen<0>, dim3(blocks), dim3(256), 0, 0, tiles, 11u, d_fsink);
          else if (form == 2)
            hipLaunchKernelGGL(k_ceiling_screen<2>, dim3(blocks), dim3(256), 0, 0, tiles, 11u, d_fsink);
          else
            hipLaunchKernelGGL(k_ceiling_screen<1>, dim3(blocks), dim3(256), 0, 0, tiles, 11u, d_fsink);
          CK(hipEventRecord(e1));
          CK(hipEventSynchronize(e1));
        }
        float ms = 0;
        CK(hipEventElapsedTime(&ms, e0, e1));
        const double pairs = (double)blocks * 4 * tiles * 2048.0;  // two 32 x 32 tiles per wave and step
        printf("{\"ceiling\": \"screening, %s, operand from LDS expanded per use, 8 x v_max3 per tile\", "
               "\"waves_per_simd\": %d, \"ms\": %.3f, \"tera_pairs_per_s\": %.3f}\n",
               form == 0   ? "fp4 e2m1 32x32x64 (8 MFMA per tile), +1 constant a literal (10 VALU per dword)"
               : form == 2 ? "fp4 e2m1 32x32x64 (8 MFMA per tile), +1 constant in a register (7 VALU per dword)"
                           : "int8 32x32x32 (16 MFMA per tile; rate probe, 0 / 1 bytes)",
               wps, ms,
               pairs / (ms * 1e-3) / 1e12);
      }
  }
  return (bad || bad4) ? 1 : 0;
}
