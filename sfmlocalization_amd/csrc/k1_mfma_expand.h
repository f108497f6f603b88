// Operand expansion of the matrix-core Hamming scan (k_hamming_screen_mfma, hamming.hip).
//
// Hamming(a, b) over the 512 stored bits = (512 - <a', b'>) / 2 with a', b' the bits as +-1: a clear bit is +1, a set
// bit -1.  +-1 is exact in OCP e2m1 (FP4): nibble 0x2 = +1.0, 0xA = -1.0, so one descriptor dword (32 bits) becomes
// the four operand dwords (32 nibbles) a lane feeds to one v_mfma_scale_f32_32x32x64_f8f6f4 (cbsz:4 blgp:4, both block
// scales 2^0 = E8M0 byte 127).  The products are +-1 and a sum of 512 of them is an integer of magnitude <= 512:
// exact in the f32 accumulator.
//
// A dot product does not care in which order K is walked as long as BOTH operands walk it in the same order, so the
// bits are not spread in place: nibble i of output dword j carries bit 4 i + j of the input dword.  That is one
// shift and one and-or per output dword (the shift by 0 falls away): 7 VALU instructions per descriptor dword.
//
// Plain functions, usable from host code (tests/cpp/k1_mfma_identity.cpp is built with g++) and from kernels.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define K1_MFMA_FN __host__ __device__ __forceinline__
#else
#define K1_MFMA_FN static inline
#endif

namespace sfmloc {

constexpr uint32_t kE2m1PlusOne = 0x2u, kE2m1MinusOne = 0xAu;  // OCP e2m1: sign | 2 exponent bits | 1 mantissa bit
constexpr uint32_t kE8m0One = 127u;                            // block scale 2^0

constexpr uint32_t kE2m1AllPlusOne = 0x22222222u;              // eight nibbles of +1

// output dword j (0..3) of descriptor dword w: nibble i = bit (4 i + j) of w as e2m1 +-1.  all_plus_one is
// kE2m1AllPlusOne; a kernel passes it in a register so that the and-or is ONE instruction (v_and_or_b32 takes one
// literal, and the mask is the other).
K1_MFMA_FN uint32_t k1_mfma_expand_dword(uint32_t w, int j, uint32_t all_plus_one = kE2m1AllPlusOne) {
  return ((w << (3 - j)) & 0x88888888u) | all_plus_one;
}

// the four operand dwords of one lane for one K step of 64 (the lane's 32 K values) from one descriptor dword
K1_MFMA_FN void k1_mfma_expand(uint32_t w, uint32_t out[4], uint32_t all_plus_one = kE2m1AllPlusOne) {
  out[0] = k1_mfma_expand_dword(w, 0, all_plus_one);
  out[1] = k1_mfma_expand_dword(w, 1, all_plus_one);
  out[2] = k1_mfma_expand_dword(w, 2, all_plus_one);
  out[3] = k1_mfma_expand_dword(w, 3, all_plus_one);
}

// Which descriptor dword lane half h (lane / 32) feeds to K step s (0..7) -- the SAME rule for the bank operand and
// for the query operand: half h walks dwords 8 h .. 8 h + 7, i.e. planes 2 h and 2 h + 1 of a tiled64 row, so a lane
// fetches its share of a row as two 16-byte loads.
K1_MFMA_FN int k1_mfma_dword_of_step(int h, int s) { return 8 * h + s; }

// dot product -> Hamming distance over the 512 stored bits
K1_MFMA_FN int k1_mfma_distance_of_dot(int dot) { return (512 - dot) / 2; }

}  // namespace sfmloc
