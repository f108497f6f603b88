// Host check of the operand expansion of the matrix-core Hamming scan (sfmlocalization_amd/csrc/k1_mfma_expand.h), with
// the very functions the kernel uses: for 64-byte rows a, b
//   (512 - sum_k a'_k b'_k) / 2 = popcount(a ^ b)
// where a', b' are the e2m1 nibbles of the expanded operands decoded here on the host, walked in the order the
// instruction walks them: K step s = 0..7, lane half h = 0..1 (each holding 32 K values: 4 dwords x 8 nibbles).  Also:
// every nibble is +1 or -1, both operands take bit k from the same place (the expansion is a bijection of the 512 bits,
// the same for either operand), and the in-register form (all_plus_one passed in) equals the default.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../sfmlocalization_amd/csrc/k1_mfma_expand.h"

using namespace sfmloc;

static int e2m1_value_x2(uint32_t nib) {  // OCP e2m1 -> twice the value (so that 0.5 stays an integer)
  static const int mag2[8] = {0, 1, 2, 3, 4, 6, 8, 12};
  const int v = mag2[nib & 7u];
  return (nib & 8u) ? -v : v;
}

// the K values of one row in instruction order, as +-1
static bool operand(const uint32_t row[16], int out[512]) {
  int k = 0;
  for (int s = 0; s < 8; ++s)
    for (int h = 0; h < 2; ++h) {
      uint32_t e[4], e2[4];
      k1_mfma_expand(row[k1_mfma_dword_of_step(h, s)], e);
      k1_mfma_expand(row[k1_mfma_dword_of_step(h, s)], e2, kE2m1AllPlusOne);
      if (memcmp(e, e2, sizeof e)) return false;
      for (int j = 0; j < 4; ++j)
        for (int i = 0; i < 8; ++i) {
          const uint32_t nib = (e[j] >> (4 * i)) & 0xFu;
          if (nib != kE2m1PlusOne && nib != kE2m1MinusOne) return false;
          out[k++] = e2m1_value_x2(nib) / 2;
        }
    }
  return k == 512;
}

static uint64_t rng_state = 12345;
static uint32_t rnd() {
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (uint32_t)(rng_state >> 32);
}

static int check_pair(const uint32_t a[16], const uint32_t b[16]) {
  int av[512], bv[512];
  if (!operand(a, av) || !operand(b, bv)) return 1;
  int dot = 0, pop = 0;
  for (int k = 0; k < 512; ++k) dot += av[k] * bv[k];
  for (int k = 0; k < 16; ++k) pop += __builtin_popcount(a[k] ^ b[k]);
  if (k1_mfma_distance_of_dot(dot) != pop || (512 - dot) % 2 != 0) {
    printf("dot %d -> %d, popcount %d\n", dot, k1_mfma_distance_of_dot(dot), pop);
    return 1;
  }
  return 0;
}

int main() {
  int bad = 0;
  uint32_t a[16], b[16];
  // same order for both operands, and a bijection: a single set bit lands in exactly one K position, the same position
  // whichever operand carries it, and 512 different bits land in 512 different positions
  bool seen[512] = {false};
  for (int bit = 0; bit < 512; ++bit) {
    memset(a, 0, sizeof a);
    a[bit >> 5] = 1u << (bit & 31);
    int v[512], pos = -1, n = 0;
    if (!operand(a, v)) ++bad;
    for (int k = 0; k < 512; ++k)
      if (v[k] == -1) pos = k, ++n;
    if (n != 1 || seen[pos]) ++bad;
    else seen[pos] = true;
  }
  // extremes
  memset(a, 0, sizeof a);
  memset(b, 0xFF, sizeof b);
  bad += check_pair(a, b);  // 512
  bad += check_pair(a, a);  // 0
  bad += check_pair(b, b);  // 0
  for (int bit = 0; bit < 512; ++bit) {  // distance 1 and 511 at every bit position
    memset(a, 0, sizeof a);
    a[bit >> 5] = 1u << (bit & 31);
    memset(b, 0, sizeof b);
    bad += check_pair(a, b);
    memset(b, 0xFF, sizeof b);
    bad += check_pair(a, b);
  }
  for (int t = 0; t < 20000; ++t) {  // random rows, dense and sparse, near-duplicates
    for (int k = 0; k < 16; ++k) a[k] = rnd(), b[k] = rnd();
    if (t % 3 == 1)
      for (int k = 0; k < 16; ++k) a[k] &= rnd() & rnd(), b[k] &= rnd() & rnd();
    if (t % 3 == 2) {
      memcpy(b, a, sizeof b);
      for (int f = 0; f < (int)(rnd() % 40); ++f) b[rnd() % 16] ^= 1u << (rnd() % 32);
    }
    bad += check_pair(a, b);
  }
  printf("%s: %d failures\n", bad ? "FAILED" : "OK", bad);
  return bad ? 1 : 0;
}
