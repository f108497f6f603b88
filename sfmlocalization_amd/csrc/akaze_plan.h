// The host side of sfmloc_akaze_create (akaze.hip): everything OpenCV's AKAZE computes once per image size -- the
// evolution levels (Allocate_Memory_Evolution), each level's Fast Explicit Diffusion cycle (fed_tau_by_process_time) and
// the constant tables of orientation and M-LDB.  Host code only, no HIP: tests/cpp/akaze_plan.cpp runs it under the host
// sanitizers and tests/test_akaze_plan.py compares it with the CPU restatement's plan, bit for bit.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

namespace sfmloc {
namespace akaze_plan {

constexpr int kMaxLevels = 32;
// The longest FED cycle of one level.  AkLevel::tsteps, the device-side table of half steps ([level][kMaxFedSteps]) and
// OctaveRun::step0 of k_octave_resident are all laid out for it; a request whose schedule needs a longer cycle (a large
// frame with many octaves: 2560 x 1280 with six) is refused by sfmloc_akaze_create.
constexpr int kMaxFedSteps = 64;
constexpr float kPiF = 3.14159265358979323846f;

struct AkLevel {
  int w, h, octave, sublevel, sigma_size, nsteps;
  float esigma, etime;
  float tsteps[kMaxFedSteps];
  size_t off;  // offset (floats) of this level inside each per-level image stack
};

struct AkPlan {
  int nlev = 0;
  AkLevel lev[kMaxLevels];
  float g16[9], g10[5];
  float gauss25[49];
  float win_ang1[64];
  int n_win = 0;
  uint16_t pair_tab[486 * 2];
  size_t total = 0;
};

inline int fround_h(float f) { return (int)(f + 0.5f); }

inline bool is_prime(int n) {
  if (n <= 3) return n > 1;
  if (n % 2 == 0 || n % 3 == 0) return false;
  for (int i = 5; i * i <= n; i += 6)
    if (n % i == 0 || n % (i + 2) == 0) return false;
  return true;
}

// fed_tau_by_process_time(T, 1, 0.25, reordering = true) of OpenCV's fed.cpp -> the cycle's length n, with tau[0 .. n)
// filled; a cycle longer than kMaxFedSteps is reported by its length alone: nothing is written.
inline int fed_tau(float T, float tau_max, float *tau /*[kMaxFedSteps]*/) {
  const int n = (int)(ceilf(sqrtf(3.0f * T / tau_max + 0.25f) - 0.5f - 1.0e-8f) + 0.5f);
  if (n <= 0) return 0;
  if (n > kMaxFedSteps) return n;
  const float scale = 3.0f * T / (tau_max * (float)(n * (n + 1)));
  float tauh[kMaxFedSteps];
  const float c = 1.0f / (4.0f * (float)n + 2.0f);
  const float d = scale * tau_max / 2.0f;
  for (int k = 0; k < n; ++k) {
    const float hh = cosf(kPiF * (2.0f * (float)k + 1.0f) * c);
    tauh[k] = d / (hh * hh);
  }
  // A cycle of one step has nothing to reorder, and kappa = 0 would make the index below -1 for every k (a read before
  // tauh; OpenCV's own code does that).  Sub-level counts of about 11 and more have such levels.
  if (n == 1) {
    tau[0] = tauh[0];
    return 1;
  }
  const int kappa = n / 2;
  int prime = n + 1;
  while (!is_prime(prime)) prime++;
  for (int k = 0, l = 0; l < n; ++k, ++l) {
    int index;
    while ((index = ((k + 1) * kappa) % prime - 1) >= n) k++;
    tau[l] = tauh[index];
  }
  return n;
}

inline void gaussian_kernel(int ksize, float sigma, float *cf) {  // cv::getGaussianKernel(ksize, sigma, CV_32F)
  const double scale2x = -0.5 / ((double)sigma * sigma);
  double sum = 0;
  for (int i = 0; i < ksize; ++i) {
    const double x = i - (ksize - 1) * 0.5;
    cf[i] = (float)exp(scale2x * x * x);
    sum += cf[i];
  }
  sum = 1.0 / sum;
  for (int i = 0; i < ksize; ++i) cf[i] = (float)(cf[i] * sum);
}

// Allocate_Memory_Evolution + FED schedule + constant tables.  -> true; or false when a level's FED cycle is longer than
// kMaxFedSteps, with that level in *bad_level and its step count in *bad_steps (the plan is then not to be used).
inline bool make_plan(int w, int h, int omax, int nsub, AkPlan &P, int *bad_level, int *bad_steps) {
  const float soffset = 1.6f, derivative_factor = 1.5f;
  P.nlev = 0;
  P.total = 0;
  for (int i = 0; i < omax; ++i) {
    const float rfactor = 1.0f / powf(2.0f, (float)i);
    const int lh = (int)(h * rfactor), lw = (int)(w * rfactor);
    if ((lw < 80 || lh < 40) && i != 0) break;
    for (int j = 0; j < nsub && P.nlev < kMaxLevels; ++j) {
      AkLevel &L = P.lev[P.nlev++];
      memset(&L, 0, sizeof(L));
      L.w = lw;
      L.h = lh;
      L.esigma = soffset * powf(2.0f, (float)j / (float)nsub + (float)i);
      L.sigma_size = fround_h(L.esigma * derivative_factor / powf(2.0f, (float)i));
      L.etime = 0.5f * (L.esigma * L.esigma);
      L.octave = i;
      L.sublevel = j;
      L.off = P.total;
      P.total += (size_t)lw * lh;
    }
  }
  for (int i = 1; i < P.nlev; ++i) {
    P.lev[i].nsteps = fed_tau(P.lev[i].etime - P.lev[i - 1].etime, 0.25f, P.lev[i].tsteps);
    if (P.lev[i].nsteps > kMaxFedSteps) {
      *bad_level = i;
      *bad_steps = P.lev[i].nsteps;
      return false;
    }
  }
  gaussian_kernel(9, 1.6f, P.g16);
  gaussian_kernel(5, 1.0f, P.g10);
  for (int i = 0; i < 7; ++i)
    for (int j = 0; j < 7; ++j)
      P.gauss25[7 * i + j] = (float)(exp(-(double)(i * i + j * j) / 12.5) / (2.0 * 3.14159265358979323846 * 6.25));
  P.n_win = 0;
  for (float a = 0.0f; a < 2.0f * kPiF; a += 0.15f) P.win_ang1[P.n_win++] = a;
  // M-LDB comparison pairs: bit dpos compares values[a] > values[b]; values are laid out [cell][channel] with the
  // cells of the three grids back to back (4 + 9 + 16)
  int dpos = 0, cell0 = 0;
  const int counts[3] = {4, 9, 16};
  for (int lvl = 0; lvl < 3; ++lvl) {
    for (int pos = 0; pos < 3; ++pos)
      for (int a = 0; a < counts[lvl]; ++a)
        for (int b = a + 1; b < counts[lvl]; ++b) {
          P.pair_tab[2 * dpos] = (uint16_t)((cell0 + a) * 3 + pos);
          P.pair_tab[2 * dpos + 1] = (uint16_t)((cell0 + b) * 3 + pos);
          ++dpos;
        }
    cell0 += counts[lvl];
  }
  return true;
}

}  // namespace akaze_plan
}  // namespace sfmloc
