// The host side of sfmloc_akaze_create (akaze.hip): everything OpenCV's AKAZE computes once per image size -- the
// evolution levels (Allocate_Memory_Evolution), each level's Fast Explicit Diffusion cycle (fed_tau_by_process_time) and
// the constant tables of orientation and M-LDB -- and, below them, the launch schedule: which kernel form every part of an
// extraction takes, with every threshold.  Host code only, no HIP: tests/cpp/akaze_plan.cpp runs it under the host
// sanitizers, tests/test_akaze_plan.py compares the plan with the CPU restatement's, bit for bit, and
// tests/test_akaze_cases_cpu.py the schedule with what every boundary case promises.
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

// Allocate_Memory_Evolution + FED schedule + constant tables.  -> true; or false when an evolved level's FED cycle is
// longer than kMaxFedSteps or has no step at all (the launch schedule below has no form for either), with that level in
// *bad_level and its step count in *bad_steps (the plan is then not to be used).
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
    if (P.lev[i].nsteps > kMaxFedSteps || P.lev[i].nsteps < 1) {
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

// ---- the launch schedule ------------------------------------------------------------------------------------------
// Which kernel form every part of an extraction takes, as pure functions of the plan and of the number of levels a call
// builds.  akaze.hip launches what these say and sizes its buffers from them; every threshold is a named constant here
// and nowhere else.  tests/cpp/akaze_plan.cpp prints the schedule, and tests/test_akaze_cases_cpu.py holds it against the
// restatement of these conditions in tests/akaze_cases.py, so that a boundary case stays on its boundary.

// -- what sfmloc_akaze_create accepts
constexpr int kMinSide = 16;           // width and height from this ...
constexpr int kMaxWidth = 16384;       // ... to this width (the x a candidate's packed word holds)
constexpr int kSupMaxRows = 4096 + 1;  // level rows the row-start tables of k_suppress hold: height <= kSupMaxRows - 1
constexpr int kMaxOctaves = 8;
enum Request { kRequestOk = 0, kRequestSize, kRequestOctaves };
inline Request check_request(int w, int h, int omax, int nsub) {
  if (w < kMinSide || h < kMinSide || w > kMaxWidth || h > kSupMaxRows - 1) return kRequestSize;
  if (omax < 1 || omax > kMaxOctaves || nsub < 1 || omax * nsub > kMaxLevels) return kRequestOctaves;
  return kRequestOk;
}

// the levels [0, levels_built) are built by a call that needs `need` of them (0: all; a description-only call asks for
// the levels up to its keypoints' highest)
inline int levels_built(const AkPlan &P, int need) { return (need > 0 && need < P.nlev) ? need : P.nlev; }

// -- the start: the contrast factor's kernels walk kGradRows image rows per workgroup; the histogram's grid is clamped to
// about kHistGridMax workgroups (each ends in atomics on the same 301 words) by giving a workgroup several such chunks
constexpr int kGradRows = 16;
constexpr unsigned int kHistGridMax = 256;

// -- evolution: the loop over the levels 1 .. levels_built - 1 goes in steps, each a resident run or a single level
constexpr unsigned int kResidentLdsBytes = 150u * 1024u;  // k_octave_resident: three float images of the octave in LDS
constexpr int kOctaveRunMax = 8;                          // levels of one octave k_octave_resident evolves in a launch
// diffusion steps per launch of k_smooth_nld / k_nld_steps: 4 on the large levels, where the tile halo's redundant work
// costs more than a launch; 8 on the upper octaves (<= 160 wide), whose steps are each far shorter than a launch boundary
// and which hold most of the schedule's steps (133 of 165 at VGA).  (The 240 x 135 octave of a 1080p frame was tried with
// the small levels' count: no effect, 1.10 / 1.23 ms either way.)
constexpr int kNldStepsLarge = 4, kNldStepsSmall = 8;
constexpr int kNldSmallWidth = 160;
constexpr int kNldFuseMax = 8;  // the largest K the step kernels are instantiated for
static_assert(kNldStepsLarge <= kNldFuseMax && kNldStepsSmall <= kNldFuseMax, "a launch with no kernel instantiated for it");

enum Source { kPrevLt, kOwnLt, kScratch };  // the previous level's Lt; this level's Lt; the scratch image
struct EvoStep {
  bool resident;     // levels first .. last of one octave in one k_octave_resident launch; else: the level `first` alone
  bool halfsample;   // `first` opens its octave: the previous level's Lt is half-sampled into `source` first
  int first, last;
  Source source;     // what the step's first launch reads
  // a single level: its FED cycle in n_launch launches of up to `fuse` steps, the first k_smooth_nld, the others
  // k_nld_steps, ping-ponging between the level's Lt and the scratch image
  int fuse, n_launch;
};
// launch j of n_launch writes the level's Lt (else the scratch image): alternating, so that the last one writes Lt.  The
// half-sampled start lands where launch 0 does not write (evolution() below); any other start is another level's Lt.
inline bool launch_writes_lt(int n_launch, int j) { return (n_launch - 1 - j) % 2 == 0; }
inline int launch_steps(const EvoStep &E, int nsteps, int j) {
  const int left = nsteps - j * E.fuse;
  return left < E.fuse ? left : E.fuse;
}

// -> the number of steps, steps[0 .. n) filled (at most kMaxLevels - 1)
inline int evolution(const AkPlan &P, int need, EvoStep *steps) {
  const int nlev = levels_built(P, need);
  int n = 0;
  for (int i = 1; i < nlev; ++i) {
    const AkLevel &L = P.lev[i], &Lp = P.lev[i - 1];
    EvoStep &E = steps[n++];
    E = EvoStep{};
    E.first = E.last = i;
    E.halfsample = L.octave > Lp.octave;
    // an octave whose image fits in LDS three times runs in one launch, from its first level of the loop to the last
    // level of it that is built, if that run is short enough
    int j = i;
    while (j + 1 < nlev && P.lev[j + 1].octave == L.octave) ++j;
    const bool opens = i == 1 || Lp.octave != L.octave;
    if (opens && (size_t)3 * L.w * L.h * sizeof(float) <= kResidentLdsBytes && j - i + 1 <= kOctaveRunMax) {
      E.resident = true;
      E.last = j;
      E.source = E.halfsample ? kScratch : kPrevLt;
      i = j;
      continue;
    }
    E.fuse = L.w <= kNldSmallWidth ? kNldStepsSmall : kNldStepsLarge;
    E.n_launch = (L.nsteps + E.fuse - 1) / E.fuse;
    E.source = !E.halfsample ? kPrevLt : (launch_writes_lt(E.n_launch, 0) ? kScratch : kOwnLt);
  }
  return n;
}

// -- detection and its buffers: functions of the frame's size and the plan alone
constexpr int kSegPx = 64;                         // a segment = what one wave of the extrema kernels covers
constexpr unsigned int kSegChunk = 4096;           // segments one workgroup of k_seg_sum / k_seg_write scans
constexpr unsigned int kSegScanOneLaunch = 65536;  // n_seg up to this: k_seg_scan, one workgroup; above, the two kernels
constexpr unsigned int kSegChunksMax = 1024;       // ... if their chunks fit the partial sums' array
constexpr unsigned int kCandCap = 1u << 16;        // extrema candidates the workspace holds
constexpr unsigned int kSpecStart = 512, kSpecMax = 4096;  // the speculative download: records at first, at most
// the fixed grids that stride over candidates / keypoints whose number is on the device: a workgroup per so many pixels
constexpr unsigned int kNbrPixPerGroup = 384, kNbrGridMin = 256, kNbrGridMax = 4096;
constexpr unsigned int kDescPixPerGroup = 96, kDescGridMin = 1024, kDescGridMax = 16384;

struct Detection {
  unsigned int rows;                   // rows of all levels, one under the other
  unsigned int segs_per_row, n_seg;    // segments per row of the FRAME's width, for every row of every level
  unsigned int seg_chunks;
  bool scan_two_launches;              // k_seg_sum + k_seg_write instead of k_seg_scan
  unsigned int hist_grid_x, grad_grid_y, hist_grid_y;  // k_pre_grad (x, grad y), k_pre_hist (x, hist y: clamped)
  unsigned int nbr_grid, desc_grid;    // k_suppress_nbr, k_orient_describe
  unsigned int cand_cap, spec_start, spec_max;
};
inline unsigned int clamp_u(size_t v, unsigned int lo, unsigned int hi) {
  return v < lo ? lo : (v > hi ? hi : (unsigned int)v);
}
inline Detection detection(const AkPlan &P, int w, int h) {
  Detection D{};
  for (int i = 0; i < P.nlev; ++i) D.rows += (unsigned int)P.lev[i].h;
  D.segs_per_row = (unsigned int)(128 / kSegPx) * (unsigned int)((w + 127) / 128);
  D.n_seg = D.rows * D.segs_per_row;
  D.seg_chunks = (D.n_seg + kSegChunk - 1u) / kSegChunk;
  D.scan_two_launches = D.n_seg > kSegScanOneLaunch && D.seg_chunks <= kSegChunksMax;
  D.hist_grid_x = (unsigned int)((w + 127) / 128);
  D.grad_grid_y = D.hist_grid_y = (unsigned int)((h + kGradRows - 1) / kGradRows);
  if (D.hist_grid_x * D.hist_grid_y > kHistGridMax) D.hist_grid_y = clamp_u(kHistGridMax / D.hist_grid_x, 1u, kHistGridMax);
  D.nbr_grid = clamp_u((size_t)w * h / kNbrPixPerGroup, kNbrGridMin, kNbrGridMax);
  D.desc_grid = clamp_u((size_t)w * h / kDescPixPerGroup, kDescGridMin, kDescGridMax);
  D.cand_cap = kCandCap;
  D.spec_start = kSpecStart;
  D.spec_max = kSpecMax;
  return D;
}

}  // namespace akaze_plan
}  // namespace sfmloc
