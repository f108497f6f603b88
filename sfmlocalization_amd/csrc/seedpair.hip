// sfmloc_seed_scores: per matched pair the median cosine between the two rays of its inlier matches -- what the choice
// of the initial pair of incremental SfM looks at (OpenMVG's AutomaticInitialPairChoice).  The semantics are stated in
// include/sfmloc.h ("Seed scores"); tests/seed_np.py restates every operation.  f64, unfused (the library's
// -ffp-contract=off), only + - * / sqrt; after the cosine nothing but comparisons and integer counts, no float atomics:
// the records are the restatement's bits.  Scene and poses: PairScene and PairPoses on the host (pair_scene.h), PairDev
// and PairPosesDev on the device (twoview_device.h), the bases of SdDev.
//
//   k_seed_scores  one workgroup of 256 threads per pair, one form for any inlier count.
//                    keys     lane l computes the inliers l, l + 256, ...: bearings, the two-view point, the clamped
//                             cosine, its ordered key -- or 0 for an inlier that is not used -- to the pair's slab in
//                             global memory (8 bytes per inlier, lane-consecutive).  n_used through one LDS counter.
//                    select   eight passes over the slab, a byte of the key each from the top: a 256-bin histogram of
//                             the keys that still carry the prefix (integer LDS atomics; a wave whose lanes all name one
//                             bin adds once), an inclusive scan of the bins from 255 down (__shfl_up inside a wave, the
//                             four waves' totals through LDS), and the one bin that holds the wanted rank extends the
//                             prefix.  After the last pass the prefix is the element's key.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "seed_host.h"
#include "twoview_device.h"

namespace sfmloc {
namespace {

constexpr int kSdThreads = 256;

thread_local double g_seed_last_ms = 0.0;

struct Seed {
  std::vector<sfmloc_seed_score> rec;
};

struct SdDev : PairDev, PairPosesDev {
  uint64_t *key;  // [n_inliers]: a pair's slab at inl_off[k]; 0 = the inlier is not used
  sfmloc_seed_score *rec;
  uint32_t min_used;
  double max_cos, min_cos;
};

// sfmloc.h "key": ascending as the doubles are, -0.0 below +0.0; never 0 for a clamped cosine
__device__ __forceinline__ uint64_t sd_key(double c) {
  const uint64_t u = geom::d2u(c);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double sd_unkey(uint64_t k) {
  return geom::u2d((k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k);
}

// sfmloc.h "cosine" of the match with bearings (a, b) in I and (u, v) in J
__device__ __forceinline__ double sd_cosine(const double *R, double a, double b, double u, double v) {
  const double x = (R[0] * u + R[3] * v) + R[6];
  const double y = (R[1] * u + R[4] * v) + R[7];
  const double z = (R[2] * u + R[5] * v) + R[8];
  const double dot = (a * x + b * y) + z;
  const double n1 = sqrt((a * a + b * b) + 1.0), n2 = sqrt((x * x + y * y) + z * z);
  const double c = dot / (n1 * n2);
  const double lo = -1.0 + 1.e-8, hi = 1.0 - 1.e-8;
  const double m = (hi < c) ? hi : c;  // std::max(lo, std::min(c, hi)): a NaN cosine becomes lo (adjust.hip)
  return (lo < m) ? m : lo;
}

__global__ __launch_bounds__(kSdThreads) void k_seed_scores(SdDev D) {
  __shared__ uint32_t hist[256];
  __shared__ uint32_t s_wtot[kSdThreads / 64];
  __shared__ uint32_t s_used, s_bin, s_want;
  const uint32_t k = blockIdx.x;
  if (k >= D.n_pairs || !D.use[k]) return;  // (the same for the whole workgroup; the records were zeroed)
  const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; ++i) R[i] = D.relR[9 * (size_t)k + i];
#pragma unroll
  for (int i = 0; i < 3; ++i) t[i] = D.relt[3 * (size_t)k + i];
  const uint64_t i0 = D.inl_off[k];
  const size_t n = (size_t)(D.inl_off[k + 1] - i0);
  uint64_t *slab = D.key + i0;
  const ViewCam ci = view_cam(D, D.pairs[2 * (size_t)k]), cj = view_cam(D, D.pairs[2 * (size_t)k + 1]);
  const uint64_t m0 = D.offsets[k];
  if (tid == 0) s_used = 0;
  __syncthreads();
  // sfmloc.h "bearings", "point", "cosine", "key"
  uint32_t mine = 0;
  for (size_t p = tid; p < n; p += kSdThreads) {
    const uint64_t mt = m0 + D.inl_idx[i0 + p];
    double a, b, u, v, zi, zj;
    feature_bearing(D, ci, D.match_i[mt], &a, &b);
    feature_bearing(D, cj, D.match_j[mt], &u, &v);
    const bool ok = two_view_depths(R, t, a, b, u, v, &zi, &zj) && geom::is_finite(zj) && zi > 0.0 && zj > 0.0;
    slab[p] = ok ? sd_key(sd_cosine(R, a, b, u, v)) : 0ull;
    mine += ok ? 1u : 0u;
  }
  if (mine) atomicAdd(&s_used, mine);  // (an integer count: the same whatever the order)
  __syncthreads();  // (also: every thread reads below only the keys it wrote itself, p = tid + 256 i)
  const uint32_t n_used = s_used;
  double cm = 0.0;
  if (n_used) {
    // sfmloc.h "median": the element with `want` keys above it
    uint32_t want = n_used / 2;
    uint64_t prefix = 0;
    for (int q = 0; q < 8; ++q) {
      const int shift = 56 - 8 * q;
      hist[tid] = 0;
      __syncthreads();
      for (size_t base = 0; base < n; base += kSdThreads) {  // (whole tiles: the ballots need every lane of a wave)
        const size_t p = base + tid;
        const uint64_t key = p < n ? slab[p] : 0ull;
        const bool in = key != 0 && (q == 0 || (key >> (shift + 8)) == prefix);
        const uint32_t bin = (uint32_t)(key >> shift) & 255u;
        const unsigned long long m = __ballot(in);
        if (m) {
          const uint32_t first = (uint32_t)__builtin_amdgcn_readlane((int)bin, __builtin_ctzll(m));
          if (__ballot(in && bin == first) == m) {
            if (lane == (uint32_t)__builtin_ctzll(m)) atomicAdd(&hist[first], (uint32_t)__popcll(m));
          } else if (in) {
            atomicAdd(&hist[bin], 1u);
          }
        }
      }
      __syncthreads();
      // thread t owns bin 255 - t: the keys in the bins above it, and with it
      const uint32_t h = hist[255 - tid];
      uint32_t incl = h;
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= (uint32_t)d) incl += o;
      }
      if (lane == 63) s_wtot[wave] = incl;
      __syncthreads();
#pragma unroll
      for (uint32_t w = 0; w < kSdThreads / 64; ++w) incl += w < wave ? s_wtot[w] : 0u;
      const uint32_t above = incl - h;
      if (above <= want && want < incl) {  // (exactly one thread: want < the keys that carry the prefix)
        s_bin = 255 - tid;
        s_want = want - above;
      }
      __syncthreads();
      prefix = (prefix << 8) | s_bin;
      want = s_want;
    }
    cm = sd_unkey(prefix);
  }
  if (tid == 0) {
    sfmloc_seed_score &o = D.rec[k];
    o.n_inliers = (uint32_t)n;
    o.n_used = n_used;
    o.candidate = (n_used >= D.min_used && cm < D.max_cos && cm > D.min_cos) ? 1u : 0u;
    o.reserved = 0;
    o.cos_median = cm;
  }
}

int seed_device(const PairScene &sc, const PairPoses &po, const sfmloc_seed_options &opt, hipStream_t s, Seed *r) {
  const size_t P = sc.n_pairs, n_inl = (size_t)po.inlier_off[P];
  PairSceneBufs scene;
  PairPosesBufs poses;
  DevBuf<uint64_t> d_key;
  DevBuf<sfmloc_seed_score> d_rec;
  SFM_RC(scene.upload(sc, s));
  SFM_RC(poses.upload(sc, po, s));
  SFM_RC(d_key.alloc(nullptr, n_inl));
  SFM_RC(d_rec.alloc(nullptr, P));
  SFM_RC(d_rec.zero(P, s));
  SdDev D{};
  static_cast<PairDev &>(D) = scene.dev();
  static_cast<PairPosesDev &>(D) = poses.dev();
  D.key = d_key, D.rec = d_rec;
  D.min_used = opt.min_used;
  D.max_cos = opt.max_cos, D.min_cos = opt.min_cos;
  SFM_RC(dev_launch(k_seed_scores, dim3(sc.n_pairs), dim3(kSdThreads), 0, s, D));
  SFM_RC(d_rec.download(r->rec.data(), P, s));
  SFM_HIP(hipStreamSynchronize(s));
  return SFMLOC_OK;
}

int seed_impl(int device, const PairScene &sc, const PairPoses &po, const sfmloc_seed_options &opt, Seed *r) {
  std::string err;
  const int rc = seed_host::check(sc, po, opt, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  r->rec.assign(sc.n_pairs, sfmloc_seed_score{});
  return timed_call(device, &g_seed_last_ms, sc.n_pairs != 0, [&](hipStream_t s) { return seed_device(sc, po, opt, s, r); });
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_seed_default_options(sfmloc_seed_options *o) {
  if (!o) return;
  o->min_used = 100;
  o->reserved = 0;
  o->max_cos = 0.9986295347545738;  // cos 3 degrees
  o->min_cos = 0.5;                 // cos 60 degrees
}

int sfmloc_seed_scores(int device, const uint64_t *view_off, uint32_t n_views, const float *kpt_xy,
                       const uint32_t *view_intrinsic, const double *intrinsics, const uint32_t *intrinsic_type,
                       uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                       const uint32_t *match_i, const uint32_t *match_j, const double *rel_R, const double *rel_t,
                       const uint64_t *inlier_off, const uint32_t *inlier_idx, const uint8_t *use_pair,
                       const sfmloc_seed_options *opt, sfmloc_seed **out) {
  const PairScene sc{view_off,     n_views, kpt_xy,  nullptr, view_intrinsic, intrinsics, intrinsic_type,
                     n_intrinsics, pairs,   n_pairs, offsets, match_i,        match_j};
  const PairPoses po{rel_R, rel_t, inlier_off, inlier_idx, use_pair};
  const sfmloc_seed_options o = options_or(opt, sfmloc_seed_default_options);
  return make_handle<Seed>("sfmloc_seed_scores", out, [&](Seed *r) { return seed_impl(device, sc, po, o, r); });
}

int sfmloc_seed_read(const sfmloc_seed *ss, sfmloc_seed_score *out) {
  SFM_CHECK(ss, SFMLOC_EINVAL, "sfmloc_seed_read: null handle");
  const Seed *r = reinterpret_cast<const Seed *>(ss);
  SFM_CHECK(out || r->rec.empty(), SFMLOC_EINVAL, "sfmloc_seed_read: null argument");
  if (!r->rec.empty()) memcpy(out, r->rec.data(), r->rec.size() * sizeof(sfmloc_seed_score));
  return SFMLOC_OK;
}

void sfmloc_seed_destroy(sfmloc_seed *s) { delete reinterpret_cast<Seed *>(s); }

double sfmloc_seed_last_ms(void) { return g_seed_last_ms; }

}  // extern "C"
