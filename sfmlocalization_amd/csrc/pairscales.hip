// sfmloc_wedge_scales: the ratio of the baselines of two pairs that share a view, from the depths of the features they
// share.  The semantics are stated in include/sfmloc.h ("Wedge scales"); tests/pairscales_np.py restates every operation.
// f64, unfused (the library's -ffp-contract=off), only + - * / sqrt; after the depths nothing but comparisons and one
// division per shared feature, no float atomics: the records are the restatement's bits.  Scene and poses: PairScene and
// PairPoses on the host (pair_scene.h), PairDev and PairPosesDev on the device (twoview_device.h), the bases of WsDev.
//
//   depths      k_ws_depths: one workgroup per pair walks its inlier list; a match gives one entry per side (pair side,
//               feature, depth), the pair side of a match that yields nothing being one past the last.
//   lists       two stable radix sorts of all entries (radix_sort.h): by feature, then by pair side.  Ties keep the order
//               of the inlier list, so the first entry of a feature's run is the one the semantics keep, and a lower
//               bound finds it: nothing is compacted.  k_ws_bounds: where each pair side begins.
//   candidates  k_ws_enum: a lane per view, a wave per view of more than wscales_host::kWaveDegree pairs.
//   count       k_ws_count: one wave per candidate, 64 features of the shorter list at a time.
//   choice      k_ws_flag, radix_sort.h's k_scan_excl, k_ws_compact: the candidates with min_shared features and more, in
//               place order; then three stable sorts of their places, by view, by l, by k.  The host reads one count.
//   ratio       k_ws_ratio: one workgroup per kept record in that order; wave 0 gathers the quotients in feature order into
//               LDS (the ballot's prefix gives the place), the workgroup sorts them (ransac_device.h's bitonic sort).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "pairscales_host.h"
#include "radix_sort.h"
#include "ransac_device.h"
#include "twoview_device.h"

namespace sfmloc {
namespace {

using wscales_host::kSideBit;
using wscales_host::kWaveDegree;
constexpr int kWsMaxShared = (int)wscales_host::kMaxShared;

thread_local double g_wscales_last_ms = 0.0;

struct Wscales {
  std::vector<sfmloc_wscale> rec;
  sfmloc_wscales_report rep{};
};

struct WsDev : PairDev, PairPosesDev {
  uint32_t n_ent, nb_view, n_heavy;
  const uint32_t *voff, *vent, *vcand, *heavy;
  uint32_t *feat, *seg;    // per entry, entry 2 t + side of inlier t
  double *z;
  const uint32_t *feat_s;  // the entries in the lists' order
  const double *z_s;
  const uint32_t *seg_begin;  // [2 n_pairs + 1]
};

// sfmloc.h "depths".  keys / ids: the first sort's input (the feature again, and the entry's own index)
__global__ __launch_bounds__(256) void k_ws_depths(WsDev D, uint32_t *keys, uint32_t *ids) {
  const uint32_t k = blockIdx.x;
  if (k >= D.n_pairs) return;
  const uint32_t vi = D.pairs[2 * (size_t)k], vj = D.pairs[2 * (size_t)k + 1];
  const double *R = D.relR + 9 * (size_t)k, *t = D.relt + 3 * (size_t)k;
  const bool used = D.use[k];
  const uint64_t m0 = D.offsets[k];
  for (uint64_t p = D.inl_off[k] + threadIdx.x; p < D.inl_off[k + 1]; p += 256) {
    const uint64_t mt = m0 + D.inl_idx[p];
    const uint32_t fi = D.match_i[mt], fj = D.match_j[mt];
    double zi = 0.0, zj = 0.0;
    bool ok = false;
    if (used) {
      double a, b, u, v;
      feature_bearing(D, view_cam(D, vi), fi, &a, &b);
      feature_bearing(D, view_cam(D, vj), fj, &u, &v);
      ok = two_view_depths(R, t, a, b, u, v, &zi, &zj) && is_finite(zj) && zi > 0.0 && zj > 0.0;
    }
    const uint32_t e = 2 * (uint32_t)p;
    D.feat[e] = keys[e] = fi;
    D.feat[e + 1] = keys[e + 1] = fj;
    D.seg[e] = ok ? 2 * k : 2 * D.n_pairs;
    D.seg[e + 1] = ok ? 2 * k + 1 : 2 * D.n_pairs;
    D.z[e] = zi;
    D.z[e + 1] = zj;
    ids[e] = e;
    ids[e + 1] = e + 1;
  }
}

// the second sort's keys: the pair side of the entries in the first sort's order
__global__ __launch_bounds__(256) void k_ws_segkeys(WsDev D, const uint32_t *ids, uint32_t *keys) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < D.n_ent) keys[i] = D.seg[ids[i]];
}

__global__ __launch_bounds__(256) void k_ws_gather(WsDev D, const uint32_t *ids, uint32_t *feat_s, double *z_s) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= D.n_ent) return;
  feat_s[i] = D.feat[ids[i]];
  z_s[i] = D.z[ids[i]];
}

// the first place in a[lo .. hi) whose value is not below x
__device__ __forceinline__ uint32_t ws_lower_bound(const uint32_t *a, uint32_t lo, uint32_t hi, uint32_t x) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (a[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// seg_begin[s] for s = 0 .. 2 n_pairs: the entries of pair side s are seg_begin[s] .. seg_begin[s + 1]
__global__ __launch_bounds__(256) void k_ws_bounds(WsDev D, const uint32_t *seg_s, uint32_t *seg_begin) {
  const uint32_t s = blockIdx.x * 256 + threadIdx.x;
  if (s <= 2 * D.n_pairs) seg_begin[s] = ws_lower_bound(seg_s, 0, D.n_ent, s);
}

// sfmloc.h "candidates": view v's are rec[vcand[v] .. vcand[v + 1]), row a = (a, a + 1), (a, a + 2), ...
__global__ __launch_bounds__(256) void k_ws_enum(WsDev D, sfmloc_wscale *rec) {
  uint32_t v;
  bool wave;
  if (blockIdx.x < D.nb_view) {
    wave = false;
    v = blockIdx.x * 256 + threadIdx.x;
    if (v >= D.n_views || D.voff[v + 1] - D.voff[v] > kWaveDegree) return;
  } else {
    wave = true;
    const uint32_t w = (blockIdx.x - D.nb_view) * 4 + (threadIdx.x >> 6);
    if (w >= D.n_heavy) return;
    v = D.heavy[w];
  }
  const uint32_t b0 = D.voff[v], d = D.voff[v + 1] - b0;
  const uint32_t first = wave ? (threadIdx.x & 63) : 0, step = wave ? 64 : 1;
  for (uint32_t a = 0; a + 1 < d; ++a) {
    const uint64_t row = (uint64_t)D.vcand[v] + ((uint64_t)a * (2 * (uint64_t)d - a - 1)) / 2;
    const uint32_t ka = D.vent[b0 + a] & ~kSideBit;
    for (uint32_t b = a + 1 + first; b < d; b += step) {
      sfmloc_wscale &o = rec[row + (b - a - 1)];
      o.view = v;
      o.k = ka;
      o.l = D.vent[b0 + b] & ~kSideBit;
      o.n_shared = 0;
      o.ratio = 0.0;
    }
  }
}

// the two lists of a record's view: [*bs, *es) the shorter (the one walked), [*bg, *eg) the other; true: the walked one is k's
__device__ __forceinline__ bool ws_lists(const WsDev &D, const sfmloc_wscale &w, uint32_t *bs, uint32_t *es, uint32_t *bg,
                                         uint32_t *eg) {
  const uint32_t sk = 2 * w.k + (D.pairs[2 * (size_t)w.k + 1] == w.view ? 1u : 0u);
  const uint32_t sl = 2 * w.l + (D.pairs[2 * (size_t)w.l + 1] == w.view ? 1u : 0u);
  const uint32_t bk = D.seg_begin[sk], ek = D.seg_begin[sk + 1], bl = D.seg_begin[sl], el = D.seg_begin[sl + 1];
  const bool walk_k = ek - bk <= el - bl;
  *bs = walk_k ? bk : bl;
  *es = walk_k ? ek : el;
  *bg = walk_k ? bl : bk;
  *eg = walk_k ? el : ek;
  return walk_k;
}

// entry i of the walked list: is it the first of its feature, and is the feature in the other list -> its place there
__device__ __forceinline__ bool ws_shared(const WsDev &D, uint32_t i, uint32_t bs, uint32_t es, uint32_t bg, uint32_t eg,
                                          uint32_t *at) {
  if (i >= es) return false;
  const uint32_t f = D.feat_s[i];
  if (i > bs && D.feat_s[i - 1] == f) return false;
  *at = ws_lower_bound(D.feat_s, bg, eg, f);
  return *at < eg && D.feat_s[*at] == f;
}

// sfmloc.h "count": one wave per candidate
__global__ __launch_bounds__(256) void k_ws_count(WsDev D, sfmloc_wscale *rec, uint32_t n_rec) {
  const uint32_t c = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= n_rec) return;
  uint32_t bs, es, bg, eg, at;
  ws_lists(D, rec[c], &bs, &es, &bg, &eg);
  uint32_t n = 0;
  for (uint32_t base = bs; base < es; base += 64)
    n += (uint32_t)__popcll(__ballot(ws_shared(D, base + (threadIdx.x & 63), bs, es, bg, eg, &at)));
  if ((threadIdx.x & 63) == 0) rec[c].n_shared = n;
}

// sfmloc.h "count", the choice: flag[c] = the candidate is kept; flag[n_cand] = 0, where the scan leaves the total
__global__ __launch_bounds__(256) void k_ws_flag(const sfmloc_wscale *rec, uint32_t n_cand, uint32_t min_shared,
                                                 uint32_t *flag) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c <= n_cand) flag[c] = (c < n_cand && rec[c].n_shared >= min_shared) ? 1u : 0u;
}

// the kept candidates, in the candidates' order, at the places the scan of the flags gives
__global__ __launch_bounds__(256) void k_ws_compact(const sfmloc_wscale *rec, uint32_t n_cand, uint32_t min_shared,
                                                    const uint32_t *place, sfmloc_wscale *kept) {
  const uint32_t c = blockIdx.x * 256 + threadIdx.x;
  if (c < n_cand && rec[c].n_shared >= min_shared) kept[place[c]] = rec[c];
}

// a sort pass's keys: field 0 view, 1 l, 2 k of the kept records in the order `ids` (null: as they stand, and ids_out
// is set to it)
__global__ __launch_bounds__(256) void k_ws_keys(const sfmloc_wscale *kept, uint32_t n, const uint32_t *ids, int field,
                                                 uint32_t *keys, uint32_t *ids_out) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const sfmloc_wscale &w = kept[ids ? ids[i] : i];
  keys[i] = field == 0 ? w.view : field == 1 ? w.l : w.k;
  if (!ids) ids_out[i] = i;
}

// sfmloc.h "ratio": one workgroup per record; record c of the result is kept[order[c]] with its ratio
__global__ __launch_bounds__(kThreads) void k_ws_ratio(WsDev D, const sfmloc_wscale *kept, const uint32_t *order,
                                                       sfmloc_wscale *rec, uint32_t n_rec, uint32_t max_shared) {
  __shared__ uint64_t key[kWsMaxShared];
  __shared__ uint32_t idx[kWsMaxShared];
  __shared__ uint32_t s_n;
  const uint32_t c = blockIdx.x;
  if (c >= n_rec) return;
  const sfmloc_wscale w = kept[order[c]];
  if (threadIdx.x < 64) {
    uint32_t bs, es, bg, eg;
    const bool walk_k = ws_lists(D, w, &bs, &es, &bg, &eg);
    const uint32_t lane = threadIdx.x;
    const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t n = 0;
    for (uint32_t base = bs; base < es && n < max_shared; base += 64) {
      uint32_t at = 0;
      const bool hit = ws_shared(D, base + lane, bs, es, bg, eg, &at);
      const unsigned long long m = __ballot(hit);
      const uint32_t place = n + (uint32_t)__popcll(m & below);
      if (hit && place < max_shared) {
        const double zs = D.z_s[base + lane], zg = D.z_s[at];
        key[place] = d2u(walk_k ? zs / zg : zg / zs);  // (a quotient of positive depths: its bits order as it does)
        idx[place] = D.feat_s[base + lane];
      }
      n += (uint32_t)__popcll(m);
    }
    if (lane == 0) s_n = n < max_shared ? n : max_shared;
  }
  __syncthreads();
  const int n = (int)s_n;
  if (threadIdx.x == 0) {
    rec[c] = w;
    rec[c].ratio = 0.0;
  }
  if (n == 0) return;  // (min_shared >= 1: no such record is kept)
  const int P = next_pow2(n);
  for (int i = n + threadIdx.x; i < P; i += kThreads) {
    key[i] = ~0ull;
    idx[i] = ~0u;
  }
  __syncthreads();
  bitonic_sort(key, idx, P);
  if (threadIdx.x == 0) rec[c].ratio = u2d(key[(n - 1) / 2]);
}

// a launch, counted in the call's report
template <class... Ts, class... As>
int ws_launch(sfmloc_wscales_report &rep, void (*kernel)(Ts...), uint32_t grid, uint32_t block, LaunchStream on, As &&...as) {
  ++rep.launches;
  return dev_launch(kernel, dim3(grid), dim3(block), 0, on, as...);
}

int wscales_device(const PairScene &sc, const PairPoses &po, const sfmloc_wscales_options &opt,
                   const wscales_host::ViewPairs &vp, hipStream_t s, Wscales *w) {
  sfmloc_wscales_report &rep = w->rep;
  const uint32_t n_views = sc.n_views, n_pairs = sc.n_pairs;
  const size_t P = n_pairs, n = n_views, n_inl = (size_t)po.inlier_off[n_pairs], n_ent = 2 * n_inl;
  const uint32_t n_cand = vp.cand[n_views];
  rep.n_candidates = n_cand;
  if (n_ent == 0 || n_cand == 0) return SFMLOC_OK;  // no depth, or no two pairs at one view: no wedge
  uint32_t max_feat = 0;
  for (size_t v = 0; v < n; ++v)
    if (sc.view_off[v + 1] - sc.view_off[v] > max_feat) max_feat = (uint32_t)(sc.view_off[v + 1] - sc.view_off[v]);
  PairSceneBufs scene;
  PairPosesBufs poses;
  DevBuf<uint32_t> d_voff, d_vent, d_vcand, d_heavy;
  DevBuf<uint32_t> d_feat, d_seg, d_ka, d_va, d_kb, d_vb, d_hist, d_feat_s, d_seg_begin;
  DevBuf<double> d_z, d_z_s;
  DevBuf<sfmloc_wscale> d_rec, d_out;
  SFM_RC(scene.upload(sc, s));
  SFM_RC(poses.upload(sc, po, s));
  SFM_RC(dev_upload(nullptr, d_voff, vp.off.data(), n + 1, s));
  SFM_RC(dev_upload(nullptr, d_vent, vp.ent.data(), vp.ent.size(), s));
  SFM_RC(dev_upload(nullptr, d_vcand, vp.cand.data(), n + 1, s));
  SFM_RC(dev_upload(nullptr, d_heavy, vp.heavy.data(), vp.heavy.size(), s, 1));
  SFM_RC(d_feat.alloc(nullptr, n_ent));
  SFM_RC(d_seg.alloc(nullptr, n_ent));
  SFM_RC(d_z.alloc(nullptr, n_ent));
  SFM_RC(d_ka.alloc(nullptr, n_ent));
  SFM_RC(d_va.alloc(nullptr, n_ent));
  SFM_RC(d_kb.alloc(nullptr, n_ent));
  SFM_RC(d_vb.alloc(nullptr, n_ent));
  SFM_RC(d_hist.alloc(nullptr, radix_hist_entries(n_ent)));
  SFM_RC(d_feat_s.alloc(nullptr, n_ent));
  SFM_RC(d_z_s.alloc(nullptr, n_ent));
  SFM_RC(d_seg_begin.alloc(nullptr, 2 * P + 1));
  SFM_RC(d_rec.alloc(nullptr, n_cand));
  WsDev D{};
  static_cast<PairDev &>(D) = scene.dev();
  static_cast<PairPosesDev &>(D) = poses.dev();
  D.n_ent = (uint32_t)n_ent;
  D.nb_view = (n_views + 255) / 256;
  D.n_heavy = (uint32_t)vp.heavy.size();
  D.voff = d_voff, D.vent = d_vent, D.vcand = d_vcand, D.heavy = d_heavy;
  D.feat = d_feat, D.seg = d_seg, D.z = d_z, D.feat_s = d_feat_s, D.z_s = d_z_s, D.seg_begin = d_seg_begin;
  const uint32_t ge = ((uint32_t)n_ent + 255) / 256;

  // sfmloc.h "depths", "lists"
  SFM_RC(ws_launch(rep, k_ws_depths, n_pairs, 256, s, D, d_ka, d_va));
  uint32_t *ks = d_ka, *vs = d_va, *ko = d_kb, *vo = d_vb;  // (ks, vs): where the sorted pairs are; (ko, vo): the scratch
  auto sort = [&](int bits) {
    rep.launches += 3 * (uint32_t)((bits + 7) / 8);
    bool swapped = false;
    SFM_RC(radix_sort_pairs(ks, vs, ko, vo, (uint32_t)n_ent, bits, d_hist, s, &swapped));
    if (swapped) {
      std::swap(ks, ko);
      std::swap(vs, vo);
    }
    return (int)SFMLOC_OK;
  };
  SFM_RC(sort(radix_key_bits(max_feat ? max_feat - 1 : 0)));
  SFM_RC(ws_launch(rep, k_ws_segkeys, ge, 256, s, D, vs, ko));
  std::swap(ks, ko);  // (the sorted features are not needed again: k_ws_gather reads the entries')
  SFM_RC(sort(radix_key_bits(2 * n_pairs)));
  SFM_RC(ws_launch(rep, k_ws_gather, ge, 256, s, D, vs, d_feat_s, d_z_s));
  SFM_RC(ws_launch(rep, k_ws_bounds, (2 * n_pairs + 1 + 255) / 256, 256, s, D, ks, d_seg_begin));
  // sfmloc.h "candidates", "count"
  SFM_RC(ws_launch(rep, k_ws_enum, D.nb_view + (D.n_heavy + 3) / 4, 256, s, D, d_rec));
  SFM_RC(ws_launch(rep, k_ws_count, (n_cand + 3) / 4, 256, s, D, d_rec, n_cand));
  // the choice and the order of the records, on the device: flag, scan, compact; then three stable sorts of the kept
  // records' places, by view, by l and by k
  DevBuf<uint32_t> d_place;
  SFM_RC(d_place.alloc(nullptr, (size_t)n_cand + 1));
  SFM_RC(d_out.alloc(nullptr, n_cand));
  SFM_RC(ws_launch(rep, k_ws_flag, n_cand / 256 + 1, 256, s, d_rec, n_cand, opt.min_shared, d_place));
  SFM_RC(ws_launch(rep, k_scan_excl, 1, 1024, s, d_place, n_cand + 1));
  SFM_RC(ws_launch(rep, k_ws_compact, (n_cand + 255) / 256, 256, s, d_rec, n_cand, opt.min_shared, d_place, d_out));
  uint32_t n_yield = 0, n_rec = 0;
  SFM_RC(d_place.download(&n_rec, 1, s, n_cand));
  SFM_RC(d_seg_begin.download(&n_yield, 1, s, 2 * P));
  SFM_HIP(hipStreamSynchronize(s));
  rep.n_depths = n_yield / 2;
  std::vector<sfmloc_wscale> rec(n_rec);
  if (n_rec) {
    DevBuf<uint32_t> d_k0, d_v0, d_k1, d_v1, d_h;
    DevBuf<sfmloc_wscale> d_final;
    SFM_RC(d_k0.alloc(nullptr, n_rec));
    SFM_RC(d_v0.alloc(nullptr, n_rec));
    SFM_RC(d_k1.alloc(nullptr, n_rec));
    SFM_RC(d_v1.alloc(nullptr, n_rec));
    SFM_RC(d_h.alloc(nullptr, radix_hist_entries(n_rec)));
    SFM_RC(d_final.alloc(nullptr, n_rec));
    uint32_t *rk = d_k0, *rv = d_v0, *ok = d_k1, *ov = d_v1;  // (rk, rv): keys and places in the order so far
    const int bits[3] = {radix_key_bits(n_views - 1), radix_key_bits(n_pairs - 1), radix_key_bits(n_pairs - 1)};
    for (int field = 0; field < 3; ++field) {
      SFM_RC(ws_launch(rep, k_ws_keys, (n_rec + 255) / 256, 256, s, d_out, n_rec, field ? rv : nullptr, field, rk, rv));
      rep.launches += 3 * (uint32_t)((bits[field] + 7) / 8);
      bool swapped = false;
      SFM_RC(radix_sort_pairs(rk, rv, ok, ov, n_rec, bits[field], d_h, s, &swapped));
      if (swapped) {
        std::swap(rk, ok);
        std::swap(rv, ov);
      }
    }
    // sfmloc.h "ratio"
    SFM_RC(ws_launch(rep, k_ws_ratio, n_rec, kThreads, s, D, d_out, rv, d_final, n_rec, opt.max_shared));
    SFM_RC(d_final.download(rec.data(), rec.size(), s));
    SFM_HIP(hipStreamSynchronize(s));
  }
  w->rec.swap(rec);
  rep.n_wedges = (uint32_t)w->rec.size();
  return SFMLOC_OK;
}

int wscales_impl(int device, const PairScene &sc, const PairPoses &po, const sfmloc_wscales_options &opt, Wscales *w) {
  wscales_host::ViewPairs vp;
  std::string err;
  const int rc = wscales_host::check(sc, po, opt, &vp, &err);
  SFM_CHECK(rc == SFMLOC_OK, rc, "%s", err.c_str());
  w->rep.n_pairs = sc.n_pairs;
  w->rep.n_pairs_used = vp.n_used;
  w->rep.n_inliers = vp.n_inliers;
  SFM_RC(timed_call(device, &g_wscales_last_ms, sc.n_pairs != 0,
                    [&](hipStream_t s) { return wscales_device(sc, po, opt, vp, s, w); }));
  w->rep.device_ms = g_wscales_last_ms;
  return SFMLOC_OK;
}

}  // namespace
}  // namespace sfmloc

using namespace sfmloc;

extern "C" {

void sfmloc_wscales_default_options(sfmloc_wscales_options *o) {
  if (!o) return;
  o->min_shared = 8;
  o->max_shared = wscales_host::kMaxShared;
}

int sfmloc_wedge_scales(int device, const uint64_t *view_off, uint32_t n_views, const float *kpt_xy,
                        const uint32_t *view_intrinsic, const double *intrinsics, const uint32_t *intrinsic_type,
                        uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                        const uint32_t *match_i, const uint32_t *match_j, const double *rel_R, const double *rel_t,
                        const uint64_t *inlier_off, const uint32_t *inlier_idx, const uint8_t *use_pair,
                        const sfmloc_wscales_options *opt, sfmloc_wscales **out) {
  const PairScene sc{view_off,     n_views, kpt_xy,  nullptr, view_intrinsic, intrinsics, intrinsic_type,
                     n_intrinsics, pairs,   n_pairs, offsets, match_i,        match_j};
  const PairPoses po{rel_R, rel_t, inlier_off, inlier_idx, use_pair};
  const sfmloc_wscales_options o = options_or(opt, sfmloc_wscales_default_options);
  return make_handle<Wscales>("sfmloc_wedge_scales", out, [&](Wscales *w) { return wscales_impl(device, sc, po, o, w); });
}

int sfmloc_wscales_count(const sfmloc_wscales *ww, uint32_t *n_wedges) {
  SFM_CHECK(ww && n_wedges, SFMLOC_EINVAL, "sfmloc_wscales_count: null argument");
  *n_wedges = (uint32_t) reinterpret_cast<const Wscales *>(ww)->rec.size();
  return SFMLOC_OK;
}

int sfmloc_wscales_read(const sfmloc_wscales *ww, sfmloc_wscale *out) {
  SFM_CHECK(ww, SFMLOC_EINVAL, "sfmloc_wscales_read: null handle");
  const Wscales *w = reinterpret_cast<const Wscales *>(ww);
  SFM_CHECK(out || w->rec.empty(), SFMLOC_EINVAL, "sfmloc_wscales_read: null argument");
  if (!w->rec.empty()) memcpy(out, w->rec.data(), w->rec.size() * sizeof(sfmloc_wscale));
  return SFMLOC_OK;
}

int sfmloc_wscales_report_read(const sfmloc_wscales *ww, sfmloc_wscales_report *rep) {
  SFM_CHECK(ww && rep, SFMLOC_EINVAL, "sfmloc_wscales_report_read: null argument");
  *rep = reinterpret_cast<const Wscales *>(ww)->rep;
  return SFMLOC_OK;
}

void sfmloc_wscales_destroy(sfmloc_wscales *w) { delete reinterpret_cast<Wscales *>(w); }

double sfmloc_wscales_last_ms(void) { return g_wscales_last_ms; }

}  // extern "C"
