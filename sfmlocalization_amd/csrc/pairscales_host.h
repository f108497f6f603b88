// The host side of sfmloc_wedge_scales (pairscales.hip): every check the call makes before anything is launched (the
// scene's and the poses' are pair_scene.h's, the options' are here), the per-view lists of pairs the kernels enumerate
// candidates from; and of sfmloc_global_poses_scaled (globalposes.hip): the checks of its wedge list and the adjacency
// of the scale graph.  Host code only, no HIP: tests/cpp/pairscales_host.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "pair_scene.h"

namespace sfmloc {
namespace wscales_host {

constexpr uint32_t kWaveDegree = 64;       // a view of more used pairs than this is enumerated by a wave, not by a lane
constexpr uint32_t kSideBit = 0x80000000u;  // in ViewPairs::ent: the view is the pair's J
constexpr uint32_t kMaxShared = 2048;      // the ratios one workgroup sorts in LDS
using pair_host::fail;
using pair_host::kMaxCount;

// sfmloc.h "candidates": the entries of view v are off[v] .. off[v + 1], the used pairs that name v ascending by pair
// index, with kSideBit when v is the pair's J.  cand[v] = the candidates of the views before v (d (d - 1) / 2 each);
// heavy = the views of more than kWaveDegree entries, ascending.
struct ViewPairs {
  std::vector<uint32_t> off, ent, cand, heavy;
  uint32_t n_used = 0, n_inliers = 0;
};

// sfmloc.h "Refusals" -> SFMLOC_OK and the lists, or the code with its text in *err and *vp untouched
inline int check(const PairScene &sc, const PairPoses &po, const sfmloc_wscales_options &opt, ViewPairs *vp,
                 std::string *err) {
  static const char *const name = "sfmloc_wedge_scales";
  const uint32_t n_views = sc.n_views, n_pairs = sc.n_pairs;
  if (n_pairs > 0x3FFFFFFFu) return fail(err, SFMLOC_ECAP, "sfmloc_wedge_scales: %llu pairs (at most 2^30 - 1)", n_pairs);
  const int rc = pair_host::walk(name, sc, true, false, true, err);
  if (rc) return rc;
  if (opt.min_shared < 1) return fail(err, SFMLOC_EINVAL, "sfmloc_wedge_scales: min_shared = %llu (at least 1)", opt.min_shared);
  if (opt.max_shared < 1 || opt.max_shared > kMaxShared)
    return fail(err, SFMLOC_EINVAL, "sfmloc_wedge_scales: max_shared = %llu (1 to 2048)", opt.max_shared);
  const int rc_inl = pair_host::check_poses(name, sc, po, err);
  if (rc_inl) return rc_inl;
  std::vector<uint32_t> off((size_t)n_views + 1, 0);
  uint32_t n_used = 0;
  uint64_t n_inl = 0;
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = sc.pairs[2 * (size_t)k], b = sc.pairs[2 * (size_t)k + 1];
    if (po.use_pair && !po.use_pair[k]) continue;
    ++n_used;
    n_inl += po.inlier_off[k + 1] - po.inlier_off[k];
    ++off[a + 1];
    ++off[b + 1];
  }
  std::vector<uint32_t> cand((size_t)n_views + 1, 0), heavy;
  uint64_t total = 0;
  for (uint32_t v = 0; v < n_views; ++v) {
    const uint64_t d = off[v + 1];
    total += d ? d * (d - 1) / 2 : 0;
    if (d > kWaveDegree) heavy.push_back(v);
    if (total > kMaxCount)
      return fail(err, SFMLOC_ECAP, "sfmloc_wedge_scales: %llu candidate wedges up to view %llu (at most 2^31 - 1024)", total, v);
    cand[v + 1] = (uint32_t)total;
    off[v + 1] += off[v];
  }
  std::vector<uint32_t> ent(2 * (size_t)n_used), at(off.begin(), off.end() - 1);
  for (uint32_t k = 0; k < n_pairs; ++k) {  // (ascending k: every view's entries come out ascending)
    if (po.use_pair && !po.use_pair[k]) continue;
    ent[at[sc.pairs[2 * (size_t)k]]++] = k;
    ent[at[sc.pairs[2 * (size_t)k + 1]]++] = k | kSideBit;
  }
  vp->off.swap(off);
  vp->ent.swap(ent);
  vp->cand.swap(cand);
  vp->heavy.swap(heavy);
  vp->n_used = n_used;
  vp->n_inliers = (uint32_t)n_inl;
  return SFMLOC_OK;
}

// sfmloc.h "Scaled global poses", the refusals of the wedge list (the pair list has passed gposes_host::check)
inline int check_wedges(const uint32_t *pairs, uint32_t n_pairs, const uint32_t *kl, const double *ratio, uint32_t n_wedges,
                        std::string *err) {
  if (n_wedges && (!kl || !ratio)) return fail(err, SFMLOC_EINVAL, "sfmloc_global_poses_scaled: wedge arrays missing");
  std::vector<uint64_t> keys(n_wedges);
  for (uint32_t w = 0; w < n_wedges; ++w) {
    const uint32_t k = kl[2 * (size_t)w], l = kl[2 * (size_t)w + 1];
    if (k >= n_pairs || l >= n_pairs)
      return fail(err, SFMLOC_EINVAL, "sfmloc_global_poses_scaled: wedge %llu = pairs (%llu, %llu) out of range", w, k, l);
    if (k >= l) return fail(err, SFMLOC_EINVAL, "sfmloc_global_poses_scaled: wedge %llu = pairs (%llu, %llu): k must be below l", w, k, l);
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1], c = pairs[2 * (size_t)l], d = pairs[2 * (size_t)l + 1];
    if (a != c && a != d && b != c && b != d)
      return fail(err, SFMLOC_EINVAL, "sfmloc_global_poses_scaled: wedge %llu = pairs (%llu, %llu) share no view", w, k, l);
    keys[w] = ((uint64_t)k << 32) | l;
  }
  std::sort(keys.begin(), keys.end());
  for (uint32_t w = 1; w < n_wedges; ++w)
    if (keys[w] == keys[w - 1])
      return fail(err, SFMLOC_EINVAL, "sfmloc_global_poses_scaled: the wedge of pairs (%llu, %llu) is listed twice", keys[w] >> 32,
                  keys[w] & 0xFFFFFFFFull);
  return SFMLOC_OK;
}

// sfmloc.h "scales": CSR by node (= pair) over both ends of every wedge with on[w], a node's entries ascending by
// neighbour; pe = the wedge's index, with kSideBit when the node is the wedge's l.  heavy = the nodes of more than
// kWaveDegree entries, ascending.  Every entry is written at its own place: a gather on the device, never a scatter.
struct ScaleGraph {
  std::vector<uint32_t> off, nbr, pe, heavy;
};

inline void scale_adjacency(uint32_t n_pairs, const uint32_t *kl, const uint8_t *on, uint32_t n_wedges, ScaleGraph *g) {
  std::vector<uint32_t> off((size_t)n_pairs + 1, 0);
  for (uint32_t w = 0; w < n_wedges; ++w)
    if (on[w]) {
      ++off[kl[2 * (size_t)w] + 1];
      ++off[kl[2 * (size_t)w + 1] + 1];
    }
  for (uint32_t v = 0; v < n_pairs; ++v) off[v + 1] += off[v];
  std::vector<uint64_t> ent(off[n_pairs]);  // (neighbour, entry): sorted as one number
  std::vector<uint32_t> at(off.begin(), off.end() - 1);
  for (uint32_t w = 0; w < n_wedges; ++w)
    if (on[w]) {
      const uint32_t k = kl[2 * (size_t)w], l = kl[2 * (size_t)w + 1];
      ent[at[k]++] = ((uint64_t)l << 32) | w;
      ent[at[l]++] = ((uint64_t)k << 32) | w | kSideBit;
    }
  g->nbr.resize(ent.size());
  g->pe.resize(ent.size());
  g->heavy.clear();
  for (uint32_t v = 0; v < n_pairs; ++v) {
    std::sort(ent.begin() + off[v], ent.begin() + off[v + 1]);
    if (off[v + 1] - off[v] > kWaveDegree) g->heavy.push_back(v);
  }
  for (size_t e = 0; e < ent.size(); ++e) {
    g->nbr[e] = (uint32_t)(ent[e] >> 32);
    g->pe[e] = (uint32_t)ent[e];
  }
  g->off.swap(off);
}

// the lower median: element (n - 1) / 2 of the sorted values (n > 0)
inline double lower_median(std::vector<double> v) {
  std::sort(v.begin(), v.end());
  return v[(v.size() - 1) / 2];
}

}  // namespace wscales_host
}  // namespace sfmloc
