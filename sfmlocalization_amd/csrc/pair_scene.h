// The two-view scene of the pair side (sfmloc_relative_poses, sfmloc_refine_relative_poses, sfmloc_wedge_scales; its
// view-offset and pair-list half is sfmloc_tracks_build's too) as one struct of host pointers, the results of the first
// call that the other two take again as a second, and every check of either that is made before anything is launched.
// Host code only, no HIP: tests/cpp/pair_scene.cpp runs it under the host sanitizers.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <string>

#include "../../include/sfmloc.h"

namespace sfmloc {

// the arguments of include/sfmloc.h "Relative poses", by their names there; view_wh may be null where it is not needed
struct PairScene {
  const uint64_t *view_off;
  uint32_t n_views;
  const float *kpt_xy;
  const uint32_t *view_wh, *view_intrinsic;
  const double *intrinsics;
  const uint32_t *intrinsic_type;
  uint32_t n_intrinsics;
  const uint32_t *pairs;
  uint32_t n_pairs;
  const uint64_t *offsets;
  const uint32_t *match_i, *match_j;
};

// what sfmloc_relative_poses gave for the scene's pairs, and the caller's choice among them (null: all)
struct PairPoses {
  const double *rel_R, *rel_t;
  const uint64_t *inlier_off;
  const uint32_t *inlier_idx;
  const uint8_t *use_pair;
};

namespace pair_host {

constexpr uint64_t kPairMaxM = 65536;  // matches per pair of a two-view call (relpose_host::kLargeMaxM)
// inliers, candidates: every grid and block count the kernels derive from twice this number (two entries per inlier,
// rounded up to a radix block of 1024) stays inside 32 bits
constexpr uint64_t kMaxCount = 0x7FFFFC00ull;

inline int fail(std::string *err, int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                unsigned long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  *err = buf;
  return code;
}

// fail() under the name of the entry point the text speaks for
struct Refuse {
  const char *name;
  std::string *err;
  int operator()(int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                 unsigned long long c = 0) const {
    fail(err, code, fmt, a, b, c);
    *err = std::string(name) + ": " + *err;
    return code;
  }
};

// The walk over the views and the pair list -> SFMLOC_OK, or the code with its text in *err.  need_intr = false: a
// caller without cameras (sfmloc_tracks_build; kpt_xy and the intrinsic arrays are not looked at); need_wh = false: one
// that has no use for the image sizes; cap_pairs: a two-view call, whose pairs hold kPairMaxM matches at most and whose
// match arrays 2^32 - 2.
inline int walk(const char *name, const PairScene &sc, bool need_intr, bool need_wh, bool cap_pairs, std::string *err) {
  const Refuse bad{name, err};
  if (!sc.view_off || sc.n_views == 0) return bad(SFMLOC_EINVAL, "no views");
  if ((need_wh && !sc.view_wh) || (need_intr && !sc.view_intrinsic)) return bad(SFMLOC_EINVAL, "view arrays missing");
  if (need_intr && (!sc.intrinsics || !sc.intrinsic_type || sc.n_intrinsics == 0)) return bad(SFMLOC_EINVAL, "no intrinsics");
  if (sc.view_off[0] != 0) return bad(SFMLOC_EINVAL, "view_off[0] must be 0");
  for (uint32_t v = 0; v < sc.n_views; ++v) {
    if (sc.view_off[v] > sc.view_off[v + 1]) return bad(SFMLOC_EINVAL, "view_off not monotone at %llu", v);
    if (need_intr && sc.view_intrinsic[v] >= sc.n_intrinsics)
      return bad(SFMLOC_EINVAL, "view %llu names intrinsic %llu of %llu", v, sc.view_intrinsic[v], sc.n_intrinsics);
  }
  if (sc.view_off[sc.n_views] > 0xFFFFFFFEull)
    return bad(SFMLOC_ECAP, "%llu feature rows (at most 2^32 - 2)", sc.view_off[sc.n_views]);
  if (need_intr && sc.view_off[sc.n_views] && !sc.kpt_xy) return bad(SFMLOC_EINVAL, "keypoints missing");
  for (uint32_t i = 0; need_intr && i < sc.n_intrinsics; ++i)
    if (sc.intrinsic_type[i] != 0 && sc.intrinsic_type[i] != 3)
      return bad(SFMLOC_EINVAL, "intrinsic %llu has type %llu (0 or 3)", i, sc.intrinsic_type[i]);
  if (sc.n_pairs && (!sc.pairs || !sc.offsets)) return bad(SFMLOC_EINVAL, "pair arrays missing");
  if (sc.n_pairs && sc.offsets[0] != 0) return bad(SFMLOC_EINVAL, "offsets[0] must be 0");
  for (uint32_t k = 0; k < sc.n_pairs; ++k) {
    const uint32_t a = sc.pairs[2 * (size_t)k], b = sc.pairs[2 * (size_t)k + 1];
    if (a >= sc.n_views || b >= sc.n_views) return bad(SFMLOC_EINVAL, "pair %llu = (%llu, %llu) out of range", k, a, b);
    if (a == b) return bad(SFMLOC_EINVAL, "pair %llu names view %llu twice", k, a);
    if (sc.offsets[k] > sc.offsets[k + 1]) return bad(SFMLOC_EINVAL, "offsets not monotone at pair %llu", k);
    const uint64_t n = sc.offsets[k + 1] - sc.offsets[k];
    if (cap_pairs && n > kPairMaxM) return bad(SFMLOC_ECAP, "pair (%llu, %llu) has %llu matches (at most 65536)", a, b, n);
    if (n && (!sc.match_i || !sc.match_j)) return bad(SFMLOC_EINVAL, "match arrays missing");
    const uint64_t na = sc.view_off[a + 1] - sc.view_off[a], nb = sc.view_off[b + 1] - sc.view_off[b];
    for (uint64_t t = 0; t < n; ++t)
      if (sc.match_i[sc.offsets[k] + t] >= na || sc.match_j[sc.offsets[k] + t] >= nb)
        return bad(SFMLOC_EINVAL, "pair (%llu, %llu) match %llu out of range", a, b, t);
  }
  if (cap_pairs && sc.n_pairs && sc.offsets[sc.n_pairs] > 0xFFFFFFFEull)
    return bad(SFMLOC_ECAP, "%llu matches (at most 2^32 - 2)", sc.offsets[sc.n_pairs]);
  return SFMLOC_OK;
}

// The checks of a PairPoses whose scene has passed walk(): sfmloc.h "Wedge scales", the refusals of rel_R, rel_t,
// inlier_off and inlier_idx (use_pair is any bytes)
inline int check_poses(const char *name, const PairScene &sc, const PairPoses &po, std::string *err) {
  const Refuse bad{name, err};
  if (sc.n_pairs && (!po.rel_R || !po.rel_t || !po.inlier_off)) return bad(SFMLOC_EINVAL, "pose or inlier arrays missing");
  if (sc.n_pairs && po.inlier_off[0] != 0) return bad(SFMLOC_EINVAL, "inlier_off[0] must be 0");
  for (uint32_t k = 0; k < sc.n_pairs; ++k) {
    const uint32_t a = sc.pairs[2 * (size_t)k], b = sc.pairs[2 * (size_t)k + 1];
    if (po.inlier_off[k] > po.inlier_off[k + 1]) return bad(SFMLOC_EINVAL, "inlier_off not monotone at pair %llu", k);
    const uint64_t n = po.inlier_off[k + 1] - po.inlier_off[k], m = sc.offsets[k + 1] - sc.offsets[k];
    if (po.inlier_off[k + 1] > kMaxCount)
      return bad(SFMLOC_ECAP, "%llu inliers up to pair %llu (at most 2^31 - 1024)", po.inlier_off[k + 1], k);
    if (n && !po.inlier_idx) return bad(SFMLOC_EINVAL, "inlier_idx missing");
    for (uint64_t p = 0; p < n; ++p)
      if (po.inlier_idx[po.inlier_off[k] + p] >= m)
        return bad(SFMLOC_EINVAL, "pair (%llu, %llu) inlier %llu out of range", a, b, p);
    for (int i = 0; i < 12; ++i)
      if (!isfinite(i < 9 ? po.rel_R[9 * (size_t)k + i] : po.rel_t[3 * (size_t)k + i - 9]))
        return bad(SFMLOC_EINVAL, "pair (%llu, %llu) has a non-finite rel_R or rel_t", a, b);
  }
  return SFMLOC_OK;
}

}  // namespace pair_host
}  // namespace sfmloc
