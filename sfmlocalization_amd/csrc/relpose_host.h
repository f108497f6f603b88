// The host side of sfmloc_relative_poses (relpose.hip): every check the call makes before anything is launched, and the
// split of the pair list into the pairs the LDS form takes and the ones that need a global-memory slot.  Host code only,
// no HIP: tests/cpp/relpose_host.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/sfmloc.h"

namespace sfmloc {
namespace relpose_host {

constexpr uint32_t kLdsMaxM = 2048;     // matches per pair the LDS form holds (forms.h kFMaxM)
constexpr uint32_t kLargeMaxM = 65536;  // matches per pair a global-memory slot holds (K3's kFLargeMaxM)

inline int fail(std::string *err, int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                unsigned long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  *err = buf;
  return code;
}

// -> SFMLOC_OK, the pairs with more than kLdsMaxM matches in *large (pair order) and the longest of them in
// *large_max_m; or the error code with its text in *err and the outputs untouched.  `name` is the entry point the text
// speaks for; need_wh = false: a caller that has no use for the image sizes (sfmloc_wedge_scales) passes no view_wh.
inline int check(const uint64_t *view_off, uint32_t n_views, const float *kpt_xy, const uint32_t *view_wh,
                 const uint32_t *view_intrinsic, const double *intrinsics, const uint32_t *intrinsic_type,
                 uint32_t n_intrinsics, const uint32_t *pairs, uint32_t n_pairs, const uint64_t *offsets,
                 const uint32_t *match_i, const uint32_t *match_j, std::vector<uint32_t> *large, uint32_t *large_max_m,
                 std::string *err, const char *name = "sfmloc_relative_poses", bool need_wh = true) {
  const auto bad = [&](int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                       unsigned long long c = 0) {
    fail(err, code, fmt, a, b, c);
    *err = std::string(name) + ": " + *err;
    return code;
  };
  if (!view_off || n_views == 0) return bad(SFMLOC_EINVAL, "no views");
  if ((need_wh && !view_wh) || !view_intrinsic) return bad(SFMLOC_EINVAL, "view arrays missing");
  if (!intrinsics || !intrinsic_type || n_intrinsics == 0)
    return bad(SFMLOC_EINVAL, "no intrinsics");
  if (view_off[0] != 0) return bad(SFMLOC_EINVAL, "view_off[0] must be 0");
  for (uint32_t v = 0; v < n_views; ++v) {
    if (view_off[v] > view_off[v + 1])
      return bad(SFMLOC_EINVAL, "view_off not monotone at %llu", v);
    if (view_intrinsic[v] >= n_intrinsics)
      return bad(SFMLOC_EINVAL, "view %llu names intrinsic %llu of %llu", v,
                  view_intrinsic[v], n_intrinsics);
  }
  if (view_off[n_views] > 0xFFFFFFFEull)
    return bad(SFMLOC_ECAP, "%llu feature rows (at most 2^32 - 2)", view_off[n_views]);
  if (view_off[n_views] && !kpt_xy) return bad(SFMLOC_EINVAL, "keypoints missing");
  for (uint32_t i = 0; i < n_intrinsics; ++i)
    if (intrinsic_type[i] != 0 && intrinsic_type[i] != 3)
      return bad(SFMLOC_EINVAL, "intrinsic %llu has type %llu (0 or 3)", i,
                  intrinsic_type[i]);
  if (n_pairs && (!pairs || !offsets)) return bad(SFMLOC_EINVAL, "pair arrays missing");
  if (n_pairs && offsets[0] != 0) return bad(SFMLOC_EINVAL, "offsets[0] must be 0");
  std::vector<uint32_t> lg;
  uint32_t lg_max = 0;
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    if (a >= n_views || b >= n_views)
      return bad(SFMLOC_EINVAL, "pair %llu = (%llu, %llu) out of range", k, a, b);
    if (a == b) return bad(SFMLOC_EINVAL, "pair %llu names view %llu twice", k, a);
    if (offsets[k] > offsets[k + 1])
      return bad(SFMLOC_EINVAL, "offsets not monotone at pair %llu", k);
    const uint64_t n = offsets[k + 1] - offsets[k];
    if (n > kLargeMaxM)
      return bad(SFMLOC_ECAP, "pair (%llu, %llu) has %llu matches (at most 65536)", a, b, n);
    if (n && (!match_i || !match_j)) return bad(SFMLOC_EINVAL, "match arrays missing");
    const uint64_t na = view_off[a + 1] - view_off[a], nb = view_off[b + 1] - view_off[b];
    for (uint64_t t = 0; t < n; ++t)
      if (match_i[offsets[k] + t] >= na || match_j[offsets[k] + t] >= nb)
        return bad(SFMLOC_EINVAL, "pair (%llu, %llu) match %llu out of range", a, b, t);
    if (n > kLdsMaxM) {
      lg.push_back(k);
      if ((uint32_t)n > lg_max) lg_max = (uint32_t)n;
    }
  }
  if (n_pairs && offsets[n_pairs] > 0xFFFFFFFEull)
    return bad(SFMLOC_ECAP, "%llu matches (at most 2^32 - 2)", offsets[n_pairs]);
  large->swap(lg);
  *large_max_m = lg_max;
  return SFMLOC_OK;
}

}  // namespace relpose_host
}  // namespace sfmloc
