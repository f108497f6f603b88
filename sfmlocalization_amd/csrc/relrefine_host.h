// The host side of sfmloc_refine_relative_poses (relrefine.hip): every check the call makes before anything is
// launched -- those of sfmloc_relative_poses on the view and pair arrays (relpose_host.h), those of sfmloc_wedge_scales
// on the poses and inlier lists (pairscales_host.h), and the options' own.  Host code only, no HIP:
// tests/cpp/relrefine_host.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "pairscales_host.h"
#include "relpose_host.h"

namespace sfmloc {
namespace relrefine_host {

constexpr uint32_t kMinPointsFloor = 6;     // five pose parameters: fewer points than six leave the reduced system short
constexpr uint32_t kMaxPairs = 0x3FFFFFFFu;  // as sfmloc_wedge_scales

// sfmloc.h "Two-view refinement", refusals -> SFMLOC_OK, or the code with its text in *err
inline int check(const uint64_t *view_off, uint32_t n_views, const float *kpt_xy, const uint32_t *view_intrinsic,
                 const double *intrinsics, const uint32_t *intrinsic_type, uint32_t n_intrinsics, const uint32_t *pairs,
                 uint32_t n_pairs, const uint64_t *offsets, const uint32_t *match_i, const uint32_t *match_j,
                 const double *rel_R, const double *rel_t, const uint64_t *inlier_off, const uint32_t *inlier_idx,
                 const sfmloc_relrefine_options &opt, std::string *err) {
  static const char *const name = "sfmloc_refine_relative_poses";
  if (n_pairs > kMaxPairs)
    return relpose_host::fail(err, SFMLOC_ECAP, "sfmloc_refine_relative_poses: %llu pairs (at most 2^30 - 1)", n_pairs);
  std::vector<uint32_t> large;
  uint32_t large_max_m = 0;
  int rc = relpose_host::check(view_off, n_views, kpt_xy, nullptr, view_intrinsic, intrinsics, intrinsic_type, n_intrinsics,
                               pairs, n_pairs, offsets, match_i, match_j, &large, &large_max_m, err, name, false);
  if (rc) return rc;
  if (opt.max_steps == 0)
    return relpose_host::fail(err, SFMLOC_EINVAL, "sfmloc_refine_relative_poses: max_steps = 0 (at least 1)");
  if (opt.min_points < kMinPointsFloor)
    return relpose_host::fail(err, SFMLOC_EINVAL, "sfmloc_refine_relative_poses: min_points = %llu (at least 6)",
                              opt.min_points);
  return wscales_host::check_inliers(name, pairs, n_pairs, offsets, rel_R, rel_t, inlier_off, inlier_idx, err);
}

}  // namespace relrefine_host
}  // namespace sfmloc
