// The host side of sfmloc_refine_relative_poses (relrefine.hip): every check the call makes before anything is
// launched -- the scene's and the poses' (pair_scene.h) under this call's name, and the options' own.  Host code only, no
// HIP: tests/cpp/relrefine_host.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>

#include <string>

#include "../../include/sfmloc.h"
#include "pair_scene.h"

namespace sfmloc {
namespace relrefine_host {

constexpr uint32_t kMinPointsFloor = 6;     // five pose parameters: fewer points than six leave the reduced system short
constexpr uint32_t kMaxPairs = 0x3FFFFFFFu;  // as sfmloc_wedge_scales

// sfmloc.h "Two-view refinement", refusals -> SFMLOC_OK, or the code with its text in *err
inline int check(const PairScene &sc, const PairPoses &po, const sfmloc_relrefine_options &opt, std::string *err) {
  static const char *const name = "sfmloc_refine_relative_poses";
  using pair_host::fail;
  if (sc.n_pairs > kMaxPairs)
    return fail(err, SFMLOC_ECAP, "sfmloc_refine_relative_poses: %llu pairs (at most 2^30 - 1)", sc.n_pairs);
  const int rc = pair_host::walk(name, sc, true, false, true, err);
  if (rc) return rc;
  if (opt.max_steps == 0) return fail(err, SFMLOC_EINVAL, "sfmloc_refine_relative_poses: max_steps = 0 (at least 1)");
  if (opt.min_points < kMinPointsFloor)
    return fail(err, SFMLOC_EINVAL, "sfmloc_refine_relative_poses: min_points = %llu (at least 6)", opt.min_points);
  return pair_host::check_poses(name, sc, po, err);
}

}  // namespace relrefine_host
}  // namespace sfmloc
