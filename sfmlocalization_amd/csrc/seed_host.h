// The host side of sfmloc_seed_scores (seedpair.hip): every check the call makes before anything is launched -- the
// scene's and the poses' (pair_scene.h) under this call's name, and the options' own -- and the choice of the seed pair
// among the records (sfmloc.h "Seed scores", the last paragraph).  Host code only, no HIP: tests/cpp/seed_host.cpp runs
// it under the host sanitizers.
#pragma once

#include <math.h>
#include <stdint.h>

#include <string>

#include "../../include/sfmloc.h"
#include "pair_scene.h"

namespace sfmloc {
namespace seed_host {

constexpr uint32_t kMaxPairs = 0x3FFFFFFFu;  // as sfmloc_wedge_scales

// a threshold is a cosine in (-1, 1]
inline bool cosine_ok(double c) { return isfinite(c) && c > -1.0 && c <= 1.0; }

// sfmloc.h "Seed scores", refusals -> SFMLOC_OK, or the code with its text in *err
inline int check(const PairScene &sc, const PairPoses &po, const sfmloc_seed_options &opt, std::string *err) {
  static const char *const name = "sfmloc_seed_scores";
  using pair_host::fail;
  if (sc.n_pairs > kMaxPairs) return fail(err, SFMLOC_ECAP, "sfmloc_seed_scores: %llu pairs (at most 2^30 - 1)", sc.n_pairs);
  const int rc = pair_host::walk(name, sc, true, false, true, err);
  if (rc) return rc;
  if (opt.min_used == 0) return fail(err, SFMLOC_EINVAL, "sfmloc_seed_scores: min_used = 0 (at least 1)");
  if (!cosine_ok(opt.max_cos)) return fail(err, SFMLOC_EINVAL, "sfmloc_seed_scores: max_cos is not a cosine in (-1, 1]");
  if (!cosine_ok(opt.min_cos)) return fail(err, SFMLOC_EINVAL, "sfmloc_seed_scores: min_cos is not a cosine in (-1, 1]");
  if (opt.min_cos >= opt.max_cos)
    return fail(err, SFMLOC_EINVAL,
                "sfmloc_seed_scores: min_cos must be below max_cos (the larger angle has the smaller cosine)");
  return pair_host::check_poses(name, sc, po, err);
}

// The seed pair: among the candidates whose two views have different id_pose (view_pose [n_views]: a view's place in
// the pose table), the smallest cos_median (the largest median angle), then the larger n_used, then the smaller pair
// index -> the pair's index, or -1 when there is none
inline int64_t choose(const sfmloc_seed_score *scores, const uint32_t *pairs, uint32_t n_pairs, const uint32_t *view_pose) {
  int64_t best = -1;
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const sfmloc_seed_score &s = scores[k];
    if (!s.candidate || view_pose[pairs[2 * (size_t)k]] == view_pose[pairs[2 * (size_t)k + 1]]) continue;
    if (best < 0 || s.cos_median < scores[best].cos_median ||
        (s.cos_median == scores[best].cos_median && s.n_used > scores[best].n_used))
      best = k;
  }
  return best;
}

}  // namespace seed_host
}  // namespace sfmloc
