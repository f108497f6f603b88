// The host side of sfmloc_relative_poses (relpose.hip): every check the call makes before anything is launched (the
// scene's are pair_scene.h's, the options' are here), and the split of the pair list into the pairs the LDS form takes and
// the ones that need a global-memory slot.  Host code only, no HIP: tests/cpp/relpose_host.cpp runs it under the host
// sanitizers.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "pair_scene.h"

namespace sfmloc {
namespace relpose_host {

constexpr uint32_t kLdsMaxM = 2048;     // matches per pair the LDS form holds (forms.h kFMaxM)
constexpr uint32_t kLargeMaxM = 65536;  // matches per pair a global-memory slot holds (K3's kFLargeMaxM)
static_assert(kLargeMaxM == pair_host::kPairMaxM, "a slot holds every pair the scene's check lets through");

// sfmloc.h "Relative poses", refusals -> SFMLOC_OK, or the code with its text in *err
inline int check(const PairScene &sc, const sfmloc_relpose_options &opt, std::string *err) {
  const int rc = pair_host::walk("sfmloc_relative_poses", sc, true, true, true, err);
  if (rc) return rc;
  if (opt.max_iteration > (1u << 30))
    return pair_host::fail(err, SFMLOC_EINVAL, "sfmloc_relative_poses: max_iteration = %llu", opt.max_iteration);
  if (opt.precision_px < 0.0 || opt.precision_px != opt.precision_px)
    return pair_host::fail(err, SFMLOC_EINVAL, "sfmloc_relative_poses: precision_px must not be negative");
  return SFMLOC_OK;
}

// the pairs of a checked scene with more than kLdsMaxM matches in *large (pair order), the longest of them in *large_max_m
inline void split_large(const PairScene &sc, std::vector<uint32_t> *large, uint32_t *large_max_m) {
  large->clear();
  *large_max_m = 0;
  for (uint32_t k = 0; k < sc.n_pairs; ++k) {
    const uint64_t n = sc.offsets[k + 1] - sc.offsets[k];
    if (n <= kLdsMaxM) continue;
    large->push_back(k);
    if ((uint32_t)n > *large_max_m) *large_max_m = (uint32_t)n;
  }
}

}  // namespace relpose_host
}  // namespace sfmloc
