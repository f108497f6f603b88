// The host side of sfmloc_tracks_build (tracks.hip): every check the call makes before anything is launched (the walk
// over views and pairs is pair_scene.h's), and the flattening of the pair list (pairs, offsets, match_i, match_j: the
// layout of sfmloc_geometric_pairs) into one edge per match between global feature rows, node = view_off[view] +
// feature.  Host code only, no HIP: tests/cpp/tracks_host.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "pair_scene.h"

namespace sfmloc {
namespace tracks_host {

constexpr uint64_t kMaxEdges = 0xFFFFFFFEull;  // 2^32 - 2, as the node rows (pair_host::walk)

// sc: the views' offsets and the pair list, nothing of the cameras.  -> SFMLOC_OK and the edges (edge_a[e], edge_b[e])
// of every match of every pair whose two views are in use, in pair order; or the error code with its text in *err and
// the outputs untouched.  A pair with a masked-out view is checked like any other and contributes nothing.
inline int flatten(const PairScene &sc, const uint8_t *view_use, std::vector<uint32_t> *edge_a,
                   std::vector<uint32_t> *edge_b, uint64_t *n_nodes, std::string *err) {
  const int rc = pair_host::walk("sfmloc_tracks_build", sc, false, false, false, err);
  if (rc) return rc;
  const auto used = [&](uint32_t k) {
    return !view_use || (view_use[sc.pairs[2 * (size_t)k]] && view_use[sc.pairs[2 * (size_t)k + 1]]);
  };
  uint64_t n_edges = 0;
  for (uint32_t k = 0; k < sc.n_pairs; ++k)
    if (used(k)) n_edges += sc.offsets[k + 1] - sc.offsets[k];
  if (n_edges > kMaxEdges)
    return pair_host::fail(err, SFMLOC_ECAP, "sfmloc_tracks_build: %llu matches (at most 2^32 - 2)", n_edges);
  std::vector<uint32_t> ea, eb;
  ea.reserve(n_edges);
  eb.reserve(n_edges);
  for (uint32_t k = 0; k < sc.n_pairs; ++k) {
    if (!used(k)) continue;
    const uint64_t ra = sc.view_off[sc.pairs[2 * (size_t)k]], rb = sc.view_off[sc.pairs[2 * (size_t)k + 1]];
    for (uint64_t t = sc.offsets[k]; t < sc.offsets[k + 1]; ++t) {
      ea.push_back((uint32_t)(ra + sc.match_i[t]));
      eb.push_back((uint32_t)(rb + sc.match_j[t]));
    }
  }
  edge_a->swap(ea);
  edge_b->swap(eb);
  *n_nodes = sc.view_off[sc.n_views];
  return SFMLOC_OK;
}

}  // namespace tracks_host
}  // namespace sfmloc
