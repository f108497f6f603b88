// The host side of sfmloc_tracks_build (tracks.hip): every check the call makes before anything is launched, and the
// flattening of the pair list (pairs, offsets, match_i, match_j: the layout of sfmloc_geometric_pairs) into one edge per
// match between global feature rows, node = view_off[view] + feature.  Host code only, no HIP: tests/cpp/tracks_host.cpp
// runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/sfmloc.h"

namespace sfmloc {
namespace tracks_host {

constexpr uint64_t kMaxNodes = 0xFFFFFFFEull;  // 2^32 - 2: a node row and a count of rows both fit uint32_t
constexpr uint64_t kMaxEdges = 0xFFFFFFFEull;

inline int fail(std::string *err, int code, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                unsigned long long c = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c);
  *err = buf;
  return code;
}

// -> SFMLOC_OK and the edges (edge_a[e], edge_b[e]) of every match of every pair whose two views are in use, in pair
// order; or the error code with its text in *err and the outputs untouched.  A pair with a masked-out view is checked
// like any other and contributes nothing.
inline int flatten(const uint64_t *view_off, uint32_t n_views, const uint8_t *view_use, const uint32_t *pairs,
                   uint32_t n_pairs, const uint64_t *offsets, const uint32_t *match_i, const uint32_t *match_j,
                   std::vector<uint32_t> *edge_a, std::vector<uint32_t> *edge_b, uint64_t *n_nodes, std::string *err) {
  if (!view_off || n_views == 0) return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: no views");
  if (view_off[0] != 0) return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: view_off[0] must be 0");
  for (uint32_t v = 0; v < n_views; ++v)
    if (view_off[v] > view_off[v + 1])
      return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: view_off not monotone at %llu", v);
  if (view_off[n_views] > kMaxNodes)
    return fail(err, SFMLOC_ECAP, "sfmloc_tracks_build: %llu feature rows (at most 2^32 - 2)", view_off[n_views]);
  if (n_pairs && (!pairs || !offsets))
    return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: pair arrays missing");
  if (n_pairs && offsets[0] != 0) return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: offsets[0] must be 0");
  uint64_t n_edges = 0;
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    if (a >= n_views || b >= n_views)
      return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: pair %llu = (%llu, %llu) out of range", k, a, b);
    if (a == b) return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: pair %llu names view %llu twice", k, a);
    if (offsets[k] > offsets[k + 1])
      return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: offsets not monotone at pair %llu", k);
    const uint64_t n = offsets[k + 1] - offsets[k];
    if (n && (!match_i || !match_j)) return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: match arrays missing");
    const uint64_t na = view_off[a + 1] - view_off[a], nb = view_off[b + 1] - view_off[b];
    for (uint64_t t = 0; t < n; ++t)
      if (match_i[offsets[k] + t] >= na || match_j[offsets[k] + t] >= nb)
        return fail(err, SFMLOC_EINVAL, "sfmloc_tracks_build: pair (%llu, %llu) match %llu out of range", a, b, t);
    if (!view_use || (view_use[a] && view_use[b])) n_edges += n;
  }
  if (n_edges > kMaxEdges)
    return fail(err, SFMLOC_ECAP, "sfmloc_tracks_build: %llu matches (at most 2^32 - 2)", n_edges);
  std::vector<uint32_t> ea, eb;
  ea.reserve(n_edges);
  eb.reserve(n_edges);
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    if (view_use && !(view_use[a] && view_use[b])) continue;
    for (uint64_t t = offsets[k]; t < offsets[k + 1]; ++t) {
      ea.push_back((uint32_t)(view_off[a] + match_i[t]));
      eb.push_back((uint32_t)(view_off[b] + match_j[t]));
    }
  }
  edge_a->swap(ea);
  edge_b->swap(eb);
  *n_nodes = view_off[n_views];
  return SFMLOC_OK;
}

}  // namespace tracks_host
}  // namespace sfmloc
