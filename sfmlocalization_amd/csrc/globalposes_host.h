// The host side of sfmloc_global_poses (globalposes.hip): every check the call makes before anything is launched, the
// adjacency the kernels gather over, and the choice of the component.  Host code only, no HIP:
// tests/cpp/globalposes_host.cpp runs it under the host sanitizers.
#pragma once

#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"

namespace sfmloc {
namespace gposes_host {

constexpr uint32_t kWaveDegree = 64;  // a view of more pairs than this is gathered by a wave, not by a lane
constexpr uint32_t kDirBit = 0x80000000u;  // in Adjacency::pe: the view is the pair's J

inline int fail(std::string *err, const char *fmt, unsigned long long a = 0, unsigned long long b = 0,
                unsigned long long c = 0, unsigned long long d = 0) {
  char buf[256];
  snprintf(buf, sizeof buf, fmt, a, b, c, d);
  *err = buf;
  return SFMLOC_EINVAL;
}

// sfmloc.h "adjacency": the entries of view v are off[v] .. off[v + 1], ascending by neighbour; pe = the pair's index,
// with kDirBit when v is the pair's J.  heavy = the views of more than kWaveDegree entries, ascending.
struct Adjacency {
  std::vector<uint32_t> off, nbr, pe, heavy;
};

// sfmloc.h "Refusals" -> SFMLOC_OK and the adjacency, or SFMLOC_EINVAL with its text in *err
inline int check(uint32_t n_views, const uint32_t *pairs, uint32_t n_pairs, const double *rel_R, const double *rel_t,
                 Adjacency *adj, std::string *err) {
  if (n_pairs && (!pairs || !rel_R || !rel_t)) return fail(err, "sfmloc_global_poses: pair arrays missing");
  if (n_pairs > 0x7FFFFFFFu) return fail(err, "sfmloc_global_poses: %llu pairs (at most 2^31 - 1)", n_pairs);
  std::vector<uint32_t> off((size_t)n_views + 1, 0);
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    if (a >= n_views || b >= n_views)
      return fail(err, "sfmloc_global_poses: pair %llu = (%llu, %llu) out of range", k, a, b);
    if (a == b) return fail(err, "sfmloc_global_poses: pair %llu names view %llu twice", k, a);
    const double *R = rel_R + 9 * (size_t)k, *t = rel_t + 3 * (size_t)k;
    for (int i = 0; i < 9; ++i)
      if (!isfinite(R[i])) return fail(err, "sfmloc_global_poses: pair %llu = (%llu, %llu) has a non-finite entry", k, a, b);
    for (int i = 0; i < 3; ++i)
      if (!isfinite(t[i])) return fail(err, "sfmloc_global_poses: pair %llu = (%llu, %llu) has a non-finite entry", k, a, b);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        const double g = (R[i] * R[j] + R[3 + i] * R[3 + j]) + R[6 + i] * R[6 + j];
        if (fabs(g - (i == j ? 1.0 : 0.0)) > 1e-6)
          return fail(err, "sfmloc_global_poses: pair %llu = (%llu, %llu): rel_R is not orthonormal", k, a, b);
      }
    if (fabs(sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]) - 1.0) > 1e-6)
      return fail(err, "sfmloc_global_poses: pair %llu = (%llu, %llu): rel_t is not of unit length", k, a, b);
    ++off[a + 1];
    ++off[b + 1];
  }
  for (uint32_t v = 0; v < n_views; ++v) off[v + 1] += off[v];
  struct Entry {
    uint32_t nbr, pe;
  };
  std::vector<Entry> ent(2 * (size_t)n_pairs);
  std::vector<uint32_t> at(off.begin(), off.end() - 1);
  for (uint32_t k = 0; k < n_pairs; ++k) {
    const uint32_t a = pairs[2 * (size_t)k], b = pairs[2 * (size_t)k + 1];
    ent[at[a]++] = Entry{b, k};
    ent[at[b]++] = Entry{a, k | kDirBit};
  }
  for (uint32_t v = 0; v < n_views; ++v) {
    std::sort(ent.begin() + off[v], ent.begin() + off[v + 1],
              [](const Entry &x, const Entry &y) { return x.nbr != y.nbr ? x.nbr < y.nbr : (x.pe & ~kDirBit) < (y.pe & ~kDirBit); });
    for (uint32_t e = off[v] + 1; e < off[v + 1]; ++e)
      if (ent[e].nbr == ent[e - 1].nbr)
        return fail(err, "sfmloc_global_poses: pair %llu lists the views (%llu, %llu) of pair %llu again", ent[e].pe & ~kDirBit,
                    std::min(v, ent[e].nbr), std::max(v, ent[e].nbr), ent[e - 1].pe & ~kDirBit);
  }
  adj->off.swap(off);
  adj->nbr.resize(ent.size());
  adj->pe.resize(ent.size());
  for (size_t e = 0; e < ent.size(); ++e) {
    adj->nbr[e] = ent[e].nbr;
    adj->pe[e] = ent[e].pe;
  }
  adj->heavy.clear();
  for (uint32_t v = 0; v < n_views; ++v)
    if (adj->off[v + 1] - adj->off[v] > kWaveDegree) adj->heavy.push_back(v);
  return SFMLOC_OK;
}

// sfmloc.h "component": label[v] = the smallest view of v's component -> the winner's label and size (size < 2: none)
inline void pick_component(const std::vector<uint32_t> &label, uint32_t *root, uint32_t *size) {
  std::vector<uint32_t> count(label.size(), 0);
  for (uint32_t l : label) ++count[l];
  *root = 0;
  *size = 0;
  for (uint32_t v = 0; v < (uint32_t)label.size(); ++v)
    if (count[v] > *size) {  // (ascending v: the smallest label wins a tie)
      *size = count[v];
      *root = v;
    }
}

}  // namespace gposes_host
}  // namespace sfmloc
