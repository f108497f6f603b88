// Host program over sfmlocalization_amd/csrc/seed_host.h and pair_scene.h, the host side of sfmloc_seed_scores: every
// refusal with its code and text -- those of the relative poses and of the wedge scales under this call's name, and the
// options' own -- and the choice of the seed pair.  No HIP, no GPU: meant to be built with
// -fsanitize=address,undefined and run on the CPU (tests/test_seedpair_cpu.py does).
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/seed_host.h"

using namespace sfmloc::seed_host;
using sfmloc::PairPoses;
using sfmloc::PairScene;

static int g_fail = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                          \
    }                                                    \
  } while (0)

// five views of four features each; the pairs (3, 1), (0, 1), (1, 2), (4, 0) with two matches each, the second an inlier
struct Case {
  uint32_t n_views = 5;
  std::vector<uint64_t> view_off{0, 4, 8, 12, 16, 20};
  std::vector<float> kpt = std::vector<float>(40, 1.f);
  std::vector<uint32_t> view_intr{0, 0, 0, 0, 0}, itype{0};
  std::vector<double> intr{100, 50, 50, 0, 0, 0};
  std::vector<uint32_t> pairs{3, 1, 0, 1, 1, 2, 4, 0};
  std::vector<uint64_t> offsets, inl_off;
  std::vector<uint32_t> mi, mj, inl;
  std::vector<double> R, t;
  sfmloc_seed_options opt{100, 0, 0.9986295347545738, 0.5};
  std::string err;
  Case() {
    const size_t P = pairs.size() / 2;
    offsets.assign(1, 0);
    inl_off.assign(1, 0);
    for (size_t k = 0; k < P; ++k) {
      mi.insert(mi.end(), {0, 3});
      mj.insert(mj.end(), {1, 2});
      offsets.push_back(mi.size());
      inl.push_back(1);
      inl_off.push_back(inl.size());
    }
    R.assign(9 * P, 0.0);
    t.assign(3 * P, 0.0);
    for (size_t k = 0; k < P; ++k) R[9 * k] = R[9 * k + 4] = R[9 * k + 8] = t[3 * k] = 1.0;
  }
  PairScene scene() const {
    return PairScene{view_off.data(), n_views,      kpt.data(), nullptr,
                     view_intr.data(), intr.data(), itype.data(), 1,
                     pairs.data(),    (uint32_t)(pairs.size() / 2), offsets.data(), mi.data(),
                     mj.data()};
  }
  PairPoses poses() const { return PairPoses{R.data(), t.data(), inl_off.data(), inl.data(), nullptr}; }
  int run(const PairScene &sc, const PairPoses &po) { return check(sc, po, opt, &err); }
  int run() { return run(scene(), poses()); }
  bool refused(int code, const char *text) {
    const int rc = run();
    if (rc != code || err.find(text) == std::string::npos) {
      printf("  got %d `%s`, wanted %d `%s`\n", rc, err.c_str(), code, text);
      return false;
    }
    return true;
  }
};

static sfmloc_seed_score score(uint32_t n_used, uint32_t candidate, double c) {
  return sfmloc_seed_score{n_used, n_used, candidate, 0, c};
}

int main() {
  {  // a good call; thresholds at the ends of their range; no pairs at all
    Case c;
    EXPECT(c.run() == SFMLOC_OK && c.err.empty());
    c.opt.min_used = 1;
    c.opt.max_cos = 1.0;
    c.opt.min_cos = -0.9999999999999999;
    EXPECT(c.run() == SFMLOC_OK);
    PairScene sc = c.scene();
    sc.pairs = nullptr, sc.n_pairs = 0, sc.offsets = nullptr, sc.match_i = sc.match_j = nullptr;
    EXPECT(c.run(sc, PairPoses{}) == SFMLOC_OK);
  }
  {  // the checks of the relative poses, under this call's name
    Case c;
    c.pairs[5] = 5;
    EXPECT(c.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: pair 2 = (1, 5) out of range"));
    Case d;
    d.pairs[2] = 1;
    EXPECT(d.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: pair 1 names view 1 twice"));
    Case e;
    e.mj[3] = 4;
    EXPECT(e.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: pair (0, 1) match 1 out of range"));
    Case f;
    f.itype[0] = 2;
    EXPECT(f.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: intrinsic 0 has type 2"));
    Case g;
    g.view_intr[4] = 1;
    EXPECT(g.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: view 4 names intrinsic 1 of 1"));
    Case h;
    h.view_off[0] = 1;
    EXPECT(h.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: view_off[0] must be 0"));
    Case i;
    i.offsets[2] = 1;
    EXPECT(i.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: offsets not monotone at pair 1"));
    Case j;
    PairScene many = j.scene();
    many.n_pairs = 0x40000000u;
    EXPECT(j.run(many, j.poses()) == SFMLOC_ECAP && j.err.find("1073741824 pairs") != std::string::npos);
  }
  {  // those of the wedge scales: an inlier position out of its pair's range; offsets that go back; a missing array
    Case c;
    c.inl[2] = 2;
    EXPECT(c.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: pair (1, 2) inlier 0 out of range"));
    Case d;
    d.inl_off = {0, 1, 3, 2, 4};
    EXPECT(d.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: inlier_off not monotone at pair 2"));
    Case e;
    e.inl_off[0] = 1;
    EXPECT(e.refused(SFMLOC_EINVAL, "inlier_off[0] must be 0"));
    Case f;
    PairPoses no_t = f.poses(), no_idx = f.poses();
    no_t.rel_t = nullptr;
    no_idx.inlier_idx = nullptr;
    EXPECT(f.run(f.scene(), no_t) == SFMLOC_EINVAL && f.err.find("pose or inlier arrays missing") != std::string::npos);
    EXPECT(f.run(f.scene(), no_idx) == SFMLOC_EINVAL && f.err.find("inlier_idx missing") != std::string::npos);
    Case g;
    g.inl_off = {0, 1, 2, 3, 0x7FFFFC01ull};  // (refused before the list behind it is read)
    EXPECT(g.refused(SFMLOC_ECAP, "2147482625 inliers up to pair 3"));
  }
  {  // a non-finite rotation or translation
    Case c;
    c.R[9 + 4] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(c.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: pair (0, 1) has a non-finite rel_R or rel_t"));
    Case d;
    d.t[3 * 3 + 2] = std::numeric_limits<double>::infinity();
    EXPECT(d.refused(SFMLOC_EINVAL, "pair (4, 0) has a non-finite rel_R or rel_t"));
  }
  {  // the options
    Case c;
    c.opt.min_used = 0;
    EXPECT(c.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: min_used = 0"));
    const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
    for (double x : {nan, inf, -inf, -1.0, 1.0000000000000002, -2.0}) {
      Case d, e;
      d.opt.max_cos = x;
      EXPECT(d.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: max_cos is not a cosine in (-1, 1]"));
      e.opt.min_cos = x;
      EXPECT(e.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: min_cos is not a cosine in (-1, 1]"));
    }
    Case f;
    f.opt.min_cos = f.opt.max_cos;
    EXPECT(f.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: min_cos must be below max_cos"));
    Case g;
    g.opt.min_cos = 0.9999;
    EXPECT(g.refused(SFMLOC_EINVAL, "sfmloc_seed_scores: min_cos must be below max_cos"));
  }
  {  // the choice: the smallest cosine among the candidates; ties by n_used, then by index; a shared id_pose; none
    const uint32_t pairs[] = {0, 1, 1, 2, 2, 3, 0, 3, 0, 2};
    const uint32_t own[] = {0, 1, 2, 3}, rig[] = {0, 1, 2, 2};
    std::vector<sfmloc_seed_score> s{score(150, 1, 0.98), score(120, 1, 0.97), score(400, 0, 0.2), score(130, 1, 0.97),
                                     score(130, 1, 0.97)};
    EXPECT(choose(s.data(), pairs, 5, own) == 3);   // 0.97 three times: 130 beats 120, pair 3 comes before pair 4
    s[3].n_used = 120;
    EXPECT(choose(s.data(), pairs, 5, own) == 4);
    s[4].n_used = 120;
    EXPECT(choose(s.data(), pairs, 5, own) == 1);
    s[2] = score(100, 1, 0.6);
    EXPECT(choose(s.data(), pairs, 5, own) == 2);
    EXPECT(choose(s.data(), pairs, 5, rig) == 1);   // (2, 3) share a pose: skipped
    for (sfmloc_seed_score &x : s) x.candidate = 0;
    EXPECT(choose(s.data(), pairs, 5, own) == -1);
    EXPECT(choose(s.data(), pairs, 0, own) == -1);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK seed_host\n");
  return 0;
}
