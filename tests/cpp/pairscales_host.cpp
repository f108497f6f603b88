// Host program over sfmlocalization_amd/csrc/pairscales_host.h, the host side of sfmloc_wedge_scales: every refusal with
// its code and text, and the per-view lists of pairs the kernels enumerate candidates from; and of
// sfmloc_global_poses_scaled: the refusals of its wedge list and the adjacency of the scale graph.  No HIP, no GPU: meant to be
// built with -fsanitize=address,undefined and run on the CPU (tests/test_pairscales_cpu.py does).
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/pairscales_host.h"

using namespace sfmloc::wscales_host;
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
  std::vector<uint8_t> use;
  sfmloc_wscales_options opt{8, 2048};
  ViewPairs vp;
  std::string err;
  Case() { fill(); }
  void fill() {
    const size_t P = pairs.size() / 2;
    offsets.assign(1, 0);
    inl_off.assign(1, 0);
    mi.clear(), mj.clear(), inl.clear();
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
  PairPoses poses() const {
    return PairPoses{R.data(), t.data(), inl_off.data(), inl.data(), use.empty() ? nullptr : use.data()};
  }
  int run(const PairScene &sc, const PairPoses &po) { return check(sc, po, opt, &vp, &err); }
  int run() { return run(scene(), poses()); }
  bool untouched() const { return vp.off.empty() && vp.ent.empty() && vp.cand.empty(); }
  bool refused(int code, const char *text) {
    const int rc = run();
    if (rc != code || !untouched() || err.find(text) == std::string::npos) {
      printf("  got %d `%s`, wanted %d `%s`\n", rc, err.c_str(), code, text);
      return false;
    }
    return true;
  }
};

int main() {
  {  // a good call: every view's pairs ascend by pair index and mark the pair's J; the candidates before each view
    Case c;
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT((c.vp.off == std::vector<uint32_t>{0, 2, 5, 6, 7, 8}));
    EXPECT((c.vp.ent == std::vector<uint32_t>{1, 3 | kSideBit, 0 | kSideBit, 1 | kSideBit, 2, 2 | kSideBit, 0, 3}));
    EXPECT((c.vp.cand == std::vector<uint32_t>{0, 1, 4, 4, 4, 4}));
    EXPECT(c.vp.heavy.empty() && c.vp.n_used == 4 && c.vp.n_inliers == 4);
  }
  {  // a pair left out takes its entries, its candidates and its inliers with it
    Case c;
    c.use = {1, 0, 1, 1};
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT((c.vp.off == std::vector<uint32_t>{0, 1, 3, 4, 5, 6}));
    EXPECT((c.vp.ent == std::vector<uint32_t>{3 | kSideBit, 0 | kSideBit, 2, 2 | kSideBit, 0, 3}));
    EXPECT((c.vp.cand == std::vector<uint32_t>{0, 0, 1, 1, 1, 1}) && c.vp.n_used == 3 && c.vp.n_inliers == 3);
  }
  {  // no pairs at all
    Case c;
    PairScene sc = c.scene();
    sc.pairs = nullptr, sc.n_pairs = 0, sc.offsets = nullptr, sc.match_i = sc.match_j = nullptr;
    EXPECT(c.run(sc, PairPoses{}) == SFMLOC_OK);
    EXPECT((c.vp.off == std::vector<uint32_t>(6, 0)) && c.vp.ent.empty() && c.vp.cand.back() == 0 && c.vp.n_used == 0);
  }
  {  // the checks of the relative poses, under this call's name
    Case c;
    c.pairs[5] = 5;
    EXPECT(c.refused(SFMLOC_EINVAL, "sfmloc_wedge_scales: pair 2 = (1, 5) out of range"));
    Case d;
    d.pairs[2] = 1;
    EXPECT(d.refused(SFMLOC_EINVAL, "sfmloc_wedge_scales: pair 1 names view 1 twice"));
    Case e;
    e.mj[3] = 4;
    EXPECT(e.refused(SFMLOC_EINVAL, "sfmloc_wedge_scales: pair (0, 1) match 1 out of range"));
    Case f;
    f.itype[0] = 2;
    EXPECT(f.refused(SFMLOC_EINVAL, "sfmloc_wedge_scales: intrinsic 0 has type 2"));
    Case g;
    g.view_intr[4] = 1;
    EXPECT(g.refused(SFMLOC_EINVAL, "sfmloc_wedge_scales: view 4 names intrinsic 1 of 1"));
  }
  {  // an inlier position out of its pair's range; offsets that go back; a missing array
    Case c;
    c.inl[2] = 2;
    EXPECT(c.refused(SFMLOC_EINVAL, "pair (1, 2) inlier 0 out of range"));
    Case d;
    d.inl_off = {0, 1, 3, 2, 4};
    EXPECT(d.refused(SFMLOC_EINVAL, "inlier_off not monotone at pair 2"));
    Case e;
    e.inl_off[0] = 1;
    EXPECT(e.refused(SFMLOC_EINVAL, "inlier_off[0] must be 0"));
    Case f;
    PairPoses no_t = f.poses(), no_idx = f.poses();
    no_t.rel_t = nullptr;
    no_idx.inlier_idx = nullptr;
    EXPECT(f.run(f.scene(), no_t) == SFMLOC_EINVAL && f.untouched());
    EXPECT(f.run(f.scene(), no_idx) == SFMLOC_EINVAL && f.err.find("inlier_idx missing") != std::string::npos);
  }
  {  // a non-finite rotation or translation, also of a pair that is left out
    Case c;
    c.R[9 + 4] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(c.refused(SFMLOC_EINVAL, "pair (0, 1) has a non-finite rel_R or rel_t"));
    Case d;
    d.t[3 * 3 + 2] = std::numeric_limits<double>::infinity();
    d.use = {1, 1, 1, 0};
    EXPECT(d.refused(SFMLOC_EINVAL, "pair (4, 0) has a non-finite rel_R or rel_t"));
  }
  {  // the options
    Case c;
    c.opt.min_shared = 0;
    EXPECT(c.refused(SFMLOC_EINVAL, "min_shared = 0"));
    for (uint32_t m : {0u, kMaxShared + 1}) {
      Case d;
      d.opt.max_shared = m;
      EXPECT(d.refused(SFMLOC_EINVAL, "max_shared = "));
    }
    Case e;
    e.opt.min_shared = 5000;  // (more than a wedge can have: no error, no record)
    e.opt.max_shared = 1;
    EXPECT(e.run() == SFMLOC_OK);
  }
  {  // a view of kWaveDegree pairs is a lane's, one more makes it a wave's; d (d - 1) / 2 candidates
    for (uint32_t deg : {kWaveDegree, kWaveDegree + 1}) {
      Case c;
      c.n_views = deg + 1;
      c.view_off.resize(deg + 2);
      for (uint32_t v = 0; v <= deg + 1; ++v) c.view_off[v] = 4 * v;
      c.kpt.assign(8 * (deg + 1), 1.f);
      c.view_intr.assign(deg + 1, 0);
      c.pairs.clear();
      for (uint32_t v = 1; v <= deg; ++v) {
        c.pairs.push_back(v % 2 ? 0 : v);
        c.pairs.push_back(v % 2 ? v : 0);
      }
      c.fill();
      EXPECT(c.run() == SFMLOC_OK);
      EXPECT(c.vp.off[1] == deg && c.vp.off[deg + 1] == 2 * deg && c.vp.cand[1] == deg * (deg - 1) / 2);
      EXPECT(c.vp.cand[deg + 1] == deg * (deg - 1) / 2);
      for (uint32_t e = 0; e < deg; ++e) EXPECT(c.vp.ent[e] == (e | ((e + 1) % 2 ? 0u : kSideBit)));
      EXPECT(c.vp.heavy == (deg > kWaveDegree ? std::vector<uint32_t>{0} : std::vector<uint32_t>{}));
    }
  }
  {  // sfmloc_global_poses_scaled: the refusals of the wedge list, each naming the wedge's pairs
    const std::vector<uint32_t> pairs{3, 1, 0, 1, 1, 2, 4, 0};  // pair 3 = (4, 0) shares a view with pair 1 = (0, 1) only
    std::string err;
    auto run = [&](std::vector<uint32_t> kl, std::vector<double> q) {
      err.clear();
      return check_wedges(pairs.data(), 4, kl.data(), q.data(), (uint32_t)q.size(), &err);
    };
    EXPECT(run({0, 1, 0, 2, 1, 2, 1, 3}, {1.0, 2.0, 0.5, 3.0}) == SFMLOC_OK && err.empty());
    EXPECT(run({}, {}) == SFMLOC_OK);
    EXPECT(check_wedges(pairs.data(), 4, nullptr, nullptr, 0, &err) == SFMLOC_OK);
    EXPECT(check_wedges(pairs.data(), 4, nullptr, nullptr, 1, &err) == SFMLOC_EINVAL && err.find("wedge arrays missing") != err.npos);
    EXPECT(run({0, 4}, {1.0}) == SFMLOC_EINVAL && err.find("wedge 0 = pairs (0, 4) out of range") != err.npos);
    EXPECT(run({0, 1, 2, 1}, {1.0, 1.0}) == SFMLOC_EINVAL && err.find("wedge 1 = pairs (2, 1): k must be below l") != err.npos);
    EXPECT(run({1, 1}, {1.0}) == SFMLOC_EINVAL && err.find("k must be below l") != err.npos);
    EXPECT(run({0, 3}, {1.0}) == SFMLOC_EINVAL && err.find("wedge 0 = pairs (0, 3) share no view") != err.npos);
    EXPECT(run({0, 1, 1, 2, 0, 1}, {1.0, 1.0, 2.0}) == SFMLOC_EINVAL && err.find("pairs (0, 1) is listed twice") != err.npos);
  }
  {  // the adjacency of the scale graph: ascending by neighbour, the side bit at the wedge's l, wedges that are off left out
    const std::vector<uint32_t> kl{1, 3, 0, 3, 0, 1, 2, 3, 0, 2};
    const std::vector<uint8_t> on{1, 1, 1, 0, 1};
    ScaleGraph g;
    scale_adjacency(5, kl.data(), on.data(), 5, &g);
    EXPECT((g.off == std::vector<uint32_t>{0, 3, 5, 6, 8, 8}));
    EXPECT((g.nbr == std::vector<uint32_t>{1, 2, 3, 0, 3, 0, 0, 1}));
    EXPECT((g.pe == std::vector<uint32_t>{2, 4, 1, 2 | kSideBit, 0, 4 | kSideBit, 1 | kSideBit, 0 | kSideBit}));
    EXPECT(g.heavy.empty());
    scale_adjacency(5, kl.data(), std::vector<uint8_t>(5, 0).data(), 5, &g);
    EXPECT(g.off == std::vector<uint32_t>(6, 0) && g.nbr.empty() && g.pe.empty());
    scale_adjacency(0, nullptr, nullptr, 0, &g);
    EXPECT(g.off == std::vector<uint32_t>(1, 0) && g.nbr.empty());
    for (uint32_t deg : {kWaveDegree, kWaveDegree + 1}) {  // a star: node 0 of deg wedges is a lane's, of one more a wave's
      std::vector<uint32_t> star;
      for (uint32_t v = deg; v >= 1; --v) star.insert(star.end(), {0u, v});
      scale_adjacency(deg + 1, star.data(), std::vector<uint8_t>(deg, 1).data(), deg, &g);
      EXPECT(g.off[1] == deg && g.off[deg + 1] == 2 * deg);
      for (uint32_t e = 0; e < deg; ++e) EXPECT(g.nbr[e] == e + 1 && g.pe[e] == deg - 1 - e);
      EXPECT(g.heavy == (deg > kWaveDegree ? std::vector<uint32_t>{0} : std::vector<uint32_t>{}));
    }
    EXPECT(lower_median({3.0, 1.0, 2.0, 4.0}) == 2.0 && lower_median({5.0, 1.0, 3.0}) == 3.0 && lower_median({7.0}) == 7.0);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK pairscales_host\n");
  return 0;
}
