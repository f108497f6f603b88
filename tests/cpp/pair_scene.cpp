// Host program over sfmlocalization_amd/csrc/pair_scene.h, the checks the four pair-side calls share: the walk over
// views and pairs under each caller's name and with each caller's switches, the checks of the poses and inlier lists,
// and the order of the refusals -- an input with two faults gets the text of the one that is looked for first.  No HIP,
// no GPU: meant to be built with -fsanitize=address,undefined and run on the CPU (tests/test_relpose_cpu.py does).
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/pairscales_host.h"
#include "../../sfmlocalization_amd/csrc/relpose_host.h"
#include "../../sfmlocalization_amd/csrc/relrefine_host.h"
#include "../../sfmlocalization_amd/csrc/tracks_host.h"

using namespace sfmloc;
using pair_host::check_poses;
using pair_host::walk;

static int g_fail = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                          \
    }                                                    \
  } while (0)

// the walker's switches as each entry point sets them
struct Caller {
  const char *name;
  bool need_intr, need_wh, cap_pairs;
};
static const Caller kRelpose{"sfmloc_relative_poses", true, true, true};
static const Caller kRefine{"sfmloc_refine_relative_poses", true, false, true};
static const Caller kWedges{"sfmloc_wedge_scales", true, false, true};
static const Caller kTracks{"sfmloc_tracks_build", false, false, false};
static const Caller kCallers[4] = {kRelpose, kRefine, kWedges, kTracks};

// four views of 3, 0, 4 and 2 features; the pairs (0, 2), (2, 3), (0, 3) with 2, 1 and 2 matches, the last of each an inlier
struct Case {
  std::vector<uint64_t> view_off{0, 3, 3, 7, 9};
  std::vector<float> kpt = std::vector<float>(18, 1.0f);
  std::vector<uint32_t> wh{640, 480, 640, 480, 640, 480, 640, 480};
  std::vector<uint32_t> vintr{0, 1, 0, 1};
  std::vector<double> intr{700, 320, 240, 0, 0, 0, 720, 318, 242, -0.1, 0.02, 0};
  std::vector<uint32_t> itype{0, 3};
  std::vector<uint32_t> pairs{0, 2, 2, 3, 0, 3};
  std::vector<uint64_t> offsets{0, 2, 3, 5};
  std::vector<uint32_t> mi{0, 2, 3, 1, 1}, mj{1, 3, 0, 0, 1};
  std::vector<double> R = std::vector<double>(27, 0.0), t = std::vector<double>(9, 0.0);
  std::vector<uint64_t> inl_off{0, 1, 2, 3};
  std::vector<uint32_t> inl{1, 0, 1};
  std::string err;
  Case() {
    for (size_t k = 0; k < 3; ++k) R[9 * k] = R[9 * k + 4] = R[9 * k + 8] = t[3 * k] = 1.0;
  }
  PairScene scene() const {
    return PairScene{view_off.data(), (uint32_t)view_off.size() - 1, kpt.data(),     wh.data(),
                     vintr.data(),    intr.data(),                   itype.data(),   (uint32_t)itype.size(),
                     pairs.data(),    (uint32_t)(pairs.size() / 2),  offsets.data(), mi.data(),
                     mj.data()};
  }
  PairPoses poses() const { return PairPoses{R.data(), t.data(), inl_off.data(), inl.data(), nullptr}; }
  int run(const Caller &c, const PairScene &sc) { return walk(c.name, sc, c.need_intr, c.need_wh, c.cap_pairs, &err); }
  int run(const Caller &c) { return run(c, scene()); }
  // the code, and the text is exactly the caller's name, ": " and `text`
  bool refused(const Caller &c, const PairScene &sc, int code, const std::string &text) {
    const int rc = run(c, sc);
    if (rc == code && err == std::string(c.name) + ": " + text) return true;
    printf("  got %d `%s`, wanted %d `%s: %s`\n", rc, err.c_str(), code, c.name, text.c_str());
    return false;
  }
  bool refused(const Caller &c, int code, const std::string &text) { return refused(c, scene(), code, text); }
  bool poses_refused(const PairPoses &po, int code, const std::string &text) {
    const int rc = check_poses(kWedges.name, scene(), po, &err);
    if (rc == code && err == std::string(kWedges.name) + ": " + text) return true;
    printf("  got %d `%s`, wanted %d `%s`\n", rc, err.c_str(), code, text.c_str());
    return false;
  }
};

// two views of one feature each and one pair of n matches
struct Long : Case {
  explicit Long(uint32_t n) {
    view_off = {0, 1, 2};
    kpt.assign(4, 1.0f);
    wh.resize(4);
    vintr = {0, 1};
    pairs = {1, 0};
    offsets = {0, n};
    mi.assign(n, 0);
    mj.assign(n, 0);
  }
};

int main() {
  for (const Caller &c : kCallers) {  // a good scene; every refusal of the walk that all four make, under the caller's name
    Case ok;
    EXPECT(ok.run(c) == SFMLOC_OK && ok.err.empty());
    Case a;
    a.pairs[3] = 4;
    EXPECT(a.refused(c, SFMLOC_EINVAL, "pair 1 = (2, 4) out of range"));
    Case b;
    b.pairs[1] = 0;
    EXPECT(b.refused(c, SFMLOC_EINVAL, "pair 0 names view 0 twice"));
    Case d;
    d.offsets = {0, 3, 2, 5};
    d.mi[2] = 0;  // (pair 0 now reaches to match 2: one of its views' features)
    EXPECT(d.refused(c, SFMLOC_EINVAL, "offsets not monotone at pair 1"));
    Case e;
    e.mj[2] = 2;
    EXPECT(e.refused(c, SFMLOC_EINVAL, "pair (2, 3) match 0 out of range"));
    Case f;
    f.view_off = {0, 3, 2, 7, 9};
    EXPECT(f.refused(c, SFMLOC_EINVAL, "view_off not monotone at 1"));
    Case g;
    g.view_off[0] = 1;
    EXPECT(g.refused(c, SFMLOC_EINVAL, "view_off[0] must be 0"));
    Case h;
    h.offsets[0] = 1;
    EXPECT(h.refused(c, SFMLOC_EINVAL, "offsets[0] must be 0"));
    Case i;
    i.view_off.back() = 0xFFFFFFFFull;
    EXPECT(i.refused(c, SFMLOC_ECAP, "4294967295 feature rows (at most 2^32 - 2)"));
    Case j;
    PairScene sc = j.scene();
    sc.n_views = 0;
    EXPECT(j.refused(c, sc, SFMLOC_EINVAL, "no views"));
    sc = j.scene();
    sc.offsets = nullptr;
    EXPECT(j.refused(c, sc, SFMLOC_EINVAL, "pair arrays missing"));
    sc = j.scene();
    sc.match_j = nullptr;
    EXPECT(j.refused(c, sc, SFMLOC_EINVAL, "match arrays missing"));
    sc = j.scene();
    sc.pairs = nullptr, sc.n_pairs = 0, sc.offsets = nullptr, sc.match_i = sc.match_j = nullptr;
    EXPECT(j.run(c, sc) == SFMLOC_OK);
  }
  {  // view_wh absent: a refusal where it is needed, nothing where it is not
    Case c;
    PairScene sc = c.scene();
    sc.view_wh = nullptr;
    EXPECT(c.refused(kRelpose, sc, SFMLOC_EINVAL, "view arrays missing"));
    EXPECT(c.run(kRefine, sc) == SFMLOC_OK && c.run(kWedges, sc) == SFMLOC_OK && c.run(kTracks, sc) == SFMLOC_OK);
  }
  {  // the cameras: looked at for the three two-view calls, not for the tracks (null arrays, or arrays that would be refused)
    Case c;
    PairScene sc = c.scene();
    sc.kpt_xy = nullptr, sc.view_wh = nullptr, sc.view_intrinsic = nullptr, sc.intrinsics = nullptr;
    sc.intrinsic_type = nullptr, sc.n_intrinsics = 0;
    EXPECT(c.run(kTracks, sc) == SFMLOC_OK);
    EXPECT(c.refused(kWedges, sc, SFMLOC_EINVAL, "view arrays missing"));
    sc.view_intrinsic = c.vintr.data();
    EXPECT(c.refused(kRefine, sc, SFMLOC_EINVAL, "no intrinsics"));
    sc = c.scene();
    sc.kpt_xy = nullptr;
    EXPECT(c.refused(kRelpose, sc, SFMLOC_EINVAL, "keypoints missing") && c.run(kTracks, sc) == SFMLOC_OK);
    Case d;
    d.vintr[2] = 2;
    EXPECT(d.refused(kRefine, SFMLOC_EINVAL, "view 2 names intrinsic 2 of 2") && d.run(kTracks) == SFMLOC_OK);
    Case e;
    e.itype[1] = 1;
    EXPECT(e.refused(kWedges, SFMLOC_EINVAL, "intrinsic 1 has type 1 (0 or 3)") && e.run(kTracks) == SFMLOC_OK);
  }
  {  // the cap on a pair's matches: 65 536 pass everywhere, 65 537 only where there is no cap
    Long at(65536), over(65537);
    for (const Caller &c : kCallers) {
      EXPECT(at.run(c) == SFMLOC_OK);
      if (c.cap_pairs) EXPECT(over.refused(c, SFMLOC_ECAP, "pair (1, 0) has 65537 matches (at most 65536)"));
      else EXPECT(over.run(c) == SFMLOC_OK);
    }
    // ... and it is looked for before the pair's matches are: a pair over the cap with a match out of range, and one
    // without its match arrays
    over.mi[7] = 1;
    EXPECT(over.refused(kRelpose, SFMLOC_ECAP, "pair (1, 0) has 65537 matches (at most 65536)"));
    EXPECT(over.refused(kTracks, SFMLOC_EINVAL, "pair (1, 0) match 7 out of range"));
    PairScene sc = over.scene();
    sc.match_i = nullptr;
    EXPECT(over.refused(kWedges, sc, SFMLOC_ECAP, "pair (1, 0) has 65537 matches (at most 65536)"));
    EXPECT(over.refused(kTracks, sc, SFMLOC_EINVAL, "match arrays missing"));
  }
  {  // two faults at once, neighbours in the order of the checks: the first one's text.  (The last check of a two-view
     // call, 2^32 - 2 matches in all, cannot be reached by arrays that exist: 65 536 pairs at the cap hold 16 GiB.)
    Case c;
    PairScene sc = c.scene();
    sc.n_views = 0, sc.view_intrinsic = nullptr;
    EXPECT(c.refused(kRelpose, sc, SFMLOC_EINVAL, "no views"));
    sc = c.scene();
    sc.view_wh = nullptr, sc.n_intrinsics = 0;
    EXPECT(c.refused(kRelpose, sc, SFMLOC_EINVAL, "view arrays missing"));
    c.view_off[0] = 1;
    sc = c.scene();
    sc.intrinsic_type = nullptr;
    EXPECT(c.refused(kRefine, sc, SFMLOC_EINVAL, "no intrinsics"));
    Case d;
    d.view_off = {1, 0, 3, 7, 9};
    EXPECT(d.refused(kTracks, SFMLOC_EINVAL, "view_off[0] must be 0"));
    Case e;  // (one view with both faults: its offsets first; an earlier view's intrinsic before a later view's offsets)
    e.view_off = {0, 3, 2, 7, 9};
    e.vintr[1] = 5;
    EXPECT(e.refused(kWedges, SFMLOC_EINVAL, "view_off not monotone at 1"));
    e.vintr = {5, 1, 0, 1};
    EXPECT(e.refused(kWedges, SFMLOC_EINVAL, "view 0 names intrinsic 5 of 2"));
    Case f;
    f.vintr[3] = 2;
    f.view_off.back() = 0xFFFFFFFFull;
    EXPECT(f.refused(kRelpose, SFMLOC_EINVAL, "view 3 names intrinsic 2 of 2"));
    Case g;
    g.view_off.back() = 0xFFFFFFFFull;
    sc = g.scene();
    sc.kpt_xy = nullptr;
    EXPECT(g.refused(kRelpose, sc, SFMLOC_ECAP, "4294967295 feature rows (at most 2^32 - 2)"));
    Case h;
    h.itype[0] = 7;
    sc = h.scene();
    sc.kpt_xy = nullptr;
    EXPECT(h.refused(kRefine, sc, SFMLOC_EINVAL, "keypoints missing"));
    sc = h.scene();
    sc.pairs = nullptr;
    EXPECT(h.refused(kRefine, sc, SFMLOC_EINVAL, "intrinsic 0 has type 7 (0 or 3)"));
    Case i;
    i.offsets[0] = 1;
    sc = i.scene();
    sc.pairs = nullptr;
    EXPECT(i.refused(kTracks, sc, SFMLOC_EINVAL, "pair arrays missing"));
    i.pairs[0] = 9;
    EXPECT(i.refused(kTracks, SFMLOC_EINVAL, "offsets[0] must be 0"));
    Case j;  // (inside one pair: range, twice, offsets, matches; and an earlier pair before a later one)
    j.pairs = {0, 9, 2, 3, 0, 3};
    j.offsets = {0, 4, 3, 5};
    EXPECT(j.refused(kRelpose, SFMLOC_EINVAL, "pair 0 = (0, 9) out of range"));
    j.pairs = {2, 2, 2, 3, 0, 3};
    EXPECT(j.refused(kRelpose, SFMLOC_EINVAL, "pair 0 names view 2 twice"));
    j.pairs = {0, 2, 2, 3, 0, 3};
    j.mi[0] = 3;
    EXPECT(j.refused(kRelpose, SFMLOC_EINVAL, "pair (0, 2) match 0 out of range"));
    Case k;
    k.mi[4] = 3;
    k.pairs[2] = 3;
    EXPECT(k.refused(kTracks, SFMLOC_EINVAL, "pair 1 names view 3 twice"));
  }
  {  // the poses and inlier lists: every refusal, and the first of two
    Case c;
    EXPECT(check_poses(kRefine.name, c.scene(), c.poses(), &c.err) == SFMLOC_OK);
    PairPoses po = c.poses();
    po.rel_t = nullptr;
    c.inl_off[0] = 1;
    EXPECT(c.poses_refused(po, SFMLOC_EINVAL, "pose or inlier arrays missing"));
    c.inl_off = {1, 0, 2, 3};
    EXPECT(c.poses_refused(c.poses(), SFMLOC_EINVAL, "inlier_off[0] must be 0"));
    Case d;
    d.inl_off = {0, 2, 1, 0x7FFFFC01ull};
    EXPECT(d.poses_refused(d.poses(), SFMLOC_EINVAL, "inlier_off not monotone at pair 1"));
    d.inl_off = {0, 0, 0, 0x7FFFFC01ull};  // (refused before the list behind it is asked for, or read)
    po = d.poses();
    po.inlier_idx = nullptr;
    EXPECT(d.poses_refused(po, SFMLOC_ECAP, "2147482625 inliers up to pair 2 (at most 2^31 - 1024)"));
    EXPECT(d.poses_refused(d.poses(), SFMLOC_ECAP, "2147482625 inliers up to pair 2 (at most 2^31 - 1024)"));
    Case e;
    e.R[4] = std::numeric_limits<double>::quiet_NaN();
    po = e.poses();
    po.inlier_idx = nullptr;
    EXPECT(e.poses_refused(po, SFMLOC_EINVAL, "inlier_idx missing"));
    e.inl[0] = 2;
    EXPECT(e.poses_refused(e.poses(), SFMLOC_EINVAL, "pair (0, 2) inlier 0 out of range"));
    e.inl[0] = 1, e.inl[1] = 1;
    EXPECT(e.poses_refused(e.poses(), SFMLOC_EINVAL, "pair (0, 2) has a non-finite rel_R or rel_t"));
    e.R[4] = 1.0;
    EXPECT(e.poses_refused(e.poses(), SFMLOC_EINVAL, "pair (2, 3) inlier 0 out of range"));
    PairScene none = e.scene();
    none.n_pairs = 0;
    EXPECT(check_poses(kWedges.name, none, PairPoses{}, &e.err) == SFMLOC_OK);
  }
  {  // the callers' own checks around the shared ones: the pair count first, the options between scene and poses
    Case c;
    c.mi[0] = 3;
    c.inl[0] = 2;
    sfmloc_relrefine_options ro{0, 13};
    PairScene many = c.scene();
    many.n_pairs = 0x40000000u;
    EXPECT(relrefine_host::check(many, c.poses(), ro, &c.err) == SFMLOC_ECAP && c.err.find("1073741824 pairs") != c.err.npos);
    EXPECT(relrefine_host::check(c.scene(), c.poses(), ro, &c.err) == SFMLOC_EINVAL &&
           c.err == "sfmloc_refine_relative_poses: pair (0, 2) match 0 out of range");
    c.mi[0] = 0;
    EXPECT(relrefine_host::check(c.scene(), c.poses(), ro, &c.err) == SFMLOC_EINVAL && c.err.find("max_steps = 0") != c.err.npos);
    ro.max_steps = 1;
    EXPECT(relrefine_host::check(c.scene(), c.poses(), ro, &c.err) == SFMLOC_EINVAL &&
           c.err == "sfmloc_refine_relative_poses: pair (0, 2) inlier 0 out of range");
    sfmloc_wscales_options wo{0, 2048};
    wscales_host::ViewPairs vp;
    EXPECT(wscales_host::check(many, c.poses(), wo, &vp, &c.err) == SFMLOC_ECAP && c.err.find("1073741824 pairs") != c.err.npos);
    EXPECT(wscales_host::check(c.scene(), c.poses(), wo, &vp, &c.err) == SFMLOC_EINVAL && c.err.find("min_shared = 0") != c.err.npos);
    wo.min_shared = 8;
    EXPECT(wscales_host::check(c.scene(), c.poses(), wo, &vp, &c.err) == SFMLOC_EINVAL &&
           c.err == "sfmloc_wedge_scales: pair (0, 2) inlier 0 out of range" && vp.off.empty());
    sfmloc_relpose_options po{(1u << 30) + 1, 0, 2.5, 1};
    c.mj[4] = 2;
    EXPECT(relpose_host::check(c.scene(), po, &c.err) == SFMLOC_EINVAL &&
           c.err == "sfmloc_relative_poses: pair (0, 3) match 1 out of range");
    c.mj[4] = 1;
    EXPECT(relpose_host::check(c.scene(), po, &c.err) == SFMLOC_EINVAL && c.err.find("max_iteration = 1073741825") != c.err.npos);
    po.max_iteration = 256, po.precision_px = -1.0;
    EXPECT(relpose_host::check(c.scene(), po, &c.err) == SFMLOC_EINVAL && c.err.find("precision_px must not be negative") != c.err.npos);
    po.precision_px = std::numeric_limits<double>::infinity();
    EXPECT(relpose_host::check(c.scene(), po, &c.err) == SFMLOC_OK);
    std::vector<uint32_t> ea, eb;
    uint64_t n_nodes = 0;
    const std::vector<uint8_t> use{1, 1, 1, 0};
    EXPECT(tracks_host::flatten(c.scene(), use.data(), &ea, &eb, &n_nodes, &c.err) == SFMLOC_OK && ea.size() == 2 && n_nodes == 9);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK pair_scene\n");
  return 0;
}
