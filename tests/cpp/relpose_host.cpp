// Host program over sfmlocalization_amd/csrc/relpose_host.h, the host side of sfmloc_relative_poses: every refusal with
// its code and text (the scene's are pair_scene.h's, under this call's name), and the split of the pair list into the LDS
// form's pairs and the large ones.  No HIP, no GPU: meant
// to be built with -fsanitize=address,undefined and run on the CPU (tests/test_relpose_cpu.py does).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/relpose_host.h"

using sfmloc::PairScene;
using sfmloc::relpose_host::check;
using sfmloc::relpose_host::split_large;

static int g_fail = 0;
#define EXPECT(c)                                          \
  do {                                                     \
    if (!(c)) {                                            \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);   \
      ++g_fail;                                            \
    }                                                      \
  } while (0)

struct Case {
  std::vector<uint64_t> view_off{0, 3, 3, 7, 9};  // four views: 3, 0, 4 and 2 features
  std::vector<float> kpt = std::vector<float>(18, 1.0f);
  std::vector<uint32_t> wh{640, 480, 640, 480, 640, 480, 640, 480};
  std::vector<uint32_t> vintr{0, 1, 0, 1};
  std::vector<double> intr{700, 320, 240, 0, 0, 0, 720, 318, 242, -0.1, 0.02, 0};
  std::vector<uint32_t> itype{0, 3};
  std::vector<uint32_t> pairs{0, 2, 2, 3, 0, 3};
  std::vector<uint64_t> offsets{0, 2, 3, 5};
  std::vector<uint32_t> mi{0, 2, 3, 1, 1}, mj{1, 3, 0, 0, 1};
  std::vector<uint32_t> large{77};
  uint32_t large_max = 555;
  sfmloc_relpose_options opt{256, 0, 2.5, 1};
  std::string err;
  PairScene scene() const {
    return PairScene{view_off.data(), (uint32_t)view_off.size() - 1, kpt.data(),   wh.data(),
                     vintr.data(),    intr.data(),                   itype.data(), (uint32_t)itype.size(),
                     pairs.data(),    (uint32_t)(pairs.size() / 2),  offsets.data(), mi.data(),
                     mj.data()};
  }
  // the call's host side: the checks, then the split of a scene that passed them
  int run(const PairScene &sc) {
    const int rc = check(sc, opt, &err);
    if (rc == SFMLOC_OK) split_large(sc, &large, &large_max);
    return rc;
  }
  int run() { return run(scene()); }
  bool untouched() const { return large == std::vector<uint32_t>{77} && large_max == 555; }
};

int main() {
  {  // a good call: no large pair
    Case c;
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT(c.large.empty() && c.large_max == 0);
  }
  {  // no pairs at all
    Case c;
    PairScene sc = c.scene();
    sc.pairs = nullptr, sc.n_pairs = 0, sc.offsets = nullptr, sc.match_i = sc.match_j = nullptr;
    EXPECT(c.run(sc) == SFMLOC_OK);
    EXPECT(c.large.empty());
  }
  {  // a view index out of range: the text names the pair
    Case c;
    c.pairs[3] = 4;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 1 = (2, 4) out of range") != std::string::npos);
  }
  {  // an intrinsic index out of range; an intrinsic type that is neither 0 nor 3
    Case c;
    c.vintr[2] = 2;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("view 2 names intrinsic 2 of 2") != std::string::npos);
    Case d;
    d.itype[1] = 1;
    EXPECT(d.run() == SFMLOC_EINVAL && d.err.find("intrinsic 1 has type 1") != std::string::npos);
  }
  {  // a pair of a view with itself
    Case c;
    c.pairs[1] = 0;
    EXPECT(c.run() == SFMLOC_EINVAL && c.err.find("pair 0 names view 0 twice") != std::string::npos);
  }
  {  // a feature index out of range, on either side; a view without features takes no match
    Case c;
    c.mi[1] = 3;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair (0, 2) match 1 out of range") != std::string::npos);
    Case d;
    d.mj[2] = 2;
    EXPECT(d.run() == SFMLOC_EINVAL && d.err.find("pair (2, 3) match 0 out of range") != std::string::npos);
    Case e;
    e.pairs = {0, 1};
    e.offsets = {0, 1};
    e.mi = {0};
    e.mj = {0};
    EXPECT(e.run() == SFMLOC_EINVAL && e.err.find("pair (0, 1) match 0 out of range") != std::string::npos);
  }
  {  // offsets that go back or do not start at 0; view_off that goes back or does not start at 0
    Case d;
    d.offsets = {0, 3, 2, 5};
    EXPECT(d.run() == SFMLOC_EINVAL && d.untouched());
    Case e;
    e.view_off = {0, 3, 2, 7, 9};
    EXPECT(e.run() == SFMLOC_EINVAL && e.untouched());
    Case f;
    f.view_off[0] = 1;
    EXPECT(f.run() == SFMLOC_EINVAL && f.untouched());
    Case g;
    g.offsets[0] = 1;
    EXPECT(g.run() == SFMLOC_EINVAL && g.untouched());
  }
  {  // null arrays
    Case c;
    PairScene a = c.scene(), b = c.scene(), d = c.scene(), e = c.scene();
    a.view_off = nullptr;
    b.kpt_xy = nullptr;
    d.intrinsics = nullptr;
    e.match_i = nullptr;
    EXPECT(c.run(a) == SFMLOC_EINVAL);
    EXPECT(c.run(b) == SFMLOC_EINVAL);
    EXPECT(c.run(d) == SFMLOC_EINVAL);
    EXPECT(c.run(e) == SFMLOC_EINVAL);
    EXPECT(c.untouched());
  }
  {  // 2048 matches stay with the LDS form, 2049 and 65 536 are large, 65 537 is SFMLOC_ECAP (the text names the pair)
    for (uint32_t n : {2048u, 2049u, 65536u, 65537u}) {
      Case c;
      c.view_off = {0, 1, 1, 2, 2};
      c.kpt.assign(4, 1.0f);
      c.pairs = {0, 2, 2, 0};
      c.offsets = {0, 3, 3 + (uint64_t)n};
      c.mi.assign(3 + (size_t)n, 0);
      c.mj.assign(3 + (size_t)n, 0);
      const int rc = c.run();
      if (n == 65537u) {
        EXPECT(rc == SFMLOC_ECAP && c.untouched());
        EXPECT(c.err.find("pair (2, 0) has 65537 matches") != std::string::npos);
      } else if (n == 2048u) {
        EXPECT(rc == SFMLOC_OK && c.large.empty() && c.large_max == 0);
      } else {
        EXPECT(rc == SFMLOC_OK && c.large == std::vector<uint32_t>{1} && c.large_max == n);
      }
    }
  }
  {  // more than 2^32 - 2 feature rows
    Case c;
    c.view_off = {0, 3, 3, 7, 0xFFFFFFFFull};
    EXPECT(c.run() == SFMLOC_ECAP && c.untouched());
    EXPECT(c.err.find("feature rows") != std::string::npos);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK relpose_host\n");
  return 0;
}
