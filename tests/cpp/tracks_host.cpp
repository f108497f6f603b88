// Host program over sfmlocalization_amd/csrc/tracks_host.h, the host side of sfmloc_tracks_build: every refusal with its
// code and text, and the flattening of a pair list into edges between global feature rows.  No HIP, no GPU: meant to be
// built with -fsanitize=address,undefined and run on the CPU (tests/test_structure_cpu.py does).
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/tracks_host.h"

using sfmloc::PairScene;
using sfmloc::tracks_host::flatten;

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
  std::vector<uint8_t> use;
  std::vector<uint32_t> pairs{0, 2, 2, 3, 0, 3};
  std::vector<uint64_t> offsets{0, 2, 3, 5};
  std::vector<uint32_t> mi{0, 2, 3, 1, 1}, mj{1, 3, 0, 0, 1};
  std::vector<uint32_t> ea{99}, eb{98};
  uint64_t n_nodes = 12345;
  std::string err;
  PairScene scene() const {  // (nothing of the cameras)
    PairScene sc{};
    sc.view_off = view_off.data(), sc.n_views = (uint32_t)view_off.size() - 1;
    sc.pairs = pairs.data(), sc.n_pairs = (uint32_t)(pairs.size() / 2), sc.offsets = offsets.data();
    sc.match_i = mi.data(), sc.match_j = mj.data();
    return sc;
  }
  int run(const PairScene &sc) { return flatten(sc, use.empty() ? nullptr : use.data(), &ea, &eb, &n_nodes, &err); }
  int run() { return run(scene()); }
  bool untouched() const { return ea == std::vector<uint32_t>{99} && eb == std::vector<uint32_t>{98} && n_nodes == 12345; }
};

int main() {
  {  // the flattening: node = view_off[view] + feature, pair order, match order
    Case c;
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT(c.n_nodes == 9);
    EXPECT((c.ea == std::vector<uint32_t>{0, 2, 6, 1, 1}));
    EXPECT((c.eb == std::vector<uint32_t>{4, 6, 7, 7, 8}));
  }
  {  // a masked-out view: its pairs contribute nothing, and are still checked
    Case c;
    c.use = {1, 1, 1, 0};
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT((c.ea == std::vector<uint32_t>{0, 2}) && (c.eb == std::vector<uint32_t>{4, 6}));
    c.mj[4] = 2;  // view 3 has two features
    c.ea = {99};
    c.eb = {98};
    c.n_nodes = 12345;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair (0, 3) match 1 out of range") != std::string::npos);
  }
  {  // no pairs at all
    Case c;
    c.pairs.clear();
    c.offsets = {0};
    c.mi.clear();
    c.mj.clear();
    PairScene sc{};
    sc.view_off = c.view_off.data(), sc.n_views = 4;
    EXPECT(c.run(sc) == SFMLOC_OK);
    EXPECT(c.ea.empty() && c.eb.empty() && c.n_nodes == 9);
  }
  {  // a view index out of range: the text names the pair
    Case c;
    c.pairs[3] = 4;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 1 = (2, 4) out of range") != std::string::npos);
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
  {  // a pair of a view with itself; offsets that go back; view_off that goes back or does not start at 0
    Case c;
    c.pairs[1] = 0;
    EXPECT(c.run() == SFMLOC_EINVAL && c.err.find("names view 0 twice") != std::string::npos);
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
    PairScene a = c.scene(), b = c.scene(), d = c.scene();
    a.view_off = nullptr;
    b.pairs = nullptr;
    d.match_i = nullptr;
    EXPECT(c.run(a) == SFMLOC_EINVAL);
    EXPECT(c.run(b) == SFMLOC_EINVAL);
    EXPECT(c.run(d) == SFMLOC_EINVAL);
    EXPECT(c.untouched());
  }
  {  // more than 2^32 - 2 feature rows: SFMLOC_ECAP before any match is looked at; 2^32 - 2 rows pass
    Case c;
    c.view_off = {0, 3, 3, 7, 0xFFFFFFFFull};
    EXPECT(c.run() == SFMLOC_ECAP && c.untouched());
    EXPECT(c.err.find("feature rows") != std::string::npos);
    c.view_off.back() = 0xFFFFFFFEull;
    EXPECT(c.run() == SFMLOC_OK && c.n_nodes == 0xFFFFFFFEull);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK tracks_host\n");
  return 0;
}
