// Host program over sfmlocalization_amd/csrc/globalposes_host.h, the host side of sfmloc_global_poses: every refusal
// with its code and text, the adjacency the kernels gather over and the choice of the component.  No HIP, no GPU: meant
// to be built with -fsanitize=address,undefined and run on the CPU (tests/test_globalposes_cpu.py does).
#include <cmath>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/globalposes_host.h"

using namespace sfmloc::gposes_host;

static int g_fail = 0;
#define EXPECT(c)                                        \
  do {                                                   \
    if (!(c)) {                                          \
      printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c); \
      ++g_fail;                                          \
    }                                                    \
  } while (0)

struct Case {
  uint32_t n_views = 5;
  std::vector<uint32_t> pairs{3, 1, 0, 1, 1, 2, 4, 0};  // (3, 1), (0, 1), (1, 2), (4, 0)
  std::vector<double> R, t;
  Adjacency adj;
  std::string err;
  Case() { fill(); }
  void fill() {
    const size_t P = pairs.size() / 2;
    R.assign(9 * P, 0.0);
    t.assign(3 * P, 0.0);
    for (size_t k = 0; k < P; ++k) {
      const double c = std::cos(0.3 * (k + 1)), s = std::sin(0.3 * (k + 1));  // a rotation about z
      const double r[9] = {c, -s, 0, s, c, 0, 0, 0, 1};
      for (int i = 0; i < 9; ++i) R[9 * k + i] = r[i];
      t[3 * k + 1] = 1.0;
    }
  }
  int run() { return check(n_views, pairs.data(), (uint32_t)(pairs.size() / 2), R.data(), t.data(), &adj, &err); }
  bool untouched() const { return adj.off.empty() && adj.nbr.empty() && adj.pe.empty(); }
};

int main() {
  {  // a good call: the adjacency ascends by neighbour and marks the pair's J
    Case c;
    EXPECT(c.run() == SFMLOC_OK);
    EXPECT((c.adj.off == std::vector<uint32_t>{0, 2, 5, 6, 7, 8}));
    EXPECT((c.adj.nbr == std::vector<uint32_t>{1, 4, 0, 2, 3, 1, 1, 0}));
    EXPECT((c.adj.pe == std::vector<uint32_t>{1, 3 | kDirBit, 1 | kDirBit, 2, 0 | kDirBit, 2 | kDirBit, 0, 3}));
    EXPECT(c.adj.heavy.empty());
  }
  {  // no pairs at all; no views at all
    Case c;
    EXPECT(check(5, nullptr, 0, nullptr, nullptr, &c.adj, &c.err) == SFMLOC_OK);
    EXPECT((c.adj.off == std::vector<uint32_t>(6, 0)) && c.adj.nbr.empty());
    EXPECT(check(0, nullptr, 0, nullptr, nullptr, &c.adj, &c.err) == SFMLOC_OK && c.adj.off.size() == 1);
  }
  {  // a view index out of range; a pair of a view with itself
    Case c;
    c.pairs[5] = 5;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 2 = (1, 5) out of range") != std::string::npos);
    Case d;
    d.pairs[2] = 1;
    EXPECT(d.run() == SFMLOC_EINVAL && d.untouched() && d.err.find("pair 1 names view 1 twice") != std::string::npos);
  }
  {  // the same unordered pair twice, in either order
    Case c;
    c.pairs = {3, 1, 0, 1, 1, 3};
    c.fill();
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 2 lists the views (1, 3) of pair 0 again") != std::string::npos);
  }
  {  // a non-finite entry, in R and in t
    Case c;
    c.R[9 + 4] = std::numeric_limits<double>::quiet_NaN();
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 1 = (0, 1) has a non-finite entry") != std::string::npos);
    Case d;
    d.t[6] = std::numeric_limits<double>::infinity();
    EXPECT(d.run() == SFMLOC_EINVAL && d.err.find("pair 2 = (1, 2) has a non-finite entry") != std::string::npos);
  }
  {  // R off a rotation by more than 1e-6, and by less; |t| off 1 by more, and by less
    Case c;
    c.R[0] += 1e-5;
    EXPECT(c.run() == SFMLOC_EINVAL && c.untouched());
    EXPECT(c.err.find("pair 0 = (3, 1): rel_R is not orthonormal") != std::string::npos);
    Case d;
    d.R[0] += 1e-8;
    EXPECT(d.run() == SFMLOC_OK);
    Case e;
    e.t[3 * 3 + 1] = 1.0 + 1e-5;
    EXPECT(e.run() == SFMLOC_EINVAL && e.err.find("pair 3 = (4, 0): rel_t is not of unit length") != std::string::npos);
    Case f;
    f.t[3 * 3 + 1] = 1.0 + 1e-8;
    EXPECT(f.run() == SFMLOC_OK);
  }
  {  // null arrays with pairs
    Case c;
    EXPECT(check(5, nullptr, 4, c.R.data(), c.t.data(), &c.adj, &c.err) == SFMLOC_EINVAL);
    EXPECT(check(5, c.pairs.data(), 4, nullptr, c.t.data(), &c.adj, &c.err) == SFMLOC_EINVAL);
    EXPECT(check(5, c.pairs.data(), 4, c.R.data(), nullptr, &c.adj, &c.err) == SFMLOC_EINVAL && c.untouched());
  }
  {  // a view of kWaveDegree pairs is a lane's, one more makes it a wave's
    for (uint32_t deg : {kWaveDegree, kWaveDegree + 1}) {
      Case c;
      c.n_views = deg + 1;
      c.pairs.clear();
      for (uint32_t v = deg; v >= 1; --v) {  // (descending: the builder sorts)
        c.pairs.push_back(v % 2 ? 0 : v);
        c.pairs.push_back(v % 2 ? v : 0);
      }
      c.fill();
      EXPECT(c.run() == SFMLOC_OK);
      EXPECT(c.adj.off[1] == deg && c.adj.off[deg + 1] == 2 * deg);
      for (uint32_t e = 0; e < deg; ++e) {
        EXPECT(c.adj.nbr[e] == e + 1);
        EXPECT((c.adj.pe[e] & ~kDirBit) == deg - 1 - e);
        EXPECT(((c.adj.pe[e] & kDirBit) != 0) == ((e + 1) % 2 == 0));
      }
      EXPECT(c.adj.heavy == (deg > kWaveDegree ? std::vector<uint32_t>{0} : std::vector<uint32_t>{}));
    }
  }
  {  // the component: the most views, the smallest label on a tie, none below two views
    uint32_t root = 9, size = 9;
    pick_component({0, 1, 1, 0, 4, 1}, &root, &size);
    EXPECT(root == 1 && size == 3);
    pick_component({0, 1, 1, 0, 4, 4}, &root, &size);
    EXPECT(root == 0 && size == 2);
    pick_component({0, 1, 2}, &root, &size);
    EXPECT(size == 1);
    pick_component({}, &root, &size);
    EXPECT(size == 0);
  }
  if (g_fail) {
    printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  printf("OK globalposes_host\n");
  return 0;
}
