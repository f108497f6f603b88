// sfmloc::LocalizeEngine::localizeImageFile (include/sfmloc_engine.hpp) on one file by both routes -- the host decode
// and deviceDecode = true (entropy pass on the host, reconstruction and extraction on the device) -- which must agree in
// every returned double, 2D and 3D point and inlier index:
//   engine_file_decode <sfmDataDir> <matchDir> <file.jpg|png> ...
// prints per file "SAME <number of returned doubles> <number of 2D-3D points>" or "DIFF", returns 0 when all are the same.
#include <cstdio>
#include <string>
#include <vector>

#include "../../include/sfmloc_engine.hpp"

int main(int argc, char **argv) {
  if (argc < 4) return 2;
  int rc = 0;
  try {
    sfmloc::LocalizeEngine eng(argv[1], argv[2], "", 0.6, 25, 4.0, false, 0, 0);
    for (int a = 3; a < argc; ++a) {
      std::vector<double> p2[2], p3[2], times, r[2];
      std::vector<int> inl[2];
      for (int dev = 0; dev < 2; ++dev)
        r[dev] = eng.localizeImageFile(argv[a], true, p2[dev], p3[dev], inl[dev], false, times, std::vector<double>(), -1.0,
                                       nullptr, dev == 1);
      const bool same = r[0] == r[1] && p2[0] == p2[1] && p3[0] == p3[1] && inl[0] == inl[1];
      if (same) {
        printf("SAME %zu %zu\n", r[0].size(), p2[0].size() / 2);
      } else {
        printf("DIFF\n");
        rc = 1;
      }
    }
  } catch (const std::exception &e) {
    printf("ERROR %s\n", e.what());
    return 3;
  }
  return rc;
}
