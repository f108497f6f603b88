// Host program over sfmlocalization_amd/csrc/akaze_plan.h, the header sfmloc_akaze_create plans with: prints the plan of
// every request on its command line for tests/test_akaze_plan.py to compare with the CPU restatement's.
//   usage: akaze_plan w h n_octaves n_sublevels [w h n_octaves n_sublevels ...]
//   per request:  "plan w h n_octaves n_sublevels <n_levels> <total floats>", then per level
//                 "level i w h octave sublevel sigma_size nsteps off <nsteps hex words: the bits of tsteps>"
//            or:  "refused w h n_octaves n_sublevels <level> <steps>"
// No HIP, no library: it builds with the host compiler alone, with or without its sanitizers.
#include <stdio.h>
#include <stdlib.h>

#include <memory>

#include "../../sfmlocalization_amd/csrc/akaze_plan.h"

using namespace sfmloc::akaze_plan;

int main(int argc, char **argv) {
  if (argc < 5 || (argc - 1) % 4 != 0) {
    fprintf(stderr, "usage: %s w h n_octaves n_sublevels [...]\n", argv[0]);
    return 2;
  }
  setvbuf(stdout, nullptr, _IOLBF, 0);  // (whatever stops the program, the plans before it are out)
  for (int a = 1; a + 3 < argc; a += 4) {
    const int w = atoi(argv[a]), h = atoi(argv[a + 1]), omax = atoi(argv[a + 2]), nsub = atoi(argv[a + 3]);
    // what sfmloc_akaze_create checks before it plans
    if (w < 16 || h < 16 || w > 16384 || h > 4096 || omax < 1 || omax > 8 || nsub < 1 || omax * nsub > kMaxLevels) {
      fprintf(stderr, "request %d %d %d %d is outside what sfmloc_akaze_create accepts\n", w, h, omax, nsub);
      return 2;
    }
    std::unique_ptr<AkPlan> P(new AkPlan());
    int bad_level = -1, bad_steps = -1;
    if (!make_plan(w, h, omax, nsub, *P, &bad_level, &bad_steps)) {
      printf("refused %d %d %d %d %d %d\n", w, h, omax, nsub, bad_level, bad_steps);
      continue;
    }
    printf("plan %d %d %d %d %d %zu\n", w, h, omax, nsub, P->nlev, P->total);
    for (int i = 0; i < P->nlev; ++i) {
      const AkLevel &L = P->lev[i];
      printf("level %d %d %d %d %d %d %d %zu", i, L.w, L.h, L.octave, L.sublevel, L.sigma_size, L.nsteps, L.off);
      for (int k = 0; k < L.nsteps; ++k) {
        uint32_t bits;
        memcpy(&bits, &L.tsteps[k], 4);
        printf(" %08x", bits);
      }
      printf("\n");
    }
  }
  return 0;
}
