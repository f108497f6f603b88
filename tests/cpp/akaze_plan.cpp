// Host program over sfmlocalization_amd/csrc/akaze_plan.h, the header sfmloc_akaze_create plans with and
// build_scale_space / akaze_detect_enqueue launch by: prints the plan and the launch schedule of every request on its
// command line for tests/akaze_header.py to parse (test_akaze_plan.py compares the plan with the CPU restatement's,
// test_akaze_cases_cpu.py the schedule with what the boundary cases promise).
//   usage: akaze_plan w h n_octaves n_sublevels [w h n_octaves n_sublevels ...]
//   first:        "constants name value name value ..."  (the header's thresholds)
//   per request:  "plan w h n_octaves n_sublevels <n_levels> <total floats>", then per level
//                 "level i w h octave sublevel sigma_size nsteps off <nsteps hex words: the bits of tsteps>", then
//                 "detect rows segs_per_row n_seg seg_chunks scan_two_launches hist_grid_x grad_grid_y hist_grid_y
//                         nbr_grid desc_grid cand_cap spec_start spec_max", then per need = 1 .. n_levels
//                 "evo need <levels built> <n_steps>" and per step
//                 "step resident first last halfsample source fuse n_launch"   (source: prev, own or scratch)
//            or:  "refused w h n_octaves n_sublevels <level> <steps>"
// A request check_request does not accept ends the program with status 2.
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
  printf("constants kMinSide %d kMaxWidth %d kSupMaxRows %d kMaxOctaves %d kMaxLevels %d kMaxFedSteps %d "
         "kResidentLdsBytes %u kOctaveRunMax %d kNldStepsLarge %d kNldStepsSmall %d kNldSmallWidth %d kNldFuseMax %d "
         "kGradRows %d kHistGridMax %u kSegPx %d kSegChunk %u kSegScanOneLaunch %u kSegChunksMax %u kCandCap %u "
         "kSpecStart %u kSpecMax %u kNbrPixPerGroup %u kNbrGridMin %u kNbrGridMax %u kDescPixPerGroup %u kDescGridMin %u "
         "kDescGridMax %u\n",
         kMinSide, kMaxWidth, kSupMaxRows, kMaxOctaves, kMaxLevels, kMaxFedSteps, kResidentLdsBytes, kOctaveRunMax,
         kNldStepsLarge, kNldStepsSmall, kNldSmallWidth, kNldFuseMax, kGradRows, kHistGridMax, kSegPx, kSegChunk,
         kSegScanOneLaunch, kSegChunksMax, kCandCap, kSpecStart, kSpecMax, kNbrPixPerGroup, kNbrGridMin, kNbrGridMax,
         kDescPixPerGroup, kDescGridMin, kDescGridMax);
  for (int a = 1; a + 3 < argc; a += 4) {
    const int w = atoi(argv[a]), h = atoi(argv[a + 1]), omax = atoi(argv[a + 2]), nsub = atoi(argv[a + 3]);
    if (check_request(w, h, omax, nsub) != kRequestOk) {
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
    const Detection D = detection(*P, w, h);
    printf("detect %u %u %u %u %d %u %u %u %u %u %u %u %u\n", D.rows, D.segs_per_row, D.n_seg, D.seg_chunks,
           (int)D.scan_two_launches, D.hist_grid_x, D.grad_grid_y, D.hist_grid_y, D.nbr_grid, D.desc_grid, D.cand_cap,
           D.spec_start, D.spec_max);
    for (int need = 1; need <= P->nlev; ++need) {
      EvoStep steps[kMaxLevels];
      const int n = evolution(*P, need, steps);
      printf("evo %d %d %d\n", need, levels_built(*P, need), n);
      for (int e = 0; e < n; ++e) {
        const EvoStep &E = steps[e];
        printf("step %d %d %d %d %s %d %d\n", (int)E.resident, E.first, E.last, (int)E.halfsample,
               E.source == kPrevLt ? "prev" : (E.source == kOwnLt ? "own" : "scratch"), E.fuse, E.n_launch);
      }
    }
  }
  return 0;
}
