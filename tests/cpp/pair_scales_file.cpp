// Host program over the pair_scales.json codec of sfmlocalization_amd/csrc/sfm_files.h:
//   pair_scales_file <in> <out>    reads <in> and writes what it read to <out>; 1 with the reader's text when it refuses
// tests/test_pairscales_cpu.py holds the bytes against fileio.write_pair_scales'.
#include <cstdio>
#include <string>

#include "../../sfmlocalization_amd/csrc/sfm_files.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  sfmfiles::PairScales ps;
  std::string err;
  if (!sfmfiles::read_pair_scales(argv[1], &ps, &err)) {
    printf("refused: %s\n", err.c_str());
    return 1;
  }
  if (!sfmfiles::write_pair_scales(argv[2], ps)) return 3;
  printf("OK %zu records, min_shared %u, max_shared %u\n", ps.rec.size(), ps.min_shared, ps.max_shared);
  return 0;
}
