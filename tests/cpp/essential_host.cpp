// Host program over sfmlocalization_amd/csrc/essential_device.h: the five-point solver's host instantiation (one lane
// after the other per phase), on the rows of a binary file -- int32 n, then n rows of 20 doubles (x1[10], x2[10]) --
// writing n rows of 91 doubles (count, then up to 10 E) to a second file.  No HIP, no GPU; built with
// -ffp-contract=off, the library's rule.  tests/test_relpose_cpu.py compares the output with the restatement's bits.
#include <cstdio>
#include <vector>

#include "../../sfmlocalization_amd/csrc/essential_device.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  int n = 0;
  if (!f || fread(&n, sizeof n, 1, f) != 1 || n < 0) return 2;
  std::vector<double> in(20 * (size_t)n);
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) return 2;
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  static sfmloc::essential::RpGroupLds L;
  for (int b = 0; b < n; ++b) {
    double out[91] = {0.0};
    out[0] = (double)sfmloc::essential::five_point_group(L, &in[20 * (size_t)b], &in[20 * (size_t)b + 10], out + 1);
    if (fwrite(out, sizeof(double), 91, o) != 91) return 2;
  }
  fclose(o);
  printf("OK essential_host %d\n", n);
  return 0;
}
