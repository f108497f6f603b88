// Host check of the JPEG decoder's split (sfmlocalization_amd/csrc/jpeg_host.h): the entropy stage writes the
// coefficient blocks into memory the caller provides, the host reconstruction reads them from there, and the pixels are
// the ones sfmloc_image_decode returns -- for every file named on the command line, gray and colour.  The caller's
// memory is a heap block of exactly the size the device reader would give it, so an overrun is the sanitizer's to find.
// Stand-alone: linked with image_io.hip alone (host code), the error text kept here.
//   jpeg_coef FILE.jpg ...      prints "OK <files> files" and returns 0, or names the first difference
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "../../sfmlocalization_amd/csrc/jpeg_host.h"

static char g_error[512];
namespace sfmloc {
void set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_error, sizeof(g_error), fmt, ap);
  va_end(ap);
}
}  // namespace sfmloc

static bool read_file(const char *path, std::vector<uint8_t> *out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), f)) > 0) out->insert(out->end(), buf, buf + got);
  fclose(f);
  return true;
}

int main(int argc, char **argv) {
  int n_files = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<uint8_t> raw;
    if (!read_file(argv[a], &raw)) {
      printf("FAIL cannot read %s\n", argv[a]);
      return 1;
    }
    int32_t w = 0, h = 0;
    if (sfmloc_image_decode(raw.data(), raw.size(), 0, nullptr, 0, &w, &h) != SFMLOC_OK) {
      printf("FAIL %s: size query: %s\n", argv[a], g_error);
      return 1;
    }
    // every component has at most 2 * ceil(w / 16) blocks per row and 2 * ceil(h / 16) rows of blocks
    const size_t cap = 3 * (2 * (size_t)((w + 15) / 16) * 8) * (2 * (size_t)((h + 15) / 16) * 8);
    for (int color = 0; color < 2; ++color) {
      std::vector<uint8_t> want((size_t)w * h * (color ? 3 : 1));
      int32_t w2 = 0, h2 = 0;
      if (sfmloc_image_decode(raw.data(), raw.size(), color, want.data(), want.size(), &w2, &h2) != SFMLOC_OK) {
        printf("FAIL %s: sfmloc_image_decode: %s\n", argv[a], g_error);
        return 1;
      }
      int16_t *coef = static_cast<int16_t *>(malloc(cap * sizeof(int16_t)));
      memset(coef, 0x55, cap * sizeof(int16_t));  // (the entropy stage zeroes what it uses)
      std::vector<uint8_t> got;
      std::string err;
      int gw = 0, gh = 0;
      if (!sfmloc::jpeg_decode_split_host(raw.data(), raw.size(), color != 0, coef, cap, &gw, &gh, &got, &err)) {
        printf("FAIL %s: split decode: %s\n", argv[a], err.c_str());
        return 1;
      }
      bool touched = false;  // the blocks did land in the caller's memory
      for (size_t i = 0; i < 64 && !touched; ++i) touched = coef[i] != 0x5555;
      free(coef);
      if (gw != w || gh != h || got != want || !touched) {
        printf("FAIL %s color %d: %dx%d vs %dx%d, pixels %s, caller's memory %s\n", argv[a], color, gw, gh, w, h,
               got == want ? "equal" : "differ", touched ? "written" : "untouched");
        return 1;
      }
      // a buffer one block short is refused, not overrun
      int16_t *small = static_cast<int16_t *>(malloc(64 * sizeof(int16_t)));
      const bool refused = !sfmloc::jpeg_decode_split_host(raw.data(), raw.size(), color != 0, small, 0, &gw, &gh, &got, &err);
      free(small);
      if (!refused) {
        printf("FAIL %s: an empty coefficient buffer was accepted\n", argv[a]);
        return 1;
      }
    }
    ++n_files;
  }
  printf("OK %d files\n", n_files);
  return 0;
}
