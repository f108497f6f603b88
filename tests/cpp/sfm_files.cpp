// Host test driver of sfmlocalization_amd/csrc/sfm_files.h, the C++ tools' file formats (plain g++, no library, no GPU):
// every command prints one line per case, and tests/test_sfm_files.py holds the lines against what fileio.py, os.path
// and engine.parse_cv_args give for the same input.
//
//   sfm_files paths P...          path <basename_of>|<dirname_of>|<stem_of>|<basename_part>|<ext_of>
//   sfm_files join A B [A B]...   join <join(A, B)>
//   sfm_files kind P...           kind file | dir | none
//   sfm_files number S...         number 0 | 1
//   sfm_files feat F...           feat refused | feat <rows> <x bits> <y bits> ...      (after two floats already there)
//   sfm_files desc F...           desc ok|refused <bytes in hex>                        (after 64 bytes 0xAB already there)
//   sfm_files matches F ID...     matches refused <why> | matches <pairs> / <offsets> / <i> / <j>   (view index = place of ID)
//   sfm_files rewrite IN OUT      rewrite refused <why> | rewrite ok                    (read_matches, write_matches)
//   sfm_files args ARGV...        pos <p> per positional, opt <key>=<value> flag=<0|1> per option
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../sfmlocalization_amd/csrc/sfm_files.h"

using namespace sfmfiles;

namespace {

void print_list(const std::vector<uint32_t> &v) {
  for (size_t i = 0; i < v.size(); ++i) printf("%s%u", i ? "," : "", v[i]);
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  const std::string cmd = argv[1];
  if (cmd == "paths") {
    for (int i = 2; i < argc; ++i)
      printf("path %s|%s|%s|%s|%s\n", basename_of(argv[i]).c_str(), dirname_of(argv[i]).c_str(), stem_of(argv[i]).c_str(),
             basename_part(argv[i]).c_str(), ext_of(argv[i]).c_str());
  } else if (cmd == "join") {
    for (int i = 2; i + 1 < argc; i += 2) printf("join %s\n", join(argv[i], argv[i + 1]).c_str());
  } else if (cmd == "kind") {
    for (int i = 2; i < argc; ++i) printf("kind %s\n", is_file(argv[i]) ? "file" : is_dir(argv[i]) ? "dir" : "none");
  } else if (cmd == "number") {
    for (int i = 2; i < argc; ++i) printf("number %d\n", is_number(argv[i]) ? 1 : 0);
  } else if (cmd == "feat") {
    for (int i = 2; i < argc; ++i) {
      std::vector<float> xy{-1.0f, -2.0f};  // read_feat appends
      if (!read_feat(argv[i], &xy) || xy.size() < 2 || xy[0] != -1.0f || xy[1] != -2.0f) {
        printf("feat refused\n");
        continue;
      }
      printf("feat %zu", (xy.size() - 2) / 2);
      for (size_t k = 2; k < xy.size(); ++k) {
        uint32_t bits;
        memcpy(&bits, &xy[k], 4);
        printf(" %08x", bits);
      }
      printf("\n");
    }
  } else if (cmd == "desc") {
    for (int i = 2; i < argc; ++i) {
      std::vector<uint8_t> rows(64, 0xAB);  // read_desc appends, and leaves the vector alone when it refuses
      printf("desc %s ", read_desc(argv[i], &rows) ? "ok" : "refused");
      for (uint8_t b : rows) printf("%02x", b);
      printf("\n");
    }
  } else if (cmd == "matches" && argc >= 3) {
    std::map<uint32_t, uint32_t> view_index;
    for (int i = 3; i < argc; ++i) view_index[(uint32_t)strtoul(argv[i], nullptr, 10)] = (uint32_t)(i - 3);
    PairList pl;
    std::string err;
    if (!read_matches(argv[2], view_index, &pl, &err)) {
      printf("matches refused %s\n", err.c_str());
      return 0;
    }
    printf("matches ");
    print_list(pl.pairs);
    printf(" / ");
    for (size_t i = 0; i < pl.offsets.size(); ++i) printf("%s%llu", i ? "," : "", (unsigned long long)pl.offsets[i]);
    printf(" / ");
    print_list(pl.mi);
    printf(" / ");
    print_list(pl.mj);
    printf("\n");
  } else if (cmd == "rewrite" && argc == 4) {
    PairMatches m;
    std::string err;
    if (!read_matches(argv[2], &m, &err)) printf("rewrite refused %s\n", err.c_str());
    else printf("rewrite %s\n", write_matches(argv[3], m) ? "ok" : "refused cannot be written");
  } else if (cmd == "args") {
    const Args a = parse_args(argc - 1, argv + 1);  // (argv[1], the command, stands where a program's name does)
    for (const std::string &p : a.pos) printf("pos %s\n", p.c_str());
    for (const auto &kv : a.opt)
      printf("opt %s=%s flag=%d\n", kv.first.c_str(), kv.second.c_str(), a.flag({kv.first.c_str()}) ? 1 : 0);
  } else {
    return 2;
  }
  return 0;
}
