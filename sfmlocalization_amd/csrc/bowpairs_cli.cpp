// ComputeBoWPairs: the pair list of a map under construction from its views' BoW vectors, as a C++ host program over
// the C ABI (plain g++, no HIP in the host code):
//
//   ComputeBoWPairs -m <matchDir> [-k 20] [-v 0] [-w <window>] [--mutual] [-o <matchDir>/pairs.bow.txt] [--device 0]
//                   [--profile]
//
// The same program as sfmlocalization_amd/bowpairs.py (its docstring states the workflow: ExtFeatAndMatch -sm, TrainBoW,
// this, ExtFeatAndMatch -p), and the same bytes: the views of <matchDir>/sfm_data.json ascending by id, each view's
// <base>.bow as float32, sfmloc_bow_knn over all of them with the window, the k-NN pairs (with --mutual only those both
// views list) united with the -v neighbours, one "a b" line per pair in ascending order (hulo::readPairFile's format).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_files.h"

using namespace sfmfiles;

namespace {

const char *kName = "ComputeBoWPairs";

void usage() {
  fprintf(stderr,
          "Usage: %s\n"
          "[-m|--match_dir] the directory of sfm_data.json and the views' .bow vectors\n"
          "\n[Optional]\n"
          "[-k|--knn] neighbours per view (20)\n"
          "[-v|--video_frame] pair every view with the next v views as well (0)\n"
          "[-w|--window] the k-NN of view i looks only at views more than w places away (the value of -v)\n"
          "[--mutual] keep a k-NN pair only if each view lists the other\n"
          "[-o|--output_file] the pair file to write (default: pairs.bow.txt in the match directory)\n"
          "[--device] HIP device (0)\n"
          "[--profile] print the device milliseconds\n",
          kName);
}

bool whole_number(const std::string &s, long long *out) {
  char *end = nullptr;
  *out = strtoll(s.c_str(), &end, 10);
  return !s.empty() && *end == '\0';
}

}  // namespace

int main(int argc, char **argv) {
  std::string match_dir, k_txt = "20", v_txt = "0", w_txt, out_file = "pairs.bow.txt", dev_txt = "0";
  bool mutual = false, profile = false;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    std::string *dst = nullptr;
    if (a == "--mutual" || a == "--profile") {
      (a == "--mutual" ? mutual : profile) = true;
      continue;
    }
    if (a.compare(0, 9, "--device=") == 0) {
      dev_txt = a.substr(9);
      continue;
    }
    if (a == "-m" || a == "--match_dir") dst = &match_dir;
    else if (a == "-k" || a == "--knn") dst = &k_txt;
    else if (a == "-v" || a == "--video_frame") dst = &v_txt;
    else if (a == "-w" || a == "--window") dst = &w_txt;
    else if (a == "-o" || a == "--output_file") dst = &out_file;
    else if (a == "--device") dst = &dev_txt;
    if (!dst || i + 1 >= argc) {
      usage();
      return 1;
    }
    *dst = argv[++i];
  }
  long long k = 0, video_frame = 0, window = 0, device = 0;
  if (!whole_number(k_txt, &k) || !whole_number(v_txt, &video_frame) || !whole_number(dev_txt, &device) ||
      (!w_txt.empty() && !whole_number(w_txt, &window)) || match_dir.empty() || out_file.empty() || k < 1 ||
      k > 0xFFFFFFFFll || video_frame < 0 || window < 0) {
    usage();
    return 1;
  }
  if (w_txt.empty()) window = video_frame;
  if (window > 0xFFFFFFFFll) window = 0xFFFFFFFFll;  // (past every view either way)

  const std::string sd_path = join(match_dir, "sfm_data.json");
  sfmloc_view_list *vl = nullptr;
  uint32_t n = 0;
  if (sfmloc_view_list_open(sd_path.c_str(), &vl, &n)) {
    fprintf(stderr, "%s: %s cannot be read. (%s)\n", kName, sd_path.c_str(), sfmloc_last_error());
    return 1;
  }
  std::vector<uint32_t> ids(n);
  std::vector<std::string> bow_path(n);
  for (uint32_t v = 0; v < n; ++v) {
    uint32_t w, h;
    const char *img = nullptr;
    sfmloc_view_list_get(vl, v, &ids[v], &w, &h, &img);
    bow_path[v] = join(match_dir, basename_part(img) + ".bow");
  }
  sfmloc_view_list_close(vl);
  if (n < 2) {
    fprintf(stderr, "%s: %s: %u views (at least two)\n", kName, sd_path.c_str(), n);
    return 1;
  }
  std::vector<float> bow;
  size_t dim = 0;
  for (uint32_t v = 0; v < n; ++v) {
    const std::string &path = bow_path[v];
    if (!is_file(path)) {
      fprintf(stderr, "%s: %s: no BoW vector of view %u (TrainBoW writes them)\n", kName, path.c_str(), ids[v]);
      return 1;
    }
    int32_t rows = 0, cols = 0;
    std::vector<double> vec;
    if (!read_mat_bin(path, &rows, &cols, &vec)) {
      fprintf(stderr, "%s: %s cannot be read.\n", kName, path.c_str());
      return 1;
    }
    if (vec.empty()) {
      fprintf(stderr, "%s: %s: an empty BoW vector\n", kName, path.c_str());
      return 1;
    }
    if (v && vec.size() != dim) {
      fprintf(stderr, "%s: %s: %zu values, %s has %zu\n", kName, path.c_str(), vec.size(), bow_path[0].c_str(), dim);
      return 1;
    }
    dim = vec.size();
    for (double x : vec) bow.push_back((float)x);
  }

  sfmloc_bowknn_options opt;
  sfmloc_bowknn_default_options(&opt);
  opt.k = (uint32_t)k;
  opt.window = (uint32_t)window;
  opt.profile = profile ? 1u : 0u;
  if ((unsigned long long)n * opt.k > (1ull << 32)) {  // (refused by the call as well: before the arrays are sized)
    fprintf(stderr, "%s: %u views x k = %u: more than 2^32 entries\n", kName, n, opt.k);
    return 1;
  }
  std::vector<uint32_t> nbr((size_t)n * opt.k), count(n);
  std::vector<float> dist((size_t)n * opt.k);
  if (sfmloc_bow_knn((int)device, bow.data(), n, (uint32_t)dim, &opt, nbr.data(), dist.data(), count.data())) {
    fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
    return 1;
  }

  // bowpairs.knn_pairs: a std::set of (a, b) is unique and ascending by (a, b)
  std::set<std::pair<uint32_t, uint32_t>> pairs;
  const auto lists = [&](uint32_t i, uint32_t j) {  // row i's list names j (it ascends)
    const uint32_t *row = nbr.data() + (size_t)i * opt.k;
    uint32_t lo = 0, hi = count[i];
    while (lo < hi) {
      const uint32_t mid = (lo + hi) / 2;
      if (row[mid] < j) lo = mid + 1;
      else hi = mid;
    }
    return lo < count[i] && row[lo] == j;
  };
  for (uint32_t i = 0; i < n; ++i)
    for (uint32_t s = 0; s < count[i]; ++s) {
      const uint32_t j = nbr[(size_t)i * opt.k + s];
      if (mutual && !lists(j, i)) continue;
      pairs.emplace(ids[i < j ? i : j], ids[i < j ? j : i]);
    }
  for (uint32_t i = 0; i < n; ++i)  // extfeat.generate_video_match_pairs (SfMDataUtils.cpp:144-157)
    for (uint64_t j = (uint64_t)i + 1; j < n && j <= (uint64_t)i + (uint64_t)video_frame; ++j) pairs.emplace(ids[i], ids[j]);

  const std::string path = (!out_file.empty() && out_file[0] == '/') ? out_file : join(match_dir, out_file);
  FILE *f = fopen(path.c_str(), "w");
  bool ok = f != nullptr;
  if (f) {
    for (const auto &p : pairs) ok = fprintf(f, "%u %u\n", p.first, p.second) > 0 && ok;
    ok = fclose(f) == 0 && ok;
  }
  if (!ok) {
    fprintf(stderr, "%s: %s cannot be written.\n", kName, path.c_str());
    return 1;
  }
  printf("BoW pairs: %zu pairs of %u views (k %u, window %u) -> %s\n", pairs.size(), n, opt.k, opt.window, path.c_str());
  if (profile) printf("device %.3f ms\n", sfmloc_bowknn_last_ms());
  return 0;
}
