// TrainBoW (TrainBoW/src/TrainBoW.cpp) as a C++ host program over the C ABI (plain g++, no HIP in the host code):
//
//   TrainBoW <inputDir> <bowFile> [-p=pcaFile] [--device=0]
//
// The same program as sfmlocalization_amd/trainbow.py, and the same bytes: every matches/sfm_data.json below inputDir
// (readSfmDataFiles, :60-93, directories in sorted order), 3 000 draws x 100 dense rows with the restated cv::RNG
// (getRandomTrainFeatures, :95-131: sfmloc_bowtrain_add_image), PCA (:174-203: sfmloc_bowtrain_pca; the k-means sample
// of the reference is drawn by a fresh cv::RNG, i.e. it is the PCA sample: it is projected in place), k-means
// (BoFSpatialPyramids::trainKMeans: sfmloc_bowtrain_kmeans), BOWfile.yml / PCAfile.yml as the project's
// fileio.write_cv_yaml writes them (floats as their shortest round-trip text), and one <view>.bow per view next to its
// sfm_data.json (saveMatBin, :238-272: sfmloc_imgbow_*).
//   TrainBoW --format-floats v...   prints each float32 as the YAML writer does (a test hook of the number format)
#include <dirent.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_files.h"
#include "sfm_json.h"

using namespace sfmfiles;

namespace {

const int kPcaTrainFeatureNum = 300000, kPcaPerImage = 100;        // TrainBoW.cpp:46-54
const int kKmeansTrainFeatureNum = 300000, kKmeansPerImage = 100;
const int kK = 100, kPcaDim = 32, kPyramidLevel = 2, kResized = 300;
const int kKmeansIteration = 100, kKmeansAttempts = 3;             // BoFSpatialPyramids.cpp:29, :100-103
const uint64_t kKmeansSeed = 0xFFFFFFFFull;                        // cv::theRNG() of a fresh process
const uint32_t kBatch = 8;

// the last part of a directory's name, however many slashes end it
std::string folder_name(std::string d) {
  while (d.size() > 1 && d.back() == '/') d.pop_back();
  return basename_of(d);
}
std::vector<std::string> sorted_entries(const std::string &d) {
  std::vector<std::string> out;
  DIR *dir = opendir(d.c_str());
  if (!dir) return out;
  for (dirent *e = readdir(dir); e; e = readdir(dir)) {
    const std::string n = e->d_name;
    if (n != "." && n != "..") out.push_back(n);
  }
  closedir(dir);
  std::sort(out.begin(), out.end());
  return out;
}

// readSfmDataFiles (TrainBoW.cpp:60-93)
void read_sfm_data_files(const std::string &d, std::vector<std::string> *out) {
  if (!is_dir(d)) return;
  const std::vector<std::string> names = sorted_entries(d);
  if (folder_name(d) == "matches") {
    for (const std::string &n : names)
      if (n == "sfm_data.json" && is_file(join(d, n))) out->push_back(join(d, n));
  } else {
    for (const std::string &n : names)
      if (is_dir(join(d, n))) read_sfm_data_files(join(d, n), out);
  }
}

// cv::RNG (include/sfmloc.h states it)
struct CvRng {
  uint64_t state = 0xFFFFFFFFull;
  uint32_t next() {
    state = (uint64_t)(uint32_t)state * 4164903690ull + (state >> 32);
    return (uint32_t)state;
  }
  float uniform01() { return (float)next() * 2.3283064365386962890625e-10f; }
};
uint32_t draw_index(uint32_t n, float r) {  // a float32 product, truncated, clamped below n
  const uint32_t k = (uint32_t)((float)n * r);
  return k < n ? k : n - 1;
}

// floats as Python's repr() writes them: the one copy shared with OpenMVG_BA's JSON writer
using sfmjson::py_repr;

// fileio.write_cv_yaml's layout: "%YAML:1.0", then per key an int, a quoted string or an f32 !!opencv-matrix on one line
struct YamlOut {
  std::string text = "%YAML:1.0\n";
  void num(const char *k, int v) { text += std::string(k) + ": " + std::to_string(v) + "\n"; }
  void str(const char *k, const char *v) { text += std::string(k) + ": \"" + v + "\"\n"; }
  void mat(const char *k, const float *d, int rows, int cols) {
    text += std::string(k) + ": !!opencv-matrix\n   rows: " + std::to_string(rows) + "\n   cols: " + std::to_string(cols) +
            "\n   dt: f\n   data: [ ";
    for (int i = 0; i < rows * cols; ++i) {
      if (i) text += ", ";
      text += py_repr((double)d[i]);
    }
    text += " ]\n";
  }
  bool write(const std::string &path) const {
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) return false;
    const bool ok = fwrite(text.data(), 1, text.size(), f) == text.size();
    return fclose(f) == 0 && ok;
  }
};

// saveMatBin (FileUtils.cpp:43-75) of a [dim x 1] CV_64F matrix
bool write_mat_bin(const std::string &path, const std::vector<double> &v) {
  FILE *f = fopen(path.c_str(), "wb");
  if (!f) return false;
  const int32_t head[3] = {(int32_t)v.size(), 1, 6};
  bool ok = fwrite(head, sizeof head, 1, f) == 1 && fwrite(v.data(), sizeof(double), v.size(), f) == v.size();
  return fclose(f) == 0 && ok;
}

bool read_bgr(const std::string &path, std::vector<uint8_t> *img, int32_t *w, int32_t *h) {
  if (sfmloc_image_read(path.c_str(), 1, nullptr, 0, w, h) != SFMLOC_OK) return false;
  img->resize((size_t)*w * *h * 3);
  return sfmloc_image_read(path.c_str(), 1, img->data(), img->size(), w, h) == SFMLOC_OK;
}

int fail(const char *what) {
  fprintf(stderr, "%s: %s\n", what, sfmloc_last_error());
  return 1;
}

struct View {
  std::string image, bow;
};

// getRandomTrainFeatures (TrainBoW.cpp:95-131) into the trainer's sample; only the last decoded image is kept
int random_train_features(sfmloc_bowtrain *tr, const std::vector<View> &views, int num, int per_image) {
  CvRng rng;
  if (sfmloc_bowtrain_reset(tr)) return fail("sfmloc_bowtrain_reset");
  std::vector<uint8_t> img;
  int32_t w = 0, h = 0;
  bool have = false;
  uint32_t last = UINT32_MAX;
  for (int i = 0; i < num / per_image; ++i) {
    const uint32_t k = draw_index((uint32_t)views.size(), rng.uniform01());
    if (k != last) {
      have = read_bgr(views[k].image, &img, &w, &h);
      last = k;
    }
    if (sfmloc_bowtrain_add_image(tr, have ? img.data() : nullptr, have ? w : 0, have ? h : 0, 3, per_image, &rng.state))
      return fail("sfmloc_bowtrain_add_image");
  }
  return 0;
}

// calcDenseLocalFeature -> calcPcaProject -> calcBoF -> saveMatBin for every view (TrainBoW.cpp:238-272)
int write_bow_vectors(const sfmloc_bof_desc &model, bool batched, const std::vector<View> &views, int device) {
  std::map<std::pair<int, int>, std::vector<sfmloc_imgbow *>> pools;
  std::map<std::pair<int, int>, std::vector<std::pair<std::vector<uint8_t>, std::string>>> pending;
  int rc = 0;
  auto flush = [&](const std::pair<int, int> &key) -> int {
    auto &items = pending[key];
    if (items.empty()) return 0;
    std::vector<sfmloc_imgbow *> &exs = pools[key];
    const int dim = sfmloc_imgbow_dim(exs[0]);
    std::vector<double> vec(dim);
    if (batched) {
      std::vector<const uint8_t *> imgs;
      for (auto &it : items) imgs.push_back(it.first.data());
      if (sfmloc_imgbow_compute_batch(exs.data(), imgs.data(), (uint32_t)items.size())) return fail("sfmloc_imgbow_compute_batch");
      for (size_t i = 0; i < items.size(); ++i) {
        if (sfmloc_imgbow_vector_read(exs[i], vec.data())) return fail("sfmloc_imgbow_vector_read");
        if (!write_mat_bin(items[i].second, vec)) { fprintf(stderr, "cannot write %s\n", items[i].second.c_str()); return 1; }
      }
    } else {  // (61-dimensional words do not fit the batched assignment's LDS layout: one chain per image)
      for (auto &it : items) {
        if (sfmloc_imgbow_compute(exs[0], it.first.data(), nullptr, vec.data())) return fail("sfmloc_imgbow_compute");
        if (!write_mat_bin(it.second, vec)) { fprintf(stderr, "cannot write %s\n", it.second.c_str()); return 1; }
      }
    }
    items.clear();
    return 0;
  };
  for (const View &v : views) {
    std::vector<uint8_t> img;
    int32_t w = 0, h = 0;
    if (!read_bgr(v.image, &img, &w, &h)) {
      rc = fail(("cannot read " + v.image).c_str());
      break;
    }
    const std::pair<int, int> key(w, h);
    if (!pools.count(key)) {
      std::vector<sfmloc_imgbow *> exs(kBatch, nullptr);
      for (uint32_t i = 0; i < kBatch && !rc; ++i)
        if (sfmloc_imgbow_create(&model, device, w, h, 3, &exs[i])) rc = fail("sfmloc_imgbow_create");
      pools[key] = exs;
      if (rc) break;
    }
    pending[key].emplace_back(std::move(img), v.bow);
    if (pending[key].size() == kBatch && (rc = flush(key))) break;
  }
  for (auto &kv : pending)
    if (!rc) rc = flush(kv.first);
  for (auto &kv : pools)
    for (sfmloc_imgbow *e : kv.second)
      if (e) sfmloc_imgbow_destroy(e);
  return rc;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc >= 2 && strcmp(argv[1], "--format-floats") == 0) {
    for (int i = 2; i < argc; ++i) printf("%s\n", py_repr((double)strtof(argv[i], nullptr)).c_str());
    return 0;
  }
  std::vector<std::string> pos;
  std::string pca_file;
  int device = 0;
  bool help = false;
  for (int i = 1; i < argc; ++i) {  // cv::CommandLineParser syntax: positional, -k=v / --key=v
    std::string a = argv[i];
    if (a.size() > 1 && a[0] == '-') {
      const size_t s = a.find_first_not_of('-');
      const size_t eq = a.find('=');
      const std::string k = a.substr(s, eq == std::string::npos ? std::string::npos : eq - s);
      const std::string v = eq == std::string::npos ? "true" : a.substr(eq + 1);
      if (k == "p" || k == "pcaFile") pca_file = v;
      else if (k == "device") device = atoi(v.c_str());
      else if (k == "h" || k == "help") help = true;
    } else {
      pos.push_back(a);
    }
  }
  if (pos.size() < 2 || help || pos[0].empty() || pos[1].empty()) {
    printf("usage: TrainBoW <inputDir> <bowFile> [-p=pcaFile] [--device=0]\n");
    return 1;
  }
  const std::string input_dir = pos[0], bow_file = pos[1];
  std::vector<std::string> sfm_files;
  read_sfm_data_files(input_dir, &sfm_files);
  printf("number of sfm data files found : %zu\n", sfm_files.size());
  std::vector<View> views;
  for (const std::string &f : sfm_files) {
    sfmloc_view_list *vl = nullptr;
    uint32_t n = 0;
    if (sfmloc_view_list_open(f.c_str(), &vl, &n)) return fail(("Cannot load " + f).c_str());
    for (uint32_t k = 0; k < n; ++k) {
      uint32_t id, w, h;
      const char *path = nullptr;
      if (sfmloc_view_list_get(vl, k, &id, &w, &h, &path)) {
        sfmloc_view_list_close(vl);
        return fail("sfmloc_view_list_get");
      }
      views.push_back({path, join(dirname_of(f), basename_part(path) + ".bow")});
    }
    sfmloc_view_list_close(vl);
  }
  printf("number of image files found : %zu\n", views.size());
  if (views.empty()) { fprintf(stderr, "no map images below %s\n", input_dir.c_str()); return 1; }

  sfmloc_bowtrain *tr = nullptr;
  if (sfmloc_bowtrain_create(device, 61, std::max(kPcaTrainFeatureNum, kKmeansTrainFeatureNum), &tr))
    return fail("sfmloc_bowtrain_create");
  int rc = 0;
  std::vector<float> mean(61), evec(61 * 61), evals(61);
  if (!pca_file.empty()) {
    rc = random_train_features(tr, views, kPcaTrainFeatureNum, kPcaPerImage);
    if (!rc && sfmloc_bowtrain_pca(tr, mean.data(), evec.data(), evals.data())) rc = fail("sfmloc_bowtrain_pca");
    if (!rc) {
      YamlOut y;  // PcaWrapper::write (PcaWrapper.cpp:53-58)
      y.num("DimPCA", kPcaDim);
      y.mat("EigenVectorsPCA", evec.data(), 61, 61);
      y.mat("EigenValuesPCA", evals.data(), 61, 1);
      y.mat("MeanPCA", mean.data(), 1, 61);
      if (!y.write(pca_file)) {
        fprintf(stderr, "cannot write %s\n", pca_file.c_str());
        rc = 1;
      }
    }
    // (the reference reloads the model from the file; the shortest round-trip text reads back as the same floats)
    sfmloc_bof_desc p;
    memset(&p, 0, sizeof p);
    p.in_dim = 61;
    p.n_pca = kPcaDim;
    p.pca_mean = mean.data();
    p.pca_eigvec = evec.data();
    p.pca_eigval = evals.data();
    if (!rc && sfmloc_bowtrain_project(tr, &p)) rc = fail("sfmloc_bowtrain_project");
  } else {
    rc = random_train_features(tr, views, kKmeansTrainFeatureNum, kKmeansPerImage);
  }
  uint32_t n = 0, dim = 0;
  if (!rc && sfmloc_bowtrain_size(tr, &n, &dim)) rc = fail("sfmloc_bowtrain_size");
  if (!rc) printf("Training feature matrix size is (%u x %u)\n", n, dim);
  std::vector<float> centers((size_t)std::min<uint32_t>(kK, n) * dim);
  double compactness = 0;
  if (!rc && sfmloc_bowtrain_kmeans(tr, kK, kKmeansAttempts, kKmeansIteration, FLT_EPSILON, kKmeansSeed, centers.data(),
                                    nullptr, nullptr, &compactness, nullptr))
    rc = fail("sfmloc_bowtrain_kmeans");
  sfmloc_bowtrain_destroy(tr);
  if (rc) return rc;
  printf("End train kmeans. Number of cluster is %d\n", kK);
  YamlOut y;  // BoFSpatialPyramids::write (BoFSpatialPyramids.cpp:57-68)
  y.num("K", kK);
  y.num("ResizedImageSize", kResized);
  y.str("NormBofFeatureType", "L1");
  y.num("UseSpatialPyramid", 1);
  y.num("PyramidLevel", kPyramidLevel);
  y.mat("Centers", centers.data(), (int)(centers.size() / dim), (int)dim);
  if (!y.write(bow_file)) { fprintf(stderr, "cannot write %s\n", bow_file.c_str()); return 1; }
  sfmloc_bof_desc model;
  memset(&model, 0, sizeof model);
  model.K = (int)(centers.size() / dim);
  model.in_dim = 61;
  model.centers = centers.data();
  model.resized_image_size = kResized;
  model.use_spatial_pyramid = 1;
  model.pyramid_level = kPyramidLevel;
  model.norm_type = 2;  // L1
  if (!pca_file.empty()) {
    model.n_pca = kPcaDim;
    model.pca_mean = mean.data();
    model.pca_eigvec = evec.data();
    model.pca_eigval = evals.data();
  }
  rc = write_bow_vectors(model, !pca_file.empty(), views, device);
  if (!rc) printf("End calculate BoF feature for all images.\n");
  return rc;
}
