// openMVG_main_ComputeSfM_DataColor as a C++ host program over the C ABI (plain g++):
//
//   openMVG_main_ComputeSfM_DataColor -i <sfm_data.json> -o <out.ply> [--device=0]
//
// The same program as sfmlocalization_amd/colorize.py, and the same bytes.  The colouring plan (which view every
// landmark takes its colour from) is computed on the device (sfmloc_sfm_color_plan); the host then reads the chosen
// views' images in plan order (sfmloc_image_read, colour) and samples the pixel at ((int)y, (int)x) of the landmark's
// observation in that view -- a few hundred pixels per frame, so no frame is uploaded.  Divergences from OpenMVG 1.1:
// a coordinate outside the image is clamped to the border (the reference reads out of bounds; a NaN reads column or
// row 0); an image that cannot be read ends the run with status 1 and the file's name, and nothing is written; a
// landmark without observations is written black.  The PLY is plyHelper::exportToPly's: the landmarks in ascending
// id with their colours, then the centre of every view that has a pose in green; numbers as %g separated by single
// spaces (Eigen pads the columns of a row to a common width; every consumer in the reference splits on whitespace).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_doc.h"
#include "sfm_files.h"
#include "sfm_json.h"

using sfmdoc::Doc;
using sfmfiles::join;
using sfmjson::Value;

namespace {

const char *kName = "openMVG_main_ComputeSfM_DataColor";

void usage() {
  fprintf(stderr,
          "Usage: %s\n"
          "[-i|--input_file] path to the input SfM_Data scene\n"
          "[-o|--output_file] path to the output PLY file\n",
          kName);
}

// (int)c clamped to [0, n - 1]; the cast truncates toward zero, a NaN gives 0
int64_t pixel(double c, int32_t n) {
  if (!(c > 0.0)) return 0;
  if (c >= (double)n) return n - 1;
  return (int64_t)c;
}

std::string num(double v) {
  if (std::isnan(v)) return "nan";
  char buf[40];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

}  // namespace

int main(int argc, char **argv) {
  std::string in, out_path;
  int device = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    std::string *dst = nullptr;
    if (a == "-i" || a == "--input_file") dst = &in;
    else if (a == "-o" || a == "--output_file") dst = &out_path;
    if (dst) {
      if (i + 1 >= argc) {
        usage();
        return 1;
      }
      *dst = argv[++i];
    } else if (a.rfind("--input_file=", 0) == 0) {
      in = a.substr(13);
    } else if (a.rfind("--output_file=", 0) == 0) {
      out_path = a.substr(14);
    } else if (a.rfind("--device=", 0) == 0) {
      device = atoi(a.c_str() + 9);
    } else {
      usage();
      return 1;
    }
  }
  if (in.empty() || out_path.empty()) {
    usage();
    return 1;
  }
  Doc d;
  std::string err;
  if (!sfmdoc::load(in, false, &d, &err)) {
    fprintf(stderr, "\nThe input SfM_Data file \"%s\" cannot be read. (%s)\n", in.c_str(), err.c_str());
    return 1;
  }
  const size_t n_lm = d.lm_id.size(), n_views = d.view_id.size();
  std::vector<uint32_t> order(n_views ? n_views : 1), lm_iter(n_lm ? n_lm : 1, 0xFFFFFFFFu);
  std::vector<uint64_t> lm_obs(n_lm ? n_lm : 1, 0);
  uint32_t n_order = 0;
  if (!d.obs_view.empty()) {  // (no observations: nothing to plan, no device call)
    sfmloc_sfm_desc desc;
    sfmdoc::fill_desc(d, &desc);
    sfmloc_params params;
    sfmloc_sfm_default_params(&params);
    params.device = device;
    sfmloc_sfm *h = nullptr;
    int rc = sfmloc_sfm_create(&desc, &params, &h);
    if (rc == 0) rc = sfmloc_sfm_color_plan(h, order.data(), &n_order, lm_iter.data(), lm_obs.data());
    sfmloc_sfm_destroy(h);
    if (rc) {
      fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
      return 1;
    }
  }
  // the landmarks of each iteration, ascending (a counting sort by iteration)
  std::vector<size_t> first(n_order + 1, 0);
  for (size_t l = 0; l < n_lm; ++l)
    if (lm_iter[l] < n_order) ++first[lm_iter[l] + 1];
  for (uint32_t k = 0; k < n_order; ++k) first[k + 1] += first[k];
  std::vector<uint32_t> by_iter(first[n_order] ? first[n_order] : 1);
  {
    std::vector<size_t> at(first.begin(), first.end() - 1);
    for (size_t l = 0; l < n_lm; ++l)
      if (lm_iter[l] < n_order) by_iter[at[lm_iter[l]]++] = (uint32_t)l;
  }
  const Value *rp = d.root.get("root_path");
  const std::string root = (rp && rp->kind == Value::Str) ? rp->s : std::string();
  const Value *views = d.root.get("views");
  std::vector<uint8_t> rgb(3 * (n_lm ? n_lm : 1), 0), img;
  for (uint32_t k = 0; k < n_order; ++k) {
    const Value *data = views->a[order[k]].get("value")->get("ptr_wrapper")->get("data");
    const Value *fn = data->get("filename");
    const std::string path = join(root, (fn && fn->kind == Value::Str) ? fn->s : std::string());
    int32_t w = 0, h = 0;
    int rc = sfmloc_image_read(path.c_str(), 1, nullptr, 0, &w, &h);
    if (rc == 0 && w > 0 && h > 0) {
      img.resize((size_t)w * h * 3);
      rc = sfmloc_image_read(path.c_str(), 1, img.data(), img.size(), &w, &h);
    } else if (rc == 0) {
      rc = SFMLOC_EIO;
    }
    if (rc) {
      fprintf(stderr, "%s: cannot read the image %s\n", kName, path.c_str());
      return 1;
    }
    for (size_t i = first[k]; i < first[k + 1]; ++i) {
      const uint32_t l = by_iter[i];
      const int64_t x = pixel(d.obs_x[2 * lm_obs[l]], w), y = pixel(d.obs_x[2 * lm_obs[l] + 1], h);
      const uint8_t *p = &img[((size_t)y * w + x) * 3];  // B G R
      rgb[3 * l] = p[2];
      rgb[3 * l + 1] = p[1];
      rgb[3 * l + 2] = p[0];
    }
  }
  std::vector<uint32_t> cams;
  for (size_t v = 0; v < n_views; ++v)
    if (d.pose_valid[d.view_pose[v]]) cams.push_back(d.view_pose[v]);
  std::string text = "ply\nformat ascii 1.0\nelement vertex " + std::to_string(n_lm + cams.size()) +
                     "\nproperty float x\nproperty float y\nproperty float z\nproperty uchar red\n"
                     "property uchar green\nproperty uchar blue\nend_header\n";
  for (size_t l = 0; l < n_lm; ++l) {
    text += num(d.lm_X[3 * l]) + " " + num(d.lm_X[3 * l + 1]) + " " + num(d.lm_X[3 * l + 2]) + " " +
            std::to_string(rgb[3 * l]) + " " + std::to_string(rgb[3 * l + 1]) + " " + std::to_string(rgb[3 * l + 2]) + "\n";
  }
  for (uint32_t p : cams)
    text += num(d.pose_C[3 * p]) + " " + num(d.pose_C[3 * p + 1]) + " " + num(d.pose_C[3 * p + 2]) + " 0 255 0\n";
  if (!sfmjson::write_file(out_path.c_str(), text)) {
    fprintf(stderr, "%s: %s cannot be written\n", kName, out_path.c_str());
    return 1;
  }
  return 0;
}
