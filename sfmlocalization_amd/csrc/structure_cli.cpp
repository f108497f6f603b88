// openMVG_main_ComputeStructureFromKnownPoses as a C++ host program over the C ABI (plain g++):
//
//   openMVG_main_ComputeStructureFromKnownPoses -i <sfm_data.json> -m <matchDir> [-f <match file = matches.f.txt>]
//                                               -o <out sfm_data.json> [-r <residual px = 4.0>] [-a <min angle deg = 2.0>]
//                                               [-b] [--blind] [--register] [--device=0]
//
// The same program as sfmlocalization_amd/structure.py, the same lines on stdout and the same bytes: the structure of a
// map rebuilt from its poses and the pairwise matches (the last stage of openMVG_main_GlobalSfM).  The input's own
// structure is ignored; <matchDir>/<stem>.feat of every view gives its features, the match file the pairs; views without
// a pose are masked out of the tracks (sfmloc_tracks_build); then, on one resident sfmloc_sfm: sfmloc_sfm_triangulate,
// sfmloc_sfm_clean(r, a, 0) and, with -b, the structure adjustment followed by a second cleanup.  The output is the input
// document with `structure` replaced (the kept landmarks, keys 0, 1, 2, ... in track order, every kept observation with
// its id_feat and the .feat pixel) and control_points [].  --register: the tracks over all views, sfmloc_sfm_register (one
// round per call, at most 16) and a cleanup after the first cleanup, and `extrinsics` written from the handle.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_doc.h"
#include "sfm_files.h"
#include "sfm_json.h"

using namespace sfmfiles;
using sfmdoc::Doc;
using sfmdoc::make_int;
using sfmdoc::set_key;
using sfmjson::Value;

namespace {

const char *kName = "openMVG_main_ComputeStructureFromKnownPoses";

void usage() {
  fprintf(stderr,
          "Usage: %s\n"
          "[-i|--input_file] path to a SfM_Data scene\n"
          "[-m|--match_dir] path to the features and descriptors that corresponds to the provided SfM_Data scene\n"
          "[-o|--output_file] file where the output data will be stored\n"
          "\n[Optional]\n"
          "[-f|--match_file] path to a matches file (default: matches.f.txt in the match directory)\n"
          "[-b|--bundle_adjustment] (switch) perform a bundle adjustment on the scene (structure only)\n"
          "[-r|--residual_threshold] maximal pixels reprojection error that will be considered for triangulations (4.0)\n"
          "[-a|--min_angle] minimal triangulation angle in degrees (2.0)\n"
          "[--blind] (switch) triangulate every track from all its views, no robust rounds\n"
          "[--register] (switch) resect the views without a pose against the structure and extend it (the tracks are\n"
          "             built over all views: a wrong match of an unposed view can drop a track the masked build keeps)\n",
          kName);
}

std::string g(double v) {
  char buf[40];
  snprintf(buf, sizeof buf, "%g", v);
  return buf;
}

}  // namespace

int main(int argc, char **argv) {
  std::string in, match_dir, out_path, match_file = "matches.f.txt", r_txt = "4.0", a_txt = "2.0";
  bool adjust = false, blind = false, reg = false;
  int device = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    std::string *dst = nullptr;
    if (a == "-i" || a == "--input_file") dst = &in;
    else if (a == "-m" || a == "--match_dir") dst = &match_dir;
    else if (a == "-o" || a == "--output_file") dst = &out_path;
    else if (a == "-f" || a == "--match_file") dst = &match_file;
    else if (a == "-r" || a == "--residual_threshold") dst = &r_txt;
    else if (a == "-a" || a == "--min_angle") dst = &a_txt;
    if (dst) {
      if (i + 1 >= argc) {
        usage();
        return 1;
      }
      *dst = argv[++i];
    } else if (a == "-b" || a == "--bundle_adjustment") {
      adjust = true;
    } else if (a == "--blind") {
      blind = true;
    } else if (a == "--register") {
      reg = true;
    } else if (a.rfind("--device=", 0) == 0) {
      device = atoi(a.c_str() + 9);
    } else {
      usage();
      return 1;
    }
  }
  char *e1 = nullptr, *e2 = nullptr;
  const double residual_px = strtod(r_txt.c_str(), &e1), angle_deg = strtod(a_txt.c_str(), &e2);
  if (r_txt.empty() || a_txt.empty() || *e1 || *e2 || in.empty() || match_dir.empty() || out_path.empty()) {
    usage();
    return 1;
  }
  Doc d;
  std::string err;
  if (!sfmdoc::load(in, true, &d, &err)) {  // the input's own structure: ignored
    fprintf(stderr, "\nThe input SfM_Data file \"%s\" cannot be read. (%s)\n", in.c_str(), err.c_str());
    return 1;
  }
  const uint32_t n_views = (uint32_t)d.view_id.size();
  const Value *views = d.root.get("views");
  std::vector<std::vector<float>> feats(n_views);
  std::vector<uint64_t> view_off(1, 0);
  for (uint32_t k = 0; k < n_views; ++k) {
    const Value *data = sfmdoc::ptr_data(views->a[k].get("value"));
    const Value *fn = data ? data->get("filename") : nullptr;
    const std::string path = join(match_dir, stem_of((fn && fn->kind == Value::Str) ? fn->s : std::string()) + ".feat");
    if (!read_feat(path, &feats[k])) {
      fprintf(stderr, "\nInvalid features. (%s cannot be read)\n", path.c_str());
      return 1;
    }
    view_off.push_back(view_off.back() + feats[k].size() / 2);
  }
  std::map<uint32_t, uint32_t> view_index;
  for (uint32_t k = 0; k < n_views; ++k) view_index[d.view_id[k]] = k;
  PairList pl;
  const std::string mpath = join(match_dir, match_file);
  if (!read_matches(mpath, view_index, &pl, &err)) {
    fprintf(stderr, "\nInvalid matches file. (%s: %s)\n", mpath.c_str(), err.c_str());
    return 1;
  }
  std::vector<uint8_t> view_use(n_views);
  uint32_t n_use = 0;
  for (uint32_t k = 0; k < n_views; ++k) n_use += (view_use[k] = d.pose_valid[d.view_pose[k]] ? 1 : 0);
  printf("#views: %u, with a pose: %u; #pairs: %zu, #matches: %zu\n", n_views, n_use, pl.pairs.size() / 2, pl.mi.size());
  fflush(stdout);

  sfmloc_tracks *trk = nullptr;
  sfmloc_sfm *h = nullptr;
  const auto fail = [&]() {
    fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
    sfmloc_sfm_destroy(h);
    sfmloc_tracks_destroy(trk);
    return 1;
  };
  if (sfmloc_tracks_build(device, view_off.data(), n_views, reg ? nullptr : view_use.data(), pl.pairs.data(), (uint32_t)(pl.pairs.size() / 2),
                          pl.offsets.data(), pl.mi.data(), pl.mj.data(), 2, &trk))
    return fail();
  uint64_t tc[4];
  sfmloc_tracks_counts(trk, tc);
  printf("Tracks: %llu components, %llu dropped for conflict, %llu dropped for length, %llu kept\n",
         (unsigned long long)tc[0], (unsigned long long)tc[1], (unsigned long long)tc[2], (unsigned long long)tc[3]);
  fflush(stdout);
  const size_t n_lm = (size_t)tc[3];
  d.obs_off.assign(n_lm + 1, 0);
  sfmloc_tracks_read(trk, d.obs_off.data(), nullptr, nullptr);
  const size_t n_obs = (size_t)d.obs_off[n_lm];
  std::vector<uint32_t> feat(n_obs ? n_obs : 1);
  d.obs_view.assign(n_obs ? n_obs : 1, 0);
  sfmloc_tracks_read(trk, nullptr, d.obs_view.data(), feat.data());
  sfmloc_tracks_destroy(trk);
  trk = nullptr;
  d.lm_id.resize(n_lm);
  for (size_t l = 0; l < n_lm; ++l) d.lm_id[l] = (uint32_t)l;
  d.lm_X.assign(3 * n_lm, 0.0);
  d.obs_x.assign(2 * (n_obs ? n_obs : 1), 0.0);
  for (size_t o = 0; o < n_obs; ++o) {
    d.obs_x[2 * o] = (double)feats[d.obs_view[o]][2 * (size_t)feat[o]];
    d.obs_x[2 * o + 1] = (double)feats[d.obs_view[o]][2 * (size_t)feat[o] + 1];
  }
  sfmloc_sfm_desc desc;
  sfmdoc::fill_desc(d, &desc);
  sfmloc_params params;
  sfmloc_sfm_default_params(&params);
  params.device = device;
  if (sfmloc_sfm_create(&desc, &params, &h)) return fail();
  sfmloc_triangulate_options opt;
  sfmloc_triangulate_default_options(&opt);
  opt.mode = blind ? SFMLOC_TRI_BLIND : SFMLOC_TRI_ROBUST;
  opt.residual_px = residual_px;
  sfmloc_triangulate_report rep;
  if (sfmloc_sfm_triangulate(h, &opt, &rep)) return fail();
  printf("Triangulation: %llu tracks, %llu kept; failed: %llu too few posed observations, %llu no valid hypothesis, "
         "%llu too few inliers; %llu of %llu observations kept; %llu rounds\n",
         (unsigned long long)rep.landmarks_in, (unsigned long long)rep.landmarks_kept, (unsigned long long)rep.failed_posed,
         (unsigned long long)rep.failed_hypothesis, (unsigned long long)rep.failed_inliers,
         (unsigned long long)rep.obs_kept, (unsigned long long)rep.obs_in, (unsigned long long)rep.rounds);
  fflush(stdout);
  const auto clean = [&]() {
    uint64_t c[4];
    if (sfmloc_sfm_clean(h, residual_px, angle_deg, 0, c)) return false;
    printf("Number of points before cleanup : %llu\nNumber of points residual error : %llu\n"
           "Number of points angle error : %llu\nNumber of points after cleanup : %llu\n",
           (unsigned long long)c[0], (unsigned long long)c[1], (unsigned long long)c[2], (unsigned long long)c[3]);
    fflush(stdout);
    return true;
  };
  if (!clean()) return fail();
  if (reg) {
    unsigned long long total[5] = {0, 0, 0, 0, 0};
    sfmloc_register_options ro;
    sfmloc_register_default_options(&ro);
    const uint32_t max_rounds = ro.max_rounds;
    ro.max_rounds = 1;  // (one round per call: the handle numbers them on)
    ro.residual_px = residual_px;
    for (uint32_t i = 0; i < max_rounds; ++i) {
      sfmloc_register_report rr;
      if (sfmloc_sfm_register(h, &ro, &rr)) return fail();
      if (rr.rounds == 0) break;
      printf("Registration round %llu: %u views tried, %u registered, %llu observations extended, %llu of %llu landmarks "
             "added\n",
             total[0], rr.views_tried, rr.views_registered, (unsigned long long)rr.obs_extended,
             (unsigned long long)rr.landmarks_added, (unsigned long long)rr.landmarks_tried);
      fflush(stdout);
      total[0] += 1;
      total[1] += rr.views_tried;
      total[2] += rr.views_registered;
      total[3] += rr.obs_extended;
      total[4] += rr.landmarks_added;
      if (rr.views_registered == 0) break;
    }
    printf("Registration: %llu rounds, %llu views registered in %llu tries, %llu observations extended, %llu landmarks "
           "added\n",
           total[0], total[2], total[1], total[3], total[4]);
    fflush(stdout);
    if (!clean()) return fail();
  }
  if (adjust) {
    sfmloc_ba_report ba;
    if (sfmloc_sfm_adjust(h, SFMLOC_BA_STRUCTURE, &ba)) return fail();
    printf("Bundle adjustment over structure: %u landmarks, cost %s -> %s\n", ba.n_blocks, g(ba.cost_initial).c_str(),
           g(ba.cost_final).c_str());
    fflush(stdout);
    if (!clean()) return fail();
  }
  std::vector<uint8_t> obs_keep(n_obs ? n_obs : 1), lm_keep(n_lm ? n_lm : 1);
  std::vector<double> X(3 * (n_lm ? n_lm : 1));
  const size_t n_poses = d.pose_id.size();
  std::vector<uint8_t> pose_valid(n_poses ? n_poses : 1);
  std::vector<double> pose_R(9 * (n_poses ? n_poses : 1)), pose_C(3 * (n_poses ? n_poses : 1));
  if (sfmloc_sfm_read(h, pose_valid.data(), pose_R.data(), pose_C.data(), obs_keep.data(), lm_keep.data()) ||
      sfmloc_sfm_read_structure(h, X.data()))
    return fail();
  sfmloc_sfm_destroy(h);
  h = nullptr;
  Value st = Value::make_arr();
  for (size_t l = 0; l < n_lm; ++l) {
    if (!lm_keep[l]) continue;
    Value obs = Value::make_arr();
    for (uint64_t o = d.obs_off[l]; o < d.obs_off[l + 1]; ++o) {
      if (!obs_keep[o]) continue;
      Value x = Value::make_arr();
      x.a.push_back(Value::make_float(d.obs_x[2 * o]));
      x.a.push_back(Value::make_float(d.obs_x[2 * o + 1]));
      Value v;
      v.kind = Value::Obj;
      v.o.emplace_back("id_feat", make_int(feat[o]));
      v.o.emplace_back("x", x);
      Value e;
      e.kind = Value::Obj;
      e.o.emplace_back("key", make_int(d.view_id[d.obs_view[o]]));
      e.o.emplace_back("value", v);
      obs.a.push_back(e);
    }
    Value xs = Value::make_arr();
    for (int j = 0; j < 3; ++j) xs.a.push_back(Value::make_float(X[3 * l + j]));
    Value val;
    val.kind = Value::Obj;
    val.o.emplace_back("X", xs);
    val.o.emplace_back("observations", obs);
    Value e;
    e.kind = Value::Obj;
    e.o.emplace_back("key", make_int(st.a.size()));
    e.o.emplace_back("value", val);
    st.a.push_back(e);
  }
  printf("#landmark found: %zu\n", st.a.size());
  fflush(stdout);
  // (the document is written from a copy of the parsed input: `structure` was emptied before the arrays were built, so
  // the key keeps the place it has in the input, as Python's dict does)
  Value outd = d.root;
  set_key(&outd, "structure", st);
  if (reg) {  // every valid pose of the handle, ascending pose id
    Value ext = Value::make_arr();
    for (size_t p = 0; p < n_poses; ++p) {
      if (!pose_valid[p]) continue;
      Value rot = Value::make_arr();
      for (int i = 0; i < 3; ++i) {
        Value row = Value::make_arr();
        for (int j = 0; j < 3; ++j) row.a.push_back(Value::make_float(pose_R[9 * p + 3 * i + j]));
        rot.a.push_back(row);
      }
      Value cen = Value::make_arr();
      for (int j = 0; j < 3; ++j) cen.a.push_back(Value::make_float(pose_C[3 * p + j]));
      Value v;
      v.kind = Value::Obj;
      v.o.emplace_back("rotation", rot);
      v.o.emplace_back("center", cen);
      Value e;
      e.kind = Value::Obj;
      e.o.emplace_back("key", make_int(d.pose_id[p]));
      e.o.emplace_back("value", v);
      ext.a.push_back(e);
    }
    set_key(&outd, "extrinsics", ext);
  }
  set_key(&outd, "control_points", Value::make_arr());
  std::string out;
  sfmjson::dump(outd, &out);
  if (!sfmjson::write_file(out_path.c_str(), out)) {
    fprintf(stderr, "%s: %s cannot be written\n", kName, out_path.c_str());
    return 1;
  }
  return 0;
}
