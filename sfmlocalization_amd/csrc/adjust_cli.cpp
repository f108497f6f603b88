// OpenMVG_BA (OpenMVG_BA/src/adjust_sfm_data.cpp) as a C++ host program over the C ABI (plain g++):
//
//   OpenMVG_BA <sfm_data> <sfm_data_out> [-c=...] [-r=0|1] [-j=0|1] [--device=0]
//
// The same program as sfmlocalization_amd/adjust.py, and the same bytes: every view with more than 10 observations is
// re-resected on the device (sfmloc_sfm_resect), <folder of sfm_data>/sfm_data_b4bd.json is written with the new poses
// and the structure untouched (:152-155), the structure is cleaned (sfmloc_sfm_clean: residual 4 px, angle 2 degrees,
// unstable poses with -r=1; :245-260) and the result is written to sfm_data_out (which may be sfm_data itself: the
// merge loop calls it in place).  Both files are what Python's json.dump writes for the document: views, intrinsics,
// root_path and key order as in the input, extrinsics in ascending pose id, control_points [] (Save without
// CONTROL_POINTS).
//
// -c=item,item,... (:158-244): after the re-resection and sfm_data_b4bd.json every item runs in order -- s adjusts the
// structure alone, r / t / rt the rotations / translations / both alone (sfmloc_sfm_adjust), a c in the item cleans
// afterwards and prints the four counts; an item with none of r t i s adjusts nothing.  With a non-empty -c there is no
// final cleanup of its own (the reference cleans in the else branch only) and the output holds the adjusted poses and X.
// The joint commands (s with r or t, anything with i) are not supported yet: every item is checked before anything is
// opened, one refused item ends the run with status 1 and nothing written.
//
// -j=1 (--joint=1, in any position) opts in to the joint adjustment: no item is refused, an item that would be goes to
// sfmloc_sfm_adjust_joint with the default options (one Levenberg-Marquardt problem over everything the item names), a
// separable item still goes to sfmloc_sfm_adjust (-c=rt,sc -j=1 gives the bytes of -c=rt,sc).  An intrinsic whose bits
// changed is written from the arrays (focal_length, principal_point, disto_k3); sfm_data_b4bd.json keeps the input's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_doc.h"
#include "sfm_json.h"

using sfmdoc::Doc;
using sfmdoc::set_key;
using sfmjson::Value;

namespace {

const double kResidualPx = 4.0, kAngleDeg = 2.0;  // STRUCTURE_CLEANUP_RESIDUAL_ERROR / _ANGLE_ERROR (:40-41)

void usage() {
  fprintf(stderr,
          "Execute bundle adjustment for sfm_data.json\n"
          "Usage: OpenMVG_BA [params] sfm_data sfm_data_out\n"
          "\t-c, --command\n\t\tCommand for order of bundle adjustment (BD) [default=no BD] [options:r = rotation, "
          "t = translation, s = structure, c = clean]. Usage example: c=r,tc,s means BD with rotation only, then BD with "
          "translation follow by cleaning, then BD with structure. Not supported yet: i (intrinsic), and s together "
          "with r or t.\n"
          "\t-r, --rm_unstable (value:0)\n\t\tRemove unstable pose and observation\n"
          "\t-j, --joint (value:0)\n\t\tWith 1, run the items that are not supported yet (i, and s together with r or t) as "
          "one joint bundle adjustment\n");
}

// extrinsics: the valid poses in ascending id; an input pose untouched keeps its JSON value as it was
Value extrinsics(const Doc &d, const std::vector<uint8_t> &valid, const std::vector<double> &R,
                 const std::vector<double> &C, const std::vector<uint8_t> &replaced) {
  Value a = Value::make_arr();
  for (size_t p = 0; p < d.pose_id.size(); ++p) {
    if (!valid[p]) continue;
    Value e;
    e.kind = Value::Obj;
    e.o.emplace_back("key", sfmdoc::make_int(d.pose_id[p]));
    if (!replaced[p] && d.pose_src[p]) {
      e.o.emplace_back("value", *d.pose_src[p]);
    } else {
      Value v;
      v.kind = Value::Obj;
      Value rot = Value::make_arr();
      for (int i = 0; i < 3; ++i) {
        Value row = Value::make_arr();
        for (int j = 0; j < 3; ++j) row.a.push_back(Value::make_float(R[9 * p + 3 * i + j]));
        rot.a.push_back(row);
      }
      Value cen = Value::make_arr();
      for (int j = 0; j < 3; ++j) cen.a.push_back(Value::make_float(C[3 * p + j]));
      v.o.emplace_back("rotation", rot);
      v.o.emplace_back("center", cen);
      e.o.emplace_back("value", v);
    }
    a.a.push_back(e);
  }
  return a;
}

bool write_doc(const std::string &path, const Value &root) {
  std::string out;
  sfmjson::dump(root, &out);
  return sfmjson::write_file(path.c_str(), out);
}

std::string folder_of(const std::string &p) {
  const size_t k = p.find_last_of('/');
  return k == std::string::npos ? std::string() : p.substr(0, k + 1);
}

// -c split on commas as the reference's getline loop splits it (no item after a trailing comma)
std::vector<std::string> command_items(const std::string &command) {
  std::vector<std::string> items;
  size_t at = 0;
  while (at < command.size()) {
    const size_t k = command.find(',', at);
    if (k == std::string::npos) {
      items.push_back(command.substr(at));
      break;
    }
    items.push_back(command.substr(at, k - at));
    at = k + 1;
  }
  return items;
}

bool has(const std::string &item, char c) { return item.find(c) != std::string::npos; }

bool bits_differ(const double *a, const double *b, size_t n) { return memcmp(a, b, n * sizeof(double)) != 0; }

// an item the separable path refuses: structure with a pose part, or intrinsics
bool joint_item(const std::string &item) {
  return has(item, 'i') || (has(item, 's') && (has(item, 'r') || has(item, 't')));
}

// intrinsic i of the document (array order) from K = f, ppx, ppy, k1, k2, k3
void set_intrinsic(Value *root, size_t i, uint32_t type, const double *K) {
  Value *list = root->get("intrinsics");
  Value *val = list ? list->a[i].get("value") : nullptr;
  Value *pw = val ? val->get("ptr_wrapper") : nullptr;
  Value *data = pw ? pw->get("data") : nullptr;
  if (!data) return;
  Value *pin = type == 3 ? data->get("value0") : data;
  if (!pin) return;
  set_key(pin, "focal_length", Value::make_float(K[0]));
  Value pp = Value::make_arr();
  pp.a.push_back(Value::make_float(K[1]));
  pp.a.push_back(Value::make_float(K[2]));
  set_key(pin, "principal_point", pp);
  if (type == 3) {
    Value k3 = Value::make_arr();
    for (int j = 3; j < 6; ++j) k3.a.push_back(Value::make_float(K[j]));
    set_key(data, "disto_k3", k3);
  }
}

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    usage();
    return 1;
  }
  std::vector<std::string> pos;
  std::string command;
  int rm_unstable = 0, device = 0, joint = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-h" || a == "--help") {
      usage();
      return 1;
    } else if (a.rfind("-c=", 0) == 0 || a.rfind("--command=", 0) == 0) {
      command = a.substr(a.find('=') + 1);
    } else if (a.rfind("-r=", 0) == 0 || a.rfind("--rm_unstable=", 0) == 0) {
      rm_unstable = atoi(a.c_str() + a.find('=') + 1);
    } else if (a.rfind("-j=", 0) == 0 || a.rfind("--joint=", 0) == 0) {
      joint = atoi(a.c_str() + a.find('=') + 1);
    } else if (a.rfind("--device=", 0) == 0) {
      device = atoi(a.c_str() + 9);
    } else if (!a.empty() && a[0] == '-') {
      usage();
      return 1;
    } else {
      pos.push_back(a);
    }
  }
  if (pos.size() < 2 || pos[0].empty() || pos[1].empty()) {
    usage();
    return 1;
  }
  const std::vector<std::string> items = command_items(command);
  for (const std::string &item : items)
    if (!joint && joint_item(item)) {
      fprintf(stderr,
              "OpenMVG_BA: -c=%s: item \"%s\" is not supported yet (-c adjusts the structure alone, or rotations / "
              "translations alone; no intrinsics); nothing was written\n",
              command.c_str(), item.c_str());
      return 1;
    }
  const std::string in = pos[0], out_path = pos[1];
  printf("Start bundle adjustment over sfm_data.json.\n");
  printf("Reading sfm_data.json file : %s\n", in.c_str());
  fflush(stdout);
  Doc d;
  std::string err;
  if (!sfmdoc::load(in, false, &d, &err)) {
    fprintf(stderr, "\nThe input sfm_data.json file \"%s\" cannot be read. (%s)\n", in.c_str(), err.c_str());
    return EXIT_FAILURE;
  }
  sfmloc_sfm_desc desc;
  sfmdoc::fill_desc(d, &desc);
  sfmloc_params params;
  sfmloc_sfm_default_params(&params);
  params.device = device;
  sfmloc_sfm *h = nullptr;
  int rc = sfmloc_sfm_create(&desc, &params, &h);
  if (rc == 0) rc = sfmloc_sfm_resect(h, nullptr, nullptr);
  std::vector<sfmloc_sfm_view_result> res(desc.n_views);
  if (rc == 0) rc = sfmloc_sfm_resect_read(h, res.data());
  if (rc) {
    fprintf(stderr, "OpenMVG_BA: %s\n", sfmloc_last_error());
    sfmloc_sfm_destroy(h);
    return 1;
  }
  bool warning = false;
  std::vector<uint8_t> replaced(desc.n_poses, 0);
  for (uint32_t k = 0; k < desc.n_views; ++k) {
    if (!res[k].ran) warning = true;
    if (res[k].ok) replaced[d.view_pose[k]] = 1;
  }
  if (warning) printf("Warning: there is/are frames with too few matches.\n");
  std::vector<uint8_t> valid(desc.n_poses);
  std::vector<double> R(9 * (size_t)desc.n_poses), C(3 * (size_t)desc.n_poses);
  rc = sfmloc_sfm_read(h, valid.data(), R.data(), C.data(), nullptr, nullptr);
  if (rc) {
    fprintf(stderr, "OpenMVG_BA: %s\n", sfmloc_last_error());
    sfmloc_sfm_destroy(h);
    return 1;
  }
  // sfm_data_b4bd.json: the new poses, the structure untouched
  Value b4 = d.root;
  set_key(&b4, "extrinsics", extrinsics(d, valid, R, C, replaced));
  set_key(&b4, "control_points", Value::make_arr());
  const std::string b4_path = folder_of(in) + "sfm_data_b4bd.json";
  if (!write_doc(b4_path, b4)) {
    fprintf(stderr, "OpenMVG_BA: %s cannot be written\n", b4_path.c_str());
    sfmloc_sfm_destroy(h);
    return 1;
  }
  bool cleaned = false;
  auto clean = [&]() {
    uint64_t counts[4];
    const int rcc = sfmloc_sfm_clean(h, kResidualPx, kAngleDeg, rm_unstable != 0, counts);
    if (rcc) return rcc;
    cleaned = true;
    printf("Number of points before cleanup : %llu\n", (unsigned long long)counts[0]);
    printf("Number of points residual error : %llu\n", (unsigned long long)counts[1]);
    printf("Number of points angle error : %llu\n", (unsigned long long)counts[2]);
    printf("Number of points after cleanup : %llu\n", (unsigned long long)counts[3]);
    return 0;
  };
  for (size_t k = 0; k < items.size() && rc == 0; ++k) {
    const std::string &item = items[k];
    const bool rot = has(item, 'r'), trn = has(item, 't'), intr = joint && has(item, 'i'), stru = has(item, 's');
    printf("\nBundle adjustment over %s%s%s%s\n", rot ? "rotations, " : "", trn ? "translations, " : "",
           intr ? "intrinsic params, " : "", stru ? "structure, " : "");
    fflush(stdout);
    const uint32_t what = (rot ? SFMLOC_BA_ROTATION : 0u) | (trn ? SFMLOC_BA_TRANSLATION : 0u) |
                          (intr ? SFMLOC_BA_INTRINSICS : 0u) | (stru ? SFMLOC_BA_STRUCTURE : 0u);
    if (joint && joint_item(item)) rc = sfmloc_sfm_adjust_joint(h, what, nullptr, nullptr);
    else rc = sfmloc_sfm_adjust(h, what, nullptr);
    if (rc == 0 && has(item, 'c')) rc = clean();
  }
  if (rc == 0 && items.empty()) rc = clean();
  std::vector<uint8_t> obs_keep(d.obs_view.size(), 1), lm_keep(d.lm_id.size(), 1);
  std::vector<double> X, K;
  if (rc == 0 && joint && !items.empty()) {
    K.resize(d.intr.size());
    rc = sfmloc_sfm_read_intrinsics(h, K.data());
  }
  if (rc == 0 && !items.empty()) {  // a pose or a landmark the adjustment moved is written from the arrays
    std::vector<double> R2(R.size()), C2(C.size());
    X.resize(d.lm_X.size());
    rc = sfmloc_sfm_read(h, nullptr, R2.data(), C2.data(), nullptr, nullptr);
    if (rc == 0 && !X.empty()) rc = sfmloc_sfm_read_structure(h, X.data());
    if (rc == 0) {
      for (uint32_t p = 0; p < desc.n_poses; ++p)
        if (bits_differ(&R2[9 * (size_t)p], &R[9 * (size_t)p], 9) || bits_differ(&C2[3 * (size_t)p], &C[3 * (size_t)p], 3))
          replaced[p] = 1;
      R.swap(R2);
      C.swap(C2);
    }
  }
  if (rc == 0)
    rc = sfmloc_sfm_read(h, valid.data(), nullptr, nullptr, cleaned ? obs_keep.data() : nullptr,
                         cleaned ? lm_keep.data() : nullptr);
  sfmloc_sfm_destroy(h);
  if (rc) {
    fprintf(stderr, "OpenMVG_BA: %s\n", sfmloc_last_error());
    return 1;
  }
  Value outd = d.root;
  set_key(&outd, "extrinsics", extrinsics(d, valid, R, C, replaced));
  for (size_t i = 0; i < d.intr_type.size() && !K.empty(); ++i)  // an intrinsic the adjustment moved: from the arrays
    if (bits_differ(&K[6 * i], &d.intr[6 * i], 6)) set_intrinsic(&outd, i, d.intr_type[i], &K[6 * i]);
  Value *st = outd.get("structure");
  if (st) {
    Value kept = Value::make_arr();
    for (size_t l = 0; l < st->a.size(); ++l) {
      if (!lm_keep[l]) continue;
      Value e = std::move(st->a[l]);
      if (!X.empty() && bits_differ(&X[3 * l], &d.lm_X[3 * l], 3)) {
        Value xs = Value::make_arr();
        for (int j = 0; j < 3; ++j) xs.a.push_back(Value::make_float(X[3 * l + j]));
        set_key(e.get("value"), "X", xs);
      }
      Value *obs = e.get("value")->get("observations");
      Value ko = Value::make_arr();
      for (size_t j = 0; j < obs->a.size(); ++j)
        if (obs_keep[d.obs_off[l] + j]) ko.a.push_back(std::move(obs->a[j]));
      *obs = std::move(ko);
      kept.a.push_back(std::move(e));
    }
    *st = std::move(kept);
  }
  set_key(&outd, "control_points", Value::make_arr());
  if (!write_doc(out_path, outd)) {
    fprintf(stderr, "OpenMVG_BA: %s cannot be written\n", out_path.c_str());
    return 1;
  }
  return 0;
}
