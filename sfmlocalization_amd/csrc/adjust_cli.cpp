// OpenMVG_BA (OpenMVG_BA/src/adjust_sfm_data.cpp) without -c as a C++ host program over the C ABI (plain g++):
//
//   OpenMVG_BA <sfm_data> <sfm_data_out> [-c=...] [-r=0|1] [--device=0]
//
// The same program as sfmlocalization_amd/adjust.py, and the same bytes: every view with more than 10 observations is
// re-resected on the device (sfmloc_sfm_resect), <folder of sfm_data>/sfm_data_b4bd.json is written with the new poses
// and the structure untouched (:152-155), the structure is cleaned (sfmloc_sfm_clean: residual 4 px, angle 2 degrees,
// unstable poses with -r=1; :245-260) and the result is written to sfm_data_out (which may be sfm_data itself: the
// merge loop calls it in place).  Both files are what Python's json.dump writes for the document: views, intrinsics,
// root_path and key order as in the input, extrinsics in ascending pose id, control_points [] (Save without
// CONTROL_POINTS).  -c (the Ceres bundle adjustment, :158-240) is not supported yet: refused, nothing written.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_json.h"

using sfmjson::Value;

namespace {

const uint32_t kUnsupportedType = 0xFFFFFFFFu;  // an intrinsic type other than pinhole / pinhole_radial_k3
const double kResidualPx = 4.0, kAngleDeg = 2.0;  // STRUCTURE_CLEANUP_RESIDUAL_ERROR / _ANGLE_ERROR (:40-41)

void usage() {
  fprintf(stderr,
          "Execute bundle adjustment for sfm_data.json\n"
          "Usage: OpenMVG_BA [params] sfm_data sfm_data_out\n"
          "\t-c, --command\n\t\tCommand for order of bundle adjustment (not supported yet: only the default, no BD)\n"
          "\t-r, --rm_unstable (value:0)\n\t\tRemove unstable pose and observation\n");
}

bool num_u32(const Value *v, uint32_t *out) {
  if (!v || v->kind != Value::Int) return false;
  const long long x = strtoll(v->s.c_str(), nullptr, 10);
  if (x < 0 || x > 0xFFFFFFFFll) return false;
  *out = (uint32_t)x;
  return true;
}
bool num_vec(const Value *v, size_t n, double *out) {
  if (!v || v->kind != Value::Arr || v->a.size() != n) return false;
  for (size_t i = 0; i < n; ++i) {
    if (!v->a[i].is_num()) return false;
    out[i] = v->a[i].num();
  }
  return true;
}
const Value *ptr_data(const Value *value) {  // cereal's polymorphic pointer: value.ptr_wrapper.data
  const Value *pw = value ? value->get("ptr_wrapper") : nullptr;
  return pw ? pw->get("data") : nullptr;
}

struct Doc {
  Value root;
  std::vector<uint32_t> view_id, view_intr, view_pose_id, intr_type;
  std::vector<double> intr;
  std::vector<uint32_t> pose_id;  // the pose table, ascending id
  std::vector<uint8_t> pose_valid;
  std::vector<double> pose_R, pose_C;
  std::vector<const Value *> pose_src;  // the input's extrinsic value of a pose, or null
  std::vector<uint32_t> view_pose;      // view -> pose table index
  std::vector<uint32_t> lm_id;
  std::vector<double> lm_X;
  std::vector<uint64_t> obs_off;
  std::vector<uint32_t> obs_view;
  std::vector<double> obs_x;
};

bool load(const std::string &path, Doc *d, std::string *err) {
  std::string text;
  if (!sfmjson::read_file(path.c_str(), &text)) return *err = "cannot be read", false;
  if (!sfmjson::parse(text, &d->root, err)) return false;
  const Value &r = d->root;
  const Value *views = r.get("views"), *intrs = r.get("intrinsics"), *exts = r.get("extrinsics"),
              *st = r.get("structure");
  if (r.kind != Value::Obj || !views || views->kind != Value::Arr || !intrs || intrs->kind != Value::Arr ||
      (exts && exts->kind != Value::Arr) || (st && st->kind != Value::Arr))
    return *err = "not an sfm_data document (views, intrinsics, extrinsics, structure)", false;
  // intrinsics: cereal names a polymorphic type at its first occurrence only (polymorphic_id with bit 31 set)
  std::map<uint32_t, std::string> type_names;
  std::map<uint32_t, uint32_t> intr_index;
  for (const Value &e : intrs->a) {
    uint32_t key, pid;
    const Value *val = e.get("value");
    if (!num_u32(e.get("key"), &key) || !val || !num_u32(val->get("polymorphic_id"), &pid))
      return *err = "malformed intrinsic", false;
    const Value *pn = val->get("polymorphic_name");
    if (pn && pn->kind == Value::Str) type_names[pid & 0x7FFFFFFFu] = pn->s;
    const std::string type = type_names.count(pid & 0x7FFFFFFFu) ? type_names[pid & 0x7FFFFFFFu] : std::string();
    const Value *data = ptr_data(val);
    double k[6] = {0, 0, 0, 0, 0, 0};
    const Value *pin = data;
    uint32_t t = 0;
    if (type == "pinhole_radial_k3") {
      t = 3;
      pin = data ? data->get("value0") : nullptr;
      if (!num_vec(data ? data->get("disto_k3") : nullptr, 3, k + 3)) return *err = "malformed disto_k3", false;
    } else if (type != "pinhole") {
      t = kUnsupportedType;  // refused by sfmloc_sfm_create (SFMLOC_EIO), as sfmloc_open refuses it
    }
    if (t != kUnsupportedType) {
      const Value *fl = pin ? pin->get("focal_length") : nullptr;
      if (!fl || !fl->is_num() || !num_vec(pin->get("principal_point"), 2, k + 1))
        return *err = "malformed intrinsic " + std::to_string(key), false;
      k[0] = fl->num();
    }
    intr_index[key] = (uint32_t)d->intr_type.size();
    d->intr_type.push_back(t);
    d->intr.insert(d->intr.end(), k, k + 6);
  }
  static const std::vector<Value> kNone;
  const std::vector<Value> &ext_list = exts ? exts->a : kNone, &lm_list = st ? st->a : kNone;
  std::map<uint32_t, const Value *> ext_by_id;
  for (const Value &e : ext_list) {
    uint32_t key;
    if (!num_u32(e.get("key"), &key) || !e.get("value")) return *err = "malformed extrinsic", false;
    ext_by_id[key] = e.get("value");
  }
  std::map<uint32_t, uint32_t> view_index;
  for (const Value &e : views->a) {
    const Value *data = ptr_data(e.get("value"));
    uint32_t vid, ii, pid;
    if (!data || !num_u32(data->get("id_view"), &vid) || !num_u32(data->get("id_intrinsic"), &ii) ||
        !num_u32(data->get("id_pose"), &pid))
      return *err = "malformed view", false;
    if (!d->view_id.empty() && vid <= d->view_id.back()) return *err = "views are not in ascending id_view", false;
    if (!intr_index.count(ii)) return *err = "view " + std::to_string(vid) + ": no intrinsic " + std::to_string(ii), false;
    view_index[vid] = (uint32_t)d->view_id.size();
    d->view_id.push_back(vid);
    d->view_intr.push_back(intr_index[ii]);
    d->view_pose_id.push_back(pid);
  }
  std::map<uint32_t, uint32_t> pose_index;
  for (const auto &kv : ext_by_id) pose_index[kv.first] = 0;
  for (uint32_t pid : d->view_pose_id) pose_index[pid] = 0;
  for (auto &kv : pose_index) {
    kv.second = (uint32_t)d->pose_id.size();
    d->pose_id.push_back(kv.first);
    double R[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, C[3] = {0, 0, 0};
    const Value *src = ext_by_id.count(kv.first) ? ext_by_id[kv.first] : nullptr;
    if (src) {
      const Value *rot = src->get("rotation");
      if (!rot || rot->kind != Value::Arr || rot->a.size() != 3 || !num_vec(&rot->a[0], 3, R) ||
          !num_vec(&rot->a[1], 3, R + 3) || !num_vec(&rot->a[2], 3, R + 6) || !num_vec(src->get("center"), 3, C))
        return *err = "malformed extrinsic " + std::to_string(kv.first), false;
    }
    d->pose_valid.push_back(src ? 1 : 0);
    d->pose_src.push_back(src);
    d->pose_R.insert(d->pose_R.end(), R, R + 9);
    d->pose_C.insert(d->pose_C.end(), C, C + 3);
  }
  for (uint32_t pid : d->view_pose_id) d->view_pose.push_back(pose_index[pid]);
  d->obs_off.push_back(0);
  for (const Value &e : lm_list) {
    uint32_t lid;
    const Value *val = e.get("value");
    double X[3];
    const Value *obs = val ? val->get("observations") : nullptr;
    if (!num_u32(e.get("key"), &lid) || !val || !num_vec(val->get("X"), 3, X) || !obs || obs->kind != Value::Arr)
      return *err = "malformed landmark", false;
    if (!d->lm_id.empty() && lid <= d->lm_id.back()) return *err = "structure is not in ascending landmark id", false;
    d->lm_id.push_back(lid);
    d->lm_X.insert(d->lm_X.end(), X, X + 3);
    for (const Value &o : obs->a) {
      uint32_t vid;
      double x[2];
      const Value *ov = o.get("value");
      if (!num_u32(o.get("key"), &vid) || !ov || !num_vec(ov->get("x"), 2, x))
        return *err = "malformed observation of landmark " + std::to_string(lid), false;
      if (!view_index.count(vid))
        return *err = "landmark " + std::to_string(lid) + ": observation of unknown view " + std::to_string(vid), false;
      d->obs_view.push_back(view_index[vid]);
      d->obs_x.push_back(x[0]);
      d->obs_x.push_back(x[1]);
    }
    d->obs_off.push_back(d->obs_view.size());
  }
  return true;
}

void set_key(Value *obj, const char *k, Value v) {
  Value *slot = obj->get(k);
  if (slot) *slot = std::move(v);
  else obj->o.emplace_back(k, std::move(v));
}

// extrinsics: the valid poses in ascending id; an input pose untouched keeps its JSON value as it was
Value extrinsics(const Doc &d, const std::vector<uint8_t> &valid, const std::vector<double> &R,
                 const std::vector<double> &C, const std::vector<uint8_t> &replaced) {
  Value a = Value::make_arr();
  for (size_t p = 0; p < d.pose_id.size(); ++p) {
    if (!valid[p]) continue;
    Value e;
    e.kind = Value::Obj;
    Value key;
    key.kind = Value::Int;
    key.s = std::to_string(d.pose_id[p]);
    e.o.emplace_back("key", key);
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

}  // namespace

int main(int argc, char **argv) {
  if (argc < 2) {
    usage();
    return 1;
  }
  std::vector<std::string> pos;
  std::string command;
  int rm_unstable = 0, device = 0;
  for (int i = 1; i < argc; ++i) {
    const std::string a = argv[i];
    if (a == "-h" || a == "--help") {
      usage();
      return 1;
    } else if (a.rfind("-c=", 0) == 0 || a.rfind("--command=", 0) == 0) {
      command = a.substr(a.find('=') + 1);
    } else if (a.rfind("-r=", 0) == 0 || a.rfind("--rm_unstable=", 0) == 0) {
      rm_unstable = atoi(a.c_str() + a.find('=') + 1);
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
  if (!command.empty()) {
    fprintf(stderr, "OpenMVG_BA: -c=%s: the bundle adjustment command (-c) is not supported yet; nothing was written\n",
            command.c_str());
    return 1;
  }
  const std::string in = pos[0], out_path = pos[1];
  printf("Start bundle adjustment over sfm_data.json.\n");
  printf("Reading sfm_data.json file : %s\n", in.c_str());
  fflush(stdout);
  Doc d;
  std::string err;
  if (!load(in, &d, &err)) {
    fprintf(stderr, "\nThe input sfm_data.json file \"%s\" cannot be read. (%s)\n", in.c_str(), err.c_str());
    return EXIT_FAILURE;
  }
  sfmloc_sfm_desc desc;
  memset(&desc, 0, sizeof desc);
  desc.n_views = (uint32_t)d.view_id.size();
  desc.view_id = d.view_id.data();
  desc.view_intrinsic = d.view_intr.data();
  desc.view_pose = d.view_pose.data();
  desc.n_intrinsics = (uint32_t)d.intr_type.size();
  desc.intrinsic_type = d.intr_type.data();
  desc.intrinsic = d.intr.data();
  desc.n_poses = (uint32_t)d.pose_id.size();
  desc.pose_valid = d.pose_valid.data();
  desc.pose_R = d.pose_R.data();
  desc.pose_C = d.pose_C.data();
  desc.n_landmarks = (uint32_t)d.lm_id.size();
  desc.landmark_id = d.lm_id.data();
  desc.landmark_X = d.lm_X.data();
  desc.obs_off = d.obs_off.data();
  desc.obs_view = d.obs_view.data();
  desc.obs_x = d.obs_x.data();
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
  uint64_t counts[4];
  rc = sfmloc_sfm_clean(h, kResidualPx, kAngleDeg, rm_unstable != 0, counts);
  std::vector<uint8_t> obs_keep(d.obs_view.size()), lm_keep(d.lm_id.size());
  if (rc == 0) rc = sfmloc_sfm_read(h, valid.data(), nullptr, nullptr, obs_keep.data(), lm_keep.data());
  sfmloc_sfm_destroy(h);
  if (rc) {
    fprintf(stderr, "OpenMVG_BA: %s\n", sfmloc_last_error());
    return 1;
  }
  printf("Number of points before cleanup : %llu\n", (unsigned long long)counts[0]);
  printf("Number of points residual error : %llu\n", (unsigned long long)counts[1]);
  printf("Number of points angle error : %llu\n", (unsigned long long)counts[2]);
  printf("Number of points after cleanup : %llu\n", (unsigned long long)counts[3]);
  Value outd = d.root;
  set_key(&outd, "extrinsics", extrinsics(d, valid, R, C, replaced));
  Value *st = outd.get("structure");
  if (st) {
    Value kept = Value::make_arr();
    for (size_t l = 0; l < st->a.size(); ++l) {
      if (!lm_keep[l]) continue;
      Value e = std::move(st->a[l]);
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
