// The sfm_data.json document as the map-side tools read it (host code only; shared by adjust_cli.cpp, colorize_cli.cpp,
// structure_cli.cpp, relpose_cli.cpp and globalposes_cli.cpp): the parsed JSON and the arrays of sfmloc_sfm_desc built from it -- views
// ascending, a pose table (every extrinsic key and every view's id_pose, ascending), landmarks ascending with their
// observations in CSR.
#pragma once

#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/sfmloc.h"
#include "sfm_json.h"

namespace sfmdoc {

using sfmjson::Value;

const uint32_t kUnsupportedType = 0xFFFFFFFFu;  // an intrinsic type other than pinhole / pinhole_radial_k3


inline bool num_u32(const Value *v, uint32_t *out) {
  if (!v || v->kind != Value::Int) return false;
  const long long x = strtoll(v->s.c_str(), nullptr, 10);
  if (x < 0 || x > 0xFFFFFFFFll) return false;
  *out = (uint32_t)x;
  return true;
}
inline bool num_vec(const Value *v, size_t n, double *out) {
  if (!v || v->kind != Value::Arr || v->a.size() != n) return false;
  for (size_t i = 0; i < n; ++i) {
    if (!v->a[i].is_num()) return false;
    out[i] = v->a[i].num();
  }
  return true;
}
inline const Value *ptr_data(const Value *value) {  // cereal's polymorphic pointer: value.ptr_wrapper.data
  const Value *pw = value ? value->get("ptr_wrapper") : nullptr;
  return pw ? pw->get("data") : nullptr;
}
// obj[k] = v as a Python dict assigns it: a key already there keeps its place.  (These two would sit beside Value in
// sfm_json.h, which the library includes too; they are for the tools alone.)
inline void set_key(Value *obj, const char *k, Value v) {
  Value *slot = obj->get(k);
  if (slot) *slot = std::move(v);
  else obj->o.emplace_back(k, std::move(v));
}
inline Value make_int(uint64_t v) {
  Value x;
  x.kind = Value::Int;
  x.s = std::to_string(v);
  return x;
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

// the arrays of a document already parsed into d->root
inline bool build(Doc *d, std::string *err) {
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

// read, parse, build; drop_structure: the input's own `structure` is emptied first (the tools that rebuild it, or never
// look at it: the key keeps its place in the document)
inline bool load(const std::string &path, bool drop_structure, Doc *d, std::string *err) {
  std::string text;
  if (!sfmjson::read_file(path.c_str(), &text)) return *err = "cannot be read", false;
  if (!sfmjson::parse(text, &d->root, err)) return false;
  if (drop_structure && d->root.kind == Value::Obj) set_key(&d->root, "structure", Value::make_arr());
  return build(d, err);
}

// the desc over a loaded document (the document must outlive it)
inline void fill_desc(const Doc &d, sfmloc_sfm_desc *desc) {
  memset(desc, 0, sizeof *desc);
  desc->n_views = (uint32_t)d.view_id.size();
  desc->view_id = d.view_id.data();
  desc->view_intrinsic = d.view_intr.data();
  desc->view_pose = d.view_pose.data();
  desc->n_intrinsics = (uint32_t)d.intr_type.size();
  desc->intrinsic_type = d.intr_type.data();
  desc->intrinsic = d.intr.data();
  desc->n_poses = (uint32_t)d.pose_id.size();
  desc->pose_valid = d.pose_valid.data();
  desc->pose_R = d.pose_R.data();
  desc->pose_C = d.pose_C.data();
  desc->n_landmarks = (uint32_t)d.lm_id.size();
  desc->landmark_id = d.lm_id.data();
  desc->landmark_X = d.lm_X.data();
  desc->obs_off = d.obs_off.data();
  desc->obs_view = d.obs_view.data();
  desc->obs_x = d.obs_x.data();
}

}  // namespace sfmdoc
