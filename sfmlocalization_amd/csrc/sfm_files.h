// The on-disk contract as the C++ tools read and write it (host code only, no HIP; shared by the *_cli.cpp programs):
// what sfmlocalization_amd/fileio.py is for the Python tools.  Every reader mirrors one function of fileio.py or of
// os.path, named at its definition; where a damaged file could be read in more than one way, fileio.py decides.
// tests/test_sfm_files.py holds these functions against their Python twins (tests/cpp/sfm_files.cpp).
#pragma once

#include <sys/stat.h>

#include <cctype>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <initializer_list>
#include <map>
#include <sstream>
#include <string>
#include <utility>
#include <vector>

#include "sfm_json.h"

namespace sfmfiles {

// ---- paths ----
// os.path.join(root, name)
inline std::string join(const std::string &root, const std::string &name) {
  if (root.empty() || (!name.empty() && name[0] == '/')) return name;
  return root + (root.back() == '/' ? "" : "/") + name;
}
// os.path.basename(p)
inline std::string basename_of(const std::string &p) {
  const size_t s = p.rfind('/');
  return s == std::string::npos ? p : p.substr(s + 1);
}
// os.path.dirname(p)
inline std::string dirname_of(const std::string &p) {
  const size_t s = p.rfind('/');
  if (s == std::string::npos) return std::string();
  std::string head = p.substr(0, s + 1);
  if (head.find_first_not_of('/') != std::string::npos)
    while (head.back() == '/') head.pop_back();
  return head;
}
// os.path.splitext(os.path.basename(p))[0]: leading dots belong to the name (the tools whose Python twin names a
// view's files this way: structure, relpose)
inline std::string stem_of(const std::string &p) {
  std::string base = basename_of(p);
  size_t lead = 0;
  while (lead < base.size() && base[lead] == '.') ++lead;
  const size_t dot = base.rfind('.');
  if (dot != std::string::npos && dot > lead) base.resize(dot);
  return base;
}
// stlplus::basename_part(p), the reference's form and the library loader's (map_io.hip): everything before the last
// dot, so ".hidden" gives "".  The tools that name files the loader or the reference's own programs look up use this
// one (extfeat, localize, trainbow); it differs from stem_of only for a name whose dots all lead it.
inline std::string basename_part(const std::string &p) {
  const std::string base = basename_of(p);
  const size_t dot = base.rfind('.');
  return dot == std::string::npos ? base : base.substr(0, dot);
}
// what follows the last dot of the base name, "" without one (the image filter of localization.cpp:204-206)
inline std::string ext_of(const std::string &p) {
  const std::string base = basename_of(p);
  const size_t dot = base.rfind('.');
  return dot == std::string::npos ? std::string() : base.substr(dot + 1);
}
// os.path.isfile(p), os.path.isdir(p)
inline bool is_file(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISREG(st.st_mode);
}
inline bool is_dir(const std::string &p) {
  struct stat st;
  return stat(p.c_str(), &st) == 0 && S_ISDIR(st.st_mode);
}

inline bool read_all(const std::string &p, std::vector<uint8_t> *out) {
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return false;
  fseek(f, 0, SEEK_END);
  const long n = ftell(f);
  fseek(f, 0, SEEK_SET);
  out->resize(n > 0 ? (size_t)n : 0);
  const bool ok = n >= 0 && fread(out->data(), 1, out->size(), f) == out->size();
  fclose(f);
  return ok;
}

// ---- <base>.desc: [u64 N][N x 64 B] (fileio.read_desc) ----
// Appends the N rows to *rows.  N is held against the file's length before anything is allocated; a short header or a
// body shorter than N rows is refused with *rows as it was, bytes after the rows are ignored.
inline bool read_desc(const std::string &p, std::vector<uint8_t> *rows) {
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return false;
  uint64_t n = 0;
  struct stat st;
  bool ok = fstat(fileno(f), &st) == 0 && st.st_size >= 8 && fread(&n, 8, 1, f) == 1 && n <= ((uint64_t)st.st_size - 8) / 64;
  if (ok && n) {
    const size_t at = rows->size();
    rows->resize(at + (size_t)n * 64);
    ok = fread(rows->data() + at, 64, (size_t)n, f) == (size_t)n;
    if (!ok) rows->resize(at);
  }
  fclose(f);
  return ok;
}

// ---- <base>.bow and the other saveMatBin files: [i32 rows][i32 cols][i32 cv depth][rows x cols values]
// (fileio.read_mat_bin; hulo::readMatBin, FileUtils.cpp:43-75) ----
// The values row-major as doubles, which hold every depth's values exactly (0 u8, 1 i8, 2 u16, 3 i16, 4 i32, 5 f32,
// 6 f64).  rows = 0 is an empty matrix with nothing after it.  A short header, an unknown depth, a negative size or a
// body shorter than rows x cols values is refused with *values as it was; bytes after the values are ignored.
inline bool read_mat_bin(const std::string &p, int32_t *rows, int32_t *cols, std::vector<double> *values) {
  static const size_t kDepthBytes[7] = {1, 1, 2, 2, 4, 4, 8};
  FILE *f = fopen(p.c_str(), "rb");
  if (!f) return false;
  int32_t head[3] = {0, 0, 0};
  struct stat st;
  bool ok = fstat(fileno(f), &st) == 0 && fread(&head[0], 4, 1, f) == 1;
  std::vector<double> v;
  if (ok && head[0] != 0) {
    ok = fread(&head[1], 4, 2, f) == 2 && head[0] > 0 && head[1] > 0 && head[2] >= 0 && head[2] <= 6;
    const uint64_t count = ok ? (uint64_t)head[0] * (uint64_t)head[1] : 0;
    ok = ok && count <= ((uint64_t)st.st_size - 12) / kDepthBytes[head[2]];
    if (ok) {
      std::vector<uint8_t> raw((size_t)count * kDepthBytes[head[2]]);
      ok = fread(raw.data(), 1, raw.size(), f) == raw.size();
      v.resize(ok ? (size_t)count : 0);
      for (size_t i = 0; ok && i < (size_t)count; ++i) {
        const uint8_t *at = raw.data() + i * kDepthBytes[head[2]];
        switch (head[2]) {
          case 0: v[i] = *at; break;
          case 1: v[i] = *reinterpret_cast<const int8_t *>(at); break;
          case 2: { uint16_t x; memcpy(&x, at, 2); v[i] = x; break; }
          case 3: { int16_t x; memcpy(&x, at, 2); v[i] = x; break; }
          case 4: { int32_t x; memcpy(&x, at, 4); v[i] = x; break; }
          case 5: { float x; memcpy(&x, at, 4); v[i] = x; break; }
          default: { double x; memcpy(&x, at, 8); v[i] = x; break; }
        }
      }
    }
  }
  fclose(f);
  if (!ok) return false;
  *rows = head[0];
  *cols = head[0] ? head[1] : 0;
  values->swap(v);
  return true;
}

// ---- <base>.feat: "x y size angle" per line (fileio.read_feat) ----
// Appends x, y of every line as float32 and stops at the first line with fewer than four tokens.  (A token that
// write_feat or `ostream << float` emits has at most six significant digits; strtof of it and the float of its strtod,
// which is how the older tools read it, are the same number.)
inline bool read_feat(const std::string &p, std::vector<float> *xy) {
  std::ifstream f(p);
  if (!f) return false;
  std::string line;
  while (std::getline(f, line)) {
    std::istringstream ss(line);
    std::string t[4];
    if (!(ss >> t[0] >> t[1] >> t[2] >> t[3])) break;
    xy->push_back(strtof(t[0].c_str(), nullptr));
    xy->push_back(strtof(t[1].c_str(), nullptr));
  }
  return true;
}

// ---- matches.*.txt: "I J\nn\ni j\n..." per pair, view ids as keys (fileio.read_matches_txt / write_matches_txt) ----
typedef std::map<std::pair<uint32_t, uint32_t>, std::pair<std::vector<uint32_t>, std::vector<uint32_t>>> PairMatches;

// the same pair twice: the later entry replaces the earlier, as a dictionary does.  A file that ends inside an entry is
// "truncated"; a token that is not a number, or not one of 32 bits without a sign, is "malformed" (fileio raises on the
// first two and wraps the last silently into uint32, which no well-formed file means).
inline bool read_matches(const std::string &path, PairMatches *out, std::string *err) {
  std::ifstream f(path);
  if (!f) return *err = "cannot be read", false;
  PairMatches all;
  std::string ta, tb, tn;
  while (f >> ta) {
    if (!(f >> tb >> tn)) return *err = "truncated", false;
    char *e1, *e2, *e3;
    const long long a = strtoll(ta.c_str(), &e1, 10), b = strtoll(tb.c_str(), &e2, 10), n = strtoll(tn.c_str(), &e3, 10);
    if (*e1 || *e2 || *e3 || a < 0 || b < 0 || n < 0 || a > 0xFFFFFFFFll || b > 0xFFFFFFFFll) return *err = "malformed", false;
    auto &dst = all[{(uint32_t)a, (uint32_t)b}];
    dst.first.clear();
    dst.second.clear();
    for (long long t = 0; t < n; ++t) {
      std::string ti, tj;
      if (!(f >> ti >> tj)) return *err = "truncated", false;
      const long long i = strtoll(ti.c_str(), &e1, 10), j = strtoll(tj.c_str(), &e2, 10);
      if (*e1 || *e2 || i < 0 || j < 0 || i > 0xFFFFFFFFll || j > 0xFFFFFFFFll) return *err = "malformed", false;
      dst.first.push_back((uint32_t)i);
      dst.second.push_back((uint32_t)j);
    }
  }
  out->swap(all);
  return true;
}

inline bool write_matches(const std::string &path, const PairMatches &m) {
  FILE *f = fopen(path.c_str(), "w");
  if (!f) return false;
  for (const auto &kv : m) {
    fprintf(f, "%u %u\n%zu\n", kv.first.first, kv.first.second, kv.second.first.size());
    for (size_t k = 0; k < kv.second.first.size(); ++k) fprintf(f, "%u %u\n", kv.second.first[k], kv.second.second[k]);
  }
  return fclose(f) == 0;
}

// the pair list layout of sfmloc_tracks_build and sfmloc_relative_poses (capi.pair_arrays): pairs as view indices in
// ascending (I, J), the matches of pair k at [offsets[k], offsets[k + 1])
struct PairList {
  std::vector<uint32_t> pairs, mi, mj;
  std::vector<uint64_t> offsets{0};
};

inline bool read_matches(const std::string &path, const std::map<uint32_t, uint32_t> &view_index, PairList *out, std::string *err) {
  PairMatches all;
  if (!read_matches(path, &all, err)) return false;
  for (const auto &kv : all) {
    const auto ia = view_index.find(kv.first.first), ib = view_index.find(kv.first.second);
    if (ia == view_index.end() || ib == view_index.end()) return *err = "a pair names an unknown view", false;
    out->pairs.push_back(ia->second);
    out->pairs.push_back(ib->second);
    out->mi.insert(out->mi.end(), kv.second.first.begin(), kv.second.first.end());
    out->mj.insert(out->mj.end(), kv.second.second.begin(), kv.second.second.end());
    out->offsets.push_back(out->mi.size());
  }
  return true;
}

// ---- pair_scales.json: the records of sfmloc_wedge_scales by view ids (fileio.read_pair_scales / write_pair_scales) ----
constexpr int kPairScalesVersion = 1;
struct PairScale {
  uint32_t view, k[2], l[2], n_shared;  // k, l: the two view ids of each pair, in the pair list's order
  double ratio;
};
struct PairScales {
  uint32_t min_shared = 8, max_shared = 2048;
  std::vector<PairScale> rec;
};

inline sfmjson::Value json_int(unsigned long long v) {
  sfmjson::Value x;
  x.kind = sfmjson::Value::Int;
  x.s = std::to_string(v);
  return x;
}

// the bytes json.dump writes for fileio.write_pair_scales' document
inline std::string format_pair_scales(const PairScales &ps) {
  using sfmjson::Value;
  Value list = Value::make_arr();
  for (const PairScale &r : ps.rec) {
    Value e, k = Value::make_arr(), l = Value::make_arr();
    for (int i = 0; i < 2; ++i) {
      k.a.push_back(json_int(r.k[i]));
      l.a.push_back(json_int(r.l[i]));
    }
    e.kind = Value::Obj;
    e.o.emplace_back("view", json_int(r.view));
    e.o.emplace_back("k", k);
    e.o.emplace_back("l", l);
    e.o.emplace_back("n_shared", json_int(r.n_shared));
    e.o.emplace_back("ratio", Value::make_float(r.ratio));
    list.a.push_back(e);
  }
  Value doc;
  doc.kind = Value::Obj;
  doc.o.emplace_back("pair_scales_version", json_int(kPairScalesVersion));
  doc.o.emplace_back("min_shared", json_int(ps.min_shared));
  doc.o.emplace_back("max_shared", json_int(ps.max_shared));
  doc.o.emplace_back("pair_scales", list);
  std::string text;
  sfmjson::dump(doc, &text);
  return text;
}

inline bool write_pair_scales(const std::string &path, const PairScales &ps) {
  return sfmjson::write_file(path.c_str(), format_pair_scales(ps));
}

inline bool read_pair_scales(const std::string &path, PairScales *out, std::string *err) {
  using sfmjson::Value;
  std::string text;
  Value doc;
  if (!sfmjson::read_file(path.c_str(), &text)) return *err = "cannot be read", false;
  if (!sfmjson::parse(text, &doc, err)) return false;
  const auto u32 = [](const Value *v, uint32_t *o) {
    if (!v || v->kind != Value::Int || v->s.empty() || v->s[0] == '-' || v->s.size() > 10) return false;
    const unsigned long long x = strtoull(v->s.c_str(), nullptr, 10);
    *o = (uint32_t)x;
    return x <= 0xFFFFFFFFull;
  };
  uint32_t version = 0;
  if (doc.kind != Value::Obj || !u32(doc.get("pair_scales_version"), &version) || version != (uint32_t)kPairScalesVersion)
    return *err = "not a pair_scales file of version 1", false;
  PairScales ps;
  const Value *list = doc.get("pair_scales");
  if (!u32(doc.get("min_shared"), &ps.min_shared) || !u32(doc.get("max_shared"), &ps.max_shared) || !list ||
      list->kind != Value::Arr)
    return *err = "malformed pair_scales file", false;
  for (const Value &e : list->a) {
    PairScale r;
    const Value *k = e.get("k"), *l = e.get("l"), *q = e.get("ratio");
    if (e.kind != Value::Obj || !k || !l || k->kind != Value::Arr || l->kind != Value::Arr || k->a.size() != 2 ||
        l->a.size() != 2 || !q || !q->is_num() || !u32(e.get("view"), &r.view) || !u32(e.get("n_shared"), &r.n_shared) ||
        !u32(&k->a[0], &r.k[0]) || !u32(&k->a[1], &r.k[1]) || !u32(&l->a[0], &r.l[0]) || !u32(&l->a[1], &r.l[1]))
      return *err = "malformed pair_scales file", false;
    r.ratio = q->num();
    ps.rec.push_back(r);
  }
  *out = std::move(ps);
  return true;
}

// ---- cv::CommandLineParser syntax: positionals, -k=v / --key=v, bare flags (engine.parse_cv_args) ----
inline bool is_number(const std::string &s) {
  char *end = nullptr;
  std::strtod(s.c_str(), &end);
  return !s.empty() && end && *end == '\0';
}

struct Args {
  std::vector<std::string> pos;
  std::map<std::string, std::string> opt;
  std::string get(std::initializer_list<const char *> names, const char *def) const {
    std::string v = def;
    for (const char *n : names) {
      auto it = opt.find(n);
      if (it != opt.end()) v = it->second;
    }
    return v;
  }
  bool flag(std::initializer_list<const char *> names) const {
    std::string v = get(names, "false");
    for (char &c : v) c = (char)tolower(c);
    return v == "1" || v == "true" || v == "yes";
  }
};

inline Args parse_args(int argc, char **argv) {
  Args a;
  for (int i = 1; i < argc; ++i) {
    std::string s = argv[i];
    if (s.size() > 1 && s[0] == '-' && !is_number(s)) {
      size_t p = s.find_first_not_of('-');
      std::string kv = s.substr(p == std::string::npos ? s.size() : p);
      size_t eq = kv.find('=');
      if (eq == std::string::npos)
        a.opt[kv] = "true";
      else
        a.opt[kv.substr(0, eq)] = kv.substr(eq + 1);
    } else {
      a.pos.push_back(s);
    }
  }
  return a;
}

}  // namespace sfmfiles
