// ComputeRelativePoses as a C++ host program over the C ABI (plain g++):
//
//   ComputeRelativePoses -i <sfm_data.json> -m <matchDir> [-f <match file = matches.f.txt>] [-o <matches.e.txt>]
//                        [-p <relative_poses.json>] [-n <iterations = 256>] [-t <precision px = 2.5>] [--seed N] [--device 0]
//                        [-s <pair scales = none>] [--refine]
//
// The same program as sfmlocalization_amd/relpose.py and the same bytes in both output files: the relative pose of every
// matched view pair (sfmloc_relative_poses, the first stage of openMVG_main_GlobalSfM).  The essential matches hold the ok
// pairs only, each with its inliers in ascending (i, j); the poses file lists them in ascending (I, J).  With --refine
// sfmloc_refine_relative_poses runs on the ok pairs: every entry gains "refine" and carries the refined R, t and E where
// its status is 1 or 3.  With -s the records of sfmloc_wedge_scales on the call's results (the refined poses after
// --refine) are written by view ids (sfm_files.h write_pair_scales).
#include <algorithm>
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
using sfmjson::Value;

namespace {

const char *kName = "ComputeRelativePoses";

void usage() {
  fprintf(stderr,
          "Usage: %s\n"
          "[-i|--input_file] path to a SfM_Data scene\n"
          "[-m|--match_dir] path to the features and matches that correspond to the provided SfM_Data scene\n"
          "\n[Optional]\n"
          "[-f|--match_file] path to a matches file (default: matches.f.txt in the match directory)\n"
          "[-o|--output_file] essential matches to write (default: matches.e.txt in the match directory)\n"
          "[-p|--poses_file] relative poses to write (default: relative_poses.json in the match directory)\n"
          "[-n|--max_iteration] AC-RANSAC iterations per pair (256)\n"
          "[-t|--precision] upper bound on the residual in pixels (2.5)\n"
          "[--seed] sampling seed\n"
          "[--device] HIP device (0)\n"
          "[-s|--scales_file] pair scales to write (default: none)\n"
          "[--refine] adjust every ok pair's pose on its inliers\n",
          kName);
}

Value floats(const double *v, int n) {
  Value a = Value::make_arr();
  for (int i = 0; i < n; ++i) a.a.push_back(Value::make_float(v[i]));
  return a;
}

Value rows3(const double *v) {
  Value a = Value::make_arr();
  for (int i = 0; i < 3; ++i) a.a.push_back(floats(v + 3 * i, 3));
  return a;
}

}  // namespace

int main(int argc, char **argv) {
  std::string in, match_dir, match_file = "matches.f.txt", out_file = "matches.e.txt", poses_file = "relative_poses.json",
              n_txt = "256", t_txt = "2.5", seed_txt, dev_txt = "0", scales_file;
  bool refine = false;
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    std::string *dst = nullptr;
    if (a == "--refine") {
      refine = true;
      continue;
    }
    const size_t eq = a.find('=');
    if (eq != std::string::npos && (a.substr(0, eq) == "--seed" || a.substr(0, eq) == "--device")) {
      (a.substr(0, eq) == "--seed" ? seed_txt : dev_txt) = a.substr(eq + 1);
      continue;
    }
    if (a == "-i" || a == "--input_file") dst = &in;
    else if (a == "-m" || a == "--match_dir") dst = &match_dir;
    else if (a == "-f" || a == "--match_file") dst = &match_file;
    else if (a == "-o" || a == "--output_file") dst = &out_file;
    else if (a == "-p" || a == "--poses_file") dst = &poses_file;
    else if (a == "-n" || a == "--max_iteration") dst = &n_txt;
    else if (a == "-t" || a == "--precision") dst = &t_txt;
    else if (a == "-s" || a == "--scales_file") dst = &scales_file;
    else if (a == "--seed") dst = &seed_txt;
    else if (a == "--device") dst = &dev_txt;
    if (!dst || i + 1 >= argc) {
      usage();
      return 1;
    }
    *dst = argv[++i];
  }
  char *e1 = nullptr, *e2 = nullptr, *e3 = nullptr, *e4 = nullptr;
  const long long max_iteration = strtoll(n_txt.c_str(), &e1, 10);
  const double precision = strtod(t_txt.c_str(), &e2);
  const unsigned long long seed = strtoull(seed_txt.c_str(), &e3, 0);
  const long device = strtol(dev_txt.c_str(), &e4, 10);
  if (n_txt.empty() || t_txt.empty() || dev_txt.empty() || *e1 || *e2 || *e3 || *e4 || in.empty() || match_dir.empty() ||
      max_iteration < 0 || !(precision >= 0.0)) {
    usage();
    return 1;
  }
  Doc d;
  std::string err;
  bool ok = sfmdoc::load(in, true, &d, &err);
  const uint32_t n_views = ok ? (uint32_t)d.view_id.size() : 0;
  const Value *views = ok ? d.root.get("views") : nullptr;
  std::vector<uint32_t> view_wh(2 * (size_t)n_views);
  for (uint32_t k = 0; ok && k < n_views; ++k) {
    const Value *data = sfmdoc::ptr_data(views->a[k].get("value"));
    if (!data || !sfmdoc::num_u32(data->get("width"), &view_wh[2 * k]) ||
        !sfmdoc::num_u32(data->get("height"), &view_wh[2 * k + 1])) {
      ok = false;
      err = "a view without width or height";
    }
  }
  if (!ok) {
    fprintf(stderr, "\nThe input SfM_Data file \"%s\" cannot be read. (%s)\n", in.c_str(), err.c_str());
    return 1;
  }
  std::vector<float> kpt;
  std::vector<uint64_t> view_off(1, 0);
  for (uint32_t k = 0; k < n_views; ++k) {
    const Value *data = sfmdoc::ptr_data(views->a[k].get("value"));
    const Value *fn = data ? data->get("filename") : nullptr;
    const std::string path = join(match_dir, stem_of((fn && fn->kind == Value::Str) ? fn->s : std::string()) + ".feat");
    if (!read_feat(path, &kpt)) {
      fprintf(stderr, "\nInvalid features. (%s cannot be read)\n", path.c_str());
      return 1;
    }
    view_off.push_back(kpt.size() / 2);
  }
  std::map<uint32_t, uint32_t> view_index;
  for (uint32_t k = 0; k < n_views; ++k) view_index[d.view_id[k]] = k;
  PairList all, pl;
  const std::string mpath = join(match_dir, match_file);
  if (!read_matches(mpath, view_index, &all, &err)) {
    fprintf(stderr, "\nInvalid matches file. (%s: %s)\n", mpath.c_str(), err.c_str());
    return 1;
  }
  std::vector<uint32_t> itype(d.intr_type);
  const auto usable = [&](uint32_t v) { return d.intr_type[d.view_intr[v]] == 0 || d.intr_type[d.view_intr[v]] == 3; };
  size_t skipped = 0;
  for (size_t k = 0; k + 1 < all.offsets.size(); ++k) {  // pairs with a view without a usable intrinsic are left out
    const uint32_t a = all.pairs[2 * k], b = all.pairs[2 * k + 1];
    if (!usable(a) || !usable(b)) {
      ++skipped;
      continue;
    }
    pl.pairs.push_back(a);
    pl.pairs.push_back(b);
    pl.mi.insert(pl.mi.end(), all.mi.begin() + all.offsets[k], all.mi.begin() + all.offsets[k + 1]);
    pl.mj.insert(pl.mj.end(), all.mj.begin() + all.offsets[k], all.mj.begin() + all.offsets[k + 1]);
    pl.offsets.push_back(pl.mi.size());
  }
  if (skipped) fprintf(stderr, "%s: %zu pairs skipped: a view without a usable intrinsic\n", kName, skipped);
  for (uint32_t &t : itype)
    if (t != 0 && t != 3) t = 0;
  const uint32_t n_pairs = (uint32_t)(pl.pairs.size() / 2);
  printf("#views: %u; #pairs: %u, #matches: %zu\n", n_views, n_pairs, pl.mi.size());
  fflush(stdout);
  sfmloc_relpose_options opt;
  sfmloc_relpose_default_options(&opt);
  opt.max_iteration = (uint32_t)max_iteration;
  opt.precision_px = precision;
  if (!seed_txt.empty()) opt.seed = seed;
  sfmloc_relpose *h = nullptr;
  if (sfmloc_relative_poses((int)device, view_off.data(), n_views, kpt.data(), view_wh.data(), d.view_intr.data(),
                            d.intr.data(), itype.data(), (uint32_t)itype.size(), pl.pairs.data(), n_pairs, pl.offsets.data(),
                            pl.mi.data(), pl.mj.data(), &opt, &h)) {
    fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
    return 1;
  }
  std::vector<sfmloc_relpose_result> res(n_pairs ? n_pairs : 1);
  std::vector<uint64_t> off((size_t)n_pairs + 1, 0);
  sfmloc_relpose_results(h, res.data());
  sfmloc_relpose_inliers(h, off.data(), nullptr);
  std::vector<uint32_t> idx(off[n_pairs] ? off[n_pairs] : 1);
  sfmloc_relpose_inliers(h, nullptr, idx.data());
  sfmloc_relpose_destroy(h);
  h = nullptr;
  size_t n_ok = 0, n_ess = 0;
  for (uint32_t k = 0; k < n_pairs; ++k)
    if (res[k].ok) {
      ++n_ok;
      n_ess += res[k].n_inliers;
    }
  printf("Relative poses: %zu of %u pairs; %zu essential matches; device %.3f ms\n", n_ok, n_pairs, n_ess,
         sfmloc_relpose_last_ms());
  fflush(stdout);
  // the poses the file and the wedge scales carry: the sample's, or after --refine the refinement's where it moved
  std::vector<double> rel_R(9 * (size_t)n_pairs + 1), rel_t(3 * (size_t)n_pairs + 1), rel_E(9 * (size_t)n_pairs + 1);
  for (uint32_t k = 0; k < n_pairs; ++k) {
    std::copy(res[k].R, res[k].R + 9, rel_R.begin() + 9 * (size_t)k);
    std::copy(res[k].t, res[k].t + 3, rel_t.begin() + 3 * (size_t)k);
    std::copy(res[k].E, res[k].E + 9, rel_E.begin() + 9 * (size_t)k);
  }
  std::vector<sfmloc_relrefine_result> fine;
  if (refine) {  // sfmloc.h "Two-view refinement" on the ok pairs
    std::vector<uint8_t> use(n_pairs ? n_pairs : 1);
    for (uint32_t k = 0; k < n_pairs; ++k) use[k] = res[k].ok ? 1 : 0;
    sfmloc_relrefine *f = nullptr;
    if (sfmloc_refine_relative_poses((int)device, view_off.data(), n_views, kpt.data(), d.view_intr.data(), d.intr.data(),
                                     itype.data(), (uint32_t)itype.size(), pl.pairs.data(), n_pairs, pl.offsets.data(),
                                     pl.mi.data(), pl.mj.data(), rel_R.data(), rel_t.data(), off.data(), idx.data(),
                                     use.data(), nullptr, &f)) {
      fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
      return 1;
    }
    fine.resize(n_pairs ? n_pairs : 1);
    sfmloc_relrefine_results(f, fine.data());
    sfmloc_relrefine_destroy(f);
    size_t count[5] = {0, 0, 0, 0, 0};
    for (uint32_t k = 0; k < n_pairs; ++k) {
      const sfmloc_relrefine_result &q = fine[k];
      if (q.status < 5) ++count[q.status];
      if (q.status != 1 && q.status != 3) continue;
      std::copy(q.R, q.R + 9, rel_R.begin() + 9 * (size_t)k);
      std::copy(q.t, q.t + 3, rel_t.begin() + 3 * (size_t)k);
      std::copy(q.E, q.E + 9, rel_E.begin() + 9 * (size_t)k);
    }
    printf("Two-view refinement: %zu converged, %zu at the step limit, %zu with too few points, %zu not moved, %zu not "
           "asked; device %.3f ms\n", count[1], count[3], count[2], count[4], count[0], sfmloc_relrefine_last_ms());
    fflush(stdout);
  }
  std::string etxt;
  Value list = Value::make_arr();
  for (uint32_t k = 0; k < n_pairs; ++k) {  // (the pair list ascends by (I, J): view ids ascend with the view index)
    const sfmloc_relpose_result &r = res[k];
    if (!r.ok) continue;
    const uint32_t a = pl.pairs[2 * k], b = pl.pairs[2 * k + 1];
    std::vector<std::pair<uint32_t, uint32_t>> ij;
    for (uint64_t p = off[k]; p < off[k + 1]; ++p) ij.emplace_back(pl.mi[pl.offsets[k] + idx[p]], pl.mj[pl.offsets[k] + idx[p]]);
    std::sort(ij.begin(), ij.end());
    etxt += std::to_string(d.view_id[a]) + " " + std::to_string(d.view_id[b]) + "\n" + std::to_string(ij.size()) + "\n";
    for (const auto &m : ij) etxt += std::to_string(m.first) + " " + std::to_string(m.second) + "\n";
    Value front = Value::make_arr();
    for (int c = 0; c < 4; ++c) front.a.push_back(make_int(r.front[c]));
    Value e;
    e.kind = Value::Obj;
    e.o.emplace_back("I", make_int(d.view_id[a]));
    e.o.emplace_back("J", make_int(d.view_id[b]));
    e.o.emplace_back("n_matches", make_int(r.n_matches));
    e.o.emplace_back("n_inliers", make_int(r.n_inliers));
    e.o.emplace_back("R", rows3(&rel_R[9 * (size_t)k]));
    e.o.emplace_back("t", floats(&rel_t[3 * (size_t)k], 3));
    e.o.emplace_back("E", rows3(&rel_E[9 * (size_t)k]));
    e.o.emplace_back("error_max", Value::make_float(r.error_max_px));
    e.o.emplace_back("front", front);
    e.o.emplace_back("choice", make_int(r.choice));
    if (refine) {
      const sfmloc_relrefine_result &q = fine[k];
      Value f;
      f.kind = Value::Obj;
      f.o.emplace_back("status", make_int(q.status));
      f.o.emplace_back("n_used", make_int(q.n_used));
      f.o.emplace_back("steps", make_int(q.steps));
      f.o.emplace_back("cost_initial", Value::make_float(q.cost_initial));
      f.o.emplace_back("cost", Value::make_float(q.cost));
      e.o.emplace_back("refine", f);
    }
    list.a.push_back(e);
  }
  Value doc;
  doc.kind = Value::Obj;
  doc.o.emplace_back("relative_poses", list);
  std::string jtxt;
  sfmjson::dump(doc, &jtxt);
  const std::string epath = join(match_dir, out_file), ppath = join(match_dir, poses_file);
  if (!sfmjson::write_file(epath.c_str(), etxt) || !sfmjson::write_file(ppath.c_str(), jtxt)) {
    fprintf(stderr, "%s: %s or %s cannot be written\n", kName, epath.c_str(), ppath.c_str());
    return 1;
  }
  if (!scales_file.empty()) {  // sfmloc.h "Wedge scales" on the pairs whose translation can be trusted
    std::vector<uint8_t> use(n_pairs ? n_pairs : 1);
    for (uint32_t k = 0; k < n_pairs; ++k) use[k] = res[k].ok && res[k].front[res[k].choice] == res[k].n_inliers;
    sfmloc_wscales_options wopt;
    sfmloc_wscales_default_options(&wopt);
    sfmloc_wscales *w = nullptr;
    if (sfmloc_wedge_scales((int)device, view_off.data(), n_views, kpt.data(), d.view_intr.data(), d.intr.data(),
                            itype.data(), (uint32_t)itype.size(), pl.pairs.data(), n_pairs, pl.offsets.data(), pl.mi.data(),
                            pl.mj.data(), rel_R.data(), rel_t.data(), off.data(), idx.data(), use.data(), &wopt, &w)) {
      fprintf(stderr, "%s: %s\n", kName, sfmloc_last_error());
      return 1;
    }
    uint32_t n_w = 0;
    sfmloc_wscales_report rep;
    sfmloc_wscales_count(w, &n_w);
    std::vector<sfmloc_wscale> rec(n_w ? n_w : 1);
    sfmloc_wscales_read(w, rec.data());
    sfmloc_wscales_report_read(w, &rep);
    sfmloc_wscales_destroy(w);
    printf("Pair scales: %u wedges of %u candidates over %u pairs; device %.3f ms\n", n_w, rep.n_candidates,
           rep.n_pairs_used, sfmloc_wscales_last_ms());
    fflush(stdout);
    PairScales ps;
    ps.min_shared = wopt.min_shared;
    ps.max_shared = wopt.max_shared;
    for (uint32_t i = 0; i < n_w; ++i) {
      const sfmloc_wscale &r = rec[i];
      ps.rec.push_back(PairScale{d.view_id[r.view],
                                 {d.view_id[pl.pairs[2 * (size_t)r.k]], d.view_id[pl.pairs[2 * (size_t)r.k + 1]]},
                                 {d.view_id[pl.pairs[2 * (size_t)r.l]], d.view_id[pl.pairs[2 * (size_t)r.l + 1]]},
                                 r.n_shared, r.ratio});
    }
    const std::string spath = join(match_dir, scales_file);
    if (!write_pair_scales(spath, ps)) {
      fprintf(stderr, "%s: %s cannot be written\n", kName, spath.c_str());
      return 1;
    }
  }
  return 0;
}
