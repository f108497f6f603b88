"""ComputeRelativePoses over the C ABI: the relative pose of every matched view pair -- the first stage of
openMVG_main_GlobalSfM and the essential filter the reference skips (PyReconstruct/src/reconstructGraph.py:165-166 copies
matches.f.txt to matches.e.txt "because OpenMVG assumes matches.e.txt for global reconstruction").

    python -m sfmlocalization_amd.relpose -i <sfm_data.json> -m <matchDir> [-f <match file = matches.f.txt>]
                                          [-o <essential matches = matches.e.txt>] [-p <poses = relative_poses.json>]
                                          [-n <iterations = 256>] [-t <precision px = 2.5>] [--seed N] [--device 0]
                                          [-s <pair scales = none>] [--refine]

The views and intrinsics come from the input, <matchDir>/<stem>.feat of every view gives its keypoints, the match file
(relative to <matchDir> unless absolute, as the two outputs are) the pairs: all read as sfmlocalization_amd.structure
does.  A pair with a view whose intrinsic is neither pinhole nor pinhole_radial_k3 is skipped and counted on stderr.
sfmloc_relative_poses (include/sfmloc.h "Relative poses" states the semantics) runs on the rest.  The essential matches
hold the ok pairs only, each with its inliers in ascending (i, j); the poses file is
{"relative_poses": [{"I", "J", "n_matches", "n_inliers", "R", "t", "E", "error_max", "front", "choice"}, ...]} in
ascending (I, J), I and J view ids, R and E as three rows, written with json.dump.  bin/ComputeRelativePoses
(csrc/relpose_cli.cpp) is the same program and writes the same bytes.  sfmlocalization_amd.globalposes consumes the
poses file (rotation and translation averaging).  Without --refine R and t are those of the winning minimal sample.  With
--refine, sfmloc_refine_relative_poses ("Two-view refinement": OpenMVG's adjustment of every pair on its inliers) runs on
the ok pairs: every entry gains "refine": {"status", "n_used", "steps", "cost_initial", "cost"} and carries the refined
R, t and E where the status is 1 or 3; n_inliers, front, choice and the essential matches stay the sample's.  With -s,
sfmloc_wedge_scales ("Wedge scales") runs on the call's results -- the pairs with ok and front[choice] == n_inliers, under
the refined poses after --refine -- and its records are written by view ids (fileio.write_pair_scales), by both programs
with the same bytes.
"""
import json
import os
import sys

import numpy as np

from . import fileio
from .adjust import sfm_arrays
from .structure import view_files

NAME = "ComputeRelativePoses"
USAGE = (f"Usage: {NAME}\n"
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
         "[--refine] adjust every ok pair's pose on its inliers\n")


def view_sizes(doc):
    """-> [n_views, 2] uint32: width and height of every view, in view order"""
    return np.array([[int(e["value"]["ptr_wrapper"]["data"]["width"]), int(e["value"]["ptr_wrapper"]["data"]["height"])]
                     for e in doc["views"]], np.uint32).reshape(-1, 2)


def pose_entries(view_id, pairs, results, refined=None):
    """the `relative_poses` list: the ok pairs, ascending (I, J).  refined (RELREFINE_RESULT per pair, or None): every
    entry gains "refine", and R, t and E are the refinement's where its status is 1 or 3"""
    out = []
    for k, ((a, b), r) in enumerate(zip(pairs, results)):
        if not int(r["ok"]):
            continue
        p = r if refined is None or int(refined[k]["status"]) not in (1, 3) else refined[k]
        out.append({"I": int(view_id[a]), "J": int(view_id[b]), "n_matches": int(r["n_matches"]),
                    "n_inliers": int(r["n_inliers"]), "R": [[float(x) for x in p["R"][3 * i:3 * i + 3]] for i in range(3)],
                    "t": [float(x) for x in p["t"]], "E": [[float(x) for x in p["E"][3 * i:3 * i + 3]] for i in range(3)],
                    "error_max": float(r["error_max_px"]), "front": [int(x) for x in r["front"]],
                    "choice": int(r["choice"])})
        if refined is not None:
            f = refined[k]
            out[-1]["refine"] = {"status": int(f["status"]), "n_used": int(f["n_used"]), "steps": int(f["steps"]),
                                 "cost_initial": float(f["cost_initial"]), "cost": float(f["cost"])}
    return out


def refined_poses(results, refined):
    """(R [P, 9], t [P, 3]): the refinement's where its status is 1 or 3, the sample's otherwise"""
    took = np.isin(refined["status"], (1, 3))
    return np.where(took[:, None], refined["R"], results["R"]), np.where(took[:, None], refined["t"], results["t"])


def scale_pairs(results):
    """the pairs whose translation can be trusted ("decision" of the relative poses): ok and every inlier in front"""
    return np.array([int(r["ok"]) and int(r["front"][int(r["choice"])]) == int(r["n_inliers"]) for r in results], np.uint8)


def scale_entries(view_id, pairs, records):
    """the records of WedgeScales by view ids, as fileio.write_pair_scales takes them"""
    def ids(k):
        return int(view_id[pairs[k][0]]), int(view_id[pairs[k][1]])
    return [(int(view_id[r["view"]]), ids(int(r["k"])), ids(int(r["l"])), int(r["n_shared"]), float(r["ratio"]))
            for r in records]


def essential_matches(view_id, pairs, offsets, match_i, match_j, rp):
    """{(I, J): (i[], j[])} of the ok pairs: the inliers, ascending (i, j)"""
    out = {}
    for k, (a, b) in enumerate(pairs):
        if not int(rp.results[k]["ok"]):
            continue
        sel = int(offsets[k]) + rp.inliers(k).astype(np.int64)
        ij = sorted(zip(match_i[sel].tolist(), match_j[sel].tolist()))
        out[(int(view_id[a]), int(view_id[b]))] = (np.array([x for x, _ in ij], np.uint32),
                                                   np.array([y for _, y in ij], np.uint32))
    return out


def run(in_path, match_dir, match_file="matches.f.txt", out_file="matches.e.txt", poses_file="relative_poses.json",
        max_iteration=256, precision_px=2.5, seed=None, device=0, log=print, scales_file=None, refine=False):
    """The tool's body.  Returns 0, or 1 after an error message on stderr."""
    from . import capi as S
    try:
        with open(in_path) as fh:
            doc = json.load(fh)
        arrays, _, _ = sfm_arrays({**doc, "structure": []})
        stems = view_files(doc)
        view_wh = view_sizes(doc)
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nThe input SfM_Data file \"{in_path}\" cannot be read. ({e})", file=sys.stderr)
        return 1
    try:
        feats = [fileio.read_feat(os.path.join(match_dir, s + ".feat")) for s in stems]
    except (OSError, ValueError) as e:
        print(f"\nInvalid features. ({e})", file=sys.stderr)
        return 1

    def at(p):
        return p if os.path.isabs(p) else os.path.join(match_dir, p)
    path = at(match_file)
    try:
        matches = fileio.read_matches_txt(path)
        index = {int(v): k for k, v in enumerate(arrays["view_id"])}
        usable = np.isin(arrays["intrinsic_type"], (0, 3))[arrays["view_intrinsic"]]
        kept = {k: v for k, v in matches.items() if usable[index[k[0]]] and usable[index[k[1]]]}
        pairs, offsets, mi, mj = S.pair_arrays(kept, index)
    except (OSError, ValueError, KeyError, IndexError) as e:
        print(f"\nInvalid matches file. ({path}: {e})", file=sys.stderr)
        return 1
    if len(kept) != len(matches):
        print(f"{NAME}: {len(matches) - len(kept)} pairs skipped: a view without a usable intrinsic", file=sys.stderr)
    view_off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64)
    kpt = (np.concatenate([f[:, :2] for f in feats]) if feats else np.zeros((0, 2))).astype(np.float32)
    itype = np.where(np.isin(arrays["intrinsic_type"], (0, 3)), arrays["intrinsic_type"], 0).astype(np.uint32)
    log(f"#views: {len(stems)}; #pairs: {len(pairs)}, #matches: {len(mi)}")
    options = dict(max_iteration=int(max_iteration), precision_px=float(precision_px))
    if seed is not None:
        options["seed"] = int(seed)
    try:
        rp = S.RelPoses(view_off, kpt, view_wh, arrays["view_intrinsic"], arrays["intrinsic"], itype, pairs, offsets, mi, mj,
                        device=int(device), **options)
    except S.SfmlocError as e:
        print(f"{NAME}: {e.message}", file=sys.stderr)
        return 1
    n_ok = int(sum(int(r["ok"]) for r in rp.results))
    log(f"Relative poses: {n_ok} of {len(pairs)} pairs; {int(sum(int(r['n_inliers']) for r in rp.results if r['ok']))} "
        f"essential matches; device {rp.ms:.3f} ms")
    rel_R, rel_t, refined = rp.results["R"], rp.results["t"], None
    if refine:
        try:
            rr = S.RelRefine(view_off, kpt, arrays["view_intrinsic"], arrays["intrinsic"], itype, pairs, offsets, mi, mj,
                             rel_R, rel_t, rp.inl_off, rp.inl_idx, use_pair=rp.results["ok"], device=int(device))
        except S.SfmlocError as e:
            print(f"{NAME}: {e.message}", file=sys.stderr)
            return 1
        refined = rr.results
        rel_R, rel_t = refined_poses(rp.results, refined)
        count = [int(np.sum(refined["status"] == s)) for s in range(5)]
        log(f"Two-view refinement: {count[1]} converged, {count[3]} at the step limit, {count[2]} with too few points, "
            f"{count[4]} not moved, {count[0]} not asked; device {rr.ms:.3f} ms")
    fileio.write_matches_txt(at(out_file), essential_matches(arrays["view_id"], pairs, offsets, mi, mj, rp))
    with open(at(poses_file), "w") as fh:
        json.dump({"relative_poses": pose_entries(arrays["view_id"], pairs, rp.results, refined)}, fh)
    if scales_file:
        try:
            ws = S.WedgeScales(view_off, kpt, arrays["view_intrinsic"], arrays["intrinsic"], itype, pairs, offsets, mi, mj,
                               rel_R, rel_t, rp.inl_off, rp.inl_idx, use_pair=scale_pairs(rp.results),
                               device=int(device))
        except S.SfmlocError as e:
            print(f"{NAME}: {e.message}", file=sys.stderr)
            return 1
        log(f"Pair scales: {len(ws.records)} wedges of {ws.report.n_candidates} candidates over {ws.report.n_pairs_used} "
            f"pairs; device {ws.ms:.3f} ms")
        opt = S.wscales_default_options()
        fileio.write_pair_scales(at(scales_file), scale_entries(arrays["view_id"], pairs, ws.records), opt.min_shared,
                                 opt.max_shared)
    return 0


def parse_args(argv):
    """-> the keyword arguments of run(), or None for a bad command line"""
    opt = {"-i": "", "-m": "", "-f": "matches.f.txt", "-o": "matches.e.txt", "-p": "relative_poses.json", "-n": "256",
           "-t": "2.5", "--seed": "", "--device": "0", "-s": ""}
    long_names = {"--input_file": "-i", "--match_dir": "-m", "--match_file": "-f", "--output_file": "-o",
                  "--poses_file": "-p", "--max_iteration": "-n", "--precision": "-t", "--scales_file": "-s"}
    i, refine = 0, False
    while i < len(argv):
        a = argv[i]
        if a == "--refine":
            refine = True
            i += 1
            continue
        if "=" in a and a.split("=", 1)[0] in ("--seed", "--device"):
            a, val = a.split("=", 1)
        else:
            a = long_names.get(a, a)
            if a not in opt or i + 1 >= len(argv):
                return None
            val = argv[i + 1]
            i += 1
        opt[a] = val
        i += 1
    try:
        kw = dict(in_path=opt["-i"], match_dir=opt["-m"], match_file=opt["-f"], out_file=opt["-o"], poses_file=opt["-p"],
                  max_iteration=int(opt["-n"]), precision_px=float(opt["-t"]),
                  seed=int(opt["--seed"], 0) if opt["--seed"] else None, device=int(opt["--device"]))
    except ValueError:
        return None
    if not kw["in_path"] or not kw["match_dir"] or kw["max_iteration"] < 0 or not kw["precision_px"] >= 0.0:
        return None
    if opt["-s"]:
        kw["scales_file"] = opt["-s"]
    if refine:
        kw["refine"] = True
    return kw


def main(argv=None):
    kw = parse_args(sys.argv[1:] if argv is None else list(argv))
    if kw is None:
        sys.stderr.write(USAGE)
        return 1

    def log(s):
        print(s, flush=True)
    return run(log=log, **kw)


if __name__ == "__main__":
    sys.exit(main())
