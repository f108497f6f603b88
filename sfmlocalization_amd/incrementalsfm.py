"""openMVG_main_IncrementalSfM over the C ABI: a folder of features and matches becomes a map that is seeded from its best
view pair and grown view by view -- the alternative PyReconstruct/src/reconstructGraph.py:165 names ("matches.f.txt for
incremental reconstruction") for the videos whose pair graph has no triplet, which rotation and translation averaging
(sfmlocalization_amd.globalsfm) cannot pose.

    python -m sfmlocalization_amd.incrementalsfm -i <sfm_data.json> -m <matchDir> -o <outDir>
                                                 [-a <image> -b <image>] [-f 0|1] [--min-seed-inliers 100] [--device 0]

-a and -b fix the initial pair by the views' file names (both or neither); -f 1 also refines the intrinsics in the final
adjustment; both are OpenMVG's switches.  The chain, every step on the device and from the second on one resident
sfmloc_sfm handle:
    1  sfmlocalization_amd.relpose on matches.f.txt -> <outDir>/matches.e.txt, <outDir>/relative_poses.json
    2  sfmloc_seed_scores over the ok pairs (their essential matches are the inliers) and the choice of the seed pair
       (include/sfmloc.h "Seed scores"), or the -a/-b pair if it is ok.  No candidate: "no seed pair: <n> ok pairs, best
       median angle ..." on stderr, exit code 1, and no sfm_data.json is written.
    3  sfmloc_refine_relative_poses on the seed pair alone; the refined R, t where its status is 1 or 3
    4  tracks over all views from the essential matches
    5  the handle with exactly two valid poses: (I, 0) for the pair's first view and (R, -R^T t) for its second
    6  robust triangulation, cleanup at 4.0 px / 2.0 degrees, joint adjustment of rotations, translations and structure,
       cleanup
    7  growth, one round per pass, until a round registers no view or no view is a candidate: best = the largest
       sfmloc_sfm_register_counts over the views without a pose; sfmloc_sfm_register(max_rounds = 1, min_points =
       max(10, ceil(0.75 best) - 1)) -- OpenMVG's rule: resect the views with at least 0.75 of the best view's tracks --
       then the joint adjustment and the cleanup, after every round
    8  a last joint adjustment (with the intrinsics under -f 1) and the cleanup with rm_unstable = 1
    9  <outDir>/sfm_data.json: the structure as sfmlocalization_amd.structure writes it, the extrinsics from the handle,
       the intrinsics from the handle under -f 1.  Views that were never reached stay without a pose (the reference's
       cleanSfM moves them to a map of their own).
The first stage that fails ends the run with its message and its exit code.  Python only, as globalsfm is.
"""
import json
import math
import os
import sys

import numpy as np

from . import fileio, relpose
from .adjust import _intrinsics, sfm_arrays
from .structure import structure_entries, track_arrays, view_files

NAME = "openMVG_main_IncrementalSfM"
MAX_ROUNDS = 1024            # far above any map's: every round but the last registers a view
RESIDUAL_PX, ANGLE_DEG = 4.0, 2.0
USAGE = (f"Usage: {NAME}\n"
         "[-i|--input_file] path to a SfM_Data scene\n"
         "[-m|--matchdir] path to the features and matches that correspond to the provided SfM_Data scene\n"
         "[-o|--outdir] path where the output data will be stored\n"
         "\n[Optional]\n"
         "[-a|--initialPairA] filename of the first image of the initial pair (without path)\n"
         "[-b|--initialPairB] filename of the second image of the initial pair (without path)\n"
         "[-f|--refineIntrinsics] 0: the intrinsics stay as they are (default), 1: the final adjustment refines them\n"
         "[--min-seed-inliers] used inliers a pair needs to seed the map (100)\n"
         "[--device] HIP device (0)\n")


def growth_min_points(best):
    """OpenMVG's "views with at least 0.75 of the best view's tracks" as sfmloc_register_options.min_points, whose test
    is ">"; never below the resection's own 10"""
    return max(10, int(math.ceil(0.75 * best)) - 1)


def seed_scene(doc, arrays, feats, essential, entries):
    """the two-view scene of the ok pairs: every pair of relative_poses.json with its essential matches, all of them
    inliers -> the arguments of capi.SeedScores / capi.RelRefine (without use_pair)"""
    from . import capi as S
    index = {int(v): k for k, v in enumerate(arrays["view_id"])}
    keys = sorted(essential)
    by_key = {(int(e["I"]), int(e["J"])): e for e in entries}
    if sorted(by_key) != keys:
        raise ValueError("relative_poses.json and the essential matches name different pairs")
    pairs, offsets, mi, mj = S.pair_arrays(essential, index)
    off = offsets.astype(np.int64)
    return dict(view_off=np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64),
                kpt_xy=(np.concatenate([f[:, :2] for f in feats]) if feats else np.zeros((0, 2))).astype(np.float32),
                view_intrinsic=arrays["view_intrinsic"], intrinsics=arrays["intrinsic"],
                intrinsic_type=np.where(np.isin(arrays["intrinsic_type"], (0, 3)), arrays["intrinsic_type"], 0).astype(np.uint32),
                pairs=pairs, offsets=offsets, match_i=mi, match_j=mj,
                rel_R=np.array([by_key[k]["R"] for k in keys], np.float64).reshape(-1, 9),
                rel_t=np.array([by_key[k]["t"] for k in keys], np.float64).reshape(-1, 3), inl_off=offsets,
                inl_idx=(np.concatenate([np.arange(off[k + 1] - off[k]) for k in range(len(keys))]) if keys
                         else np.zeros(0)).astype(np.uint32))


def named_pair(doc, pairs, name_a, name_b):
    """the index of the pair whose two views carry the file names name_a and name_b (in either order), or -1"""
    names = [os.path.basename(e["value"]["ptr_wrapper"]["data"]["filename"]) for e in doc["views"]]
    want = {os.path.basename(name_a), os.path.basename(name_b)}
    for k, (a, b) in enumerate(pairs):
        if {names[a], names[b]} == want and names[a] != names[b]:
            return k
    return -1


def seed_poses(arrays, vi, vj, R, t):
    """the pose table with exactly two valid poses: (I, 0) for view vi, (R, -R^T t) for view vj"""
    n = len(arrays["pose_valid"])
    pv, pR, pC = np.zeros(n, np.uint8), np.zeros((n, 9)), np.zeros((n, 3))
    R = np.asarray(R, np.float64).reshape(3, 3)
    pi, pj = int(arrays["view_pose"][vi]), int(arrays["view_pose"][vj])
    pv[[pi, pj]] = 1
    pR[pi], pR[pj] = np.eye(3).reshape(9), R.reshape(9)
    pC[pj] = -(R.T @ np.asarray(t, np.float64))
    return pv, pR, pC


def run(in_path, match_dir, out_dir, pair_a="", pair_b="", refine_intrinsics=False, min_seed_inliers=100, device=0,
        log=print):
    """The tool's body.  Returns 0, or the exit code of the stage that failed after its message on stderr."""
    from . import capi as S
    os.makedirs(out_dir, exist_ok=True)
    essential_path = os.path.join(os.path.abspath(out_dir), "matches.e.txt")
    poses_path = os.path.join(os.path.abspath(out_dir), "relative_poses.json")
    # 1
    rc = relpose.run(in_path, match_dir, out_file=essential_path, poses_file=poses_path, device=device, log=log)
    if rc:
        return rc
    try:
        with open(in_path) as fh:
            doc = json.load(fh)
        arrays, pose_id, _ = sfm_arrays({**doc, "structure": []})
        feats = [fileio.read_feat(os.path.join(match_dir, s + ".feat")) for s in view_files(doc)]
        essential = fileio.read_matches_txt(essential_path)
        with open(poses_path) as fh:
            entries = json.load(fh)["relative_poses"]
        scene = seed_scene(doc, arrays, feats, essential, entries)
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"{NAME}: the relative poses cannot be read back ({e})", file=sys.stderr)
        return 1
    pairs = scene["pairs"]
    h = None
    try:
        # 2
        seeds = S.SeedScores(**scene, device=int(device), min_used=int(min_seed_inliers))
        if pair_a or pair_b:
            k = named_pair(doc, pairs, pair_a, pair_b)
            if k < 0:
                print(f"{NAME}: the initial pair ({pair_a}, {pair_b}) is not among the {len(pairs)} ok pairs", file=sys.stderr)
                return 1
        else:
            k = seeds.choose(arrays["view_pose"])
        if k < 0:
            used = seeds.scores[seeds.scores["n_used"] > 0]
            best = f"{math.degrees(math.acos(float(used['cos_median'].min()))):.3f} degrees" if len(used) else "none"
            print(f"{NAME}: no seed pair: {len(pairs)} ok pairs, best median angle {best}, most used inliers "
                  f"{int(seeds.scores['n_used'].max()) if len(pairs) else 0} (--min-seed-inliers {int(min_seed_inliers)})",
                  file=sys.stderr)
            return 1
        vi, vj = int(pairs[k][0]), int(pairs[k][1])
        sk = seeds.scores[k]
        log(f"Seed pair: views ({int(arrays['view_id'][vi])}, {int(arrays['view_id'][vj])}), {int(sk['n_used'])} of "
            f"{int(sk['n_inliers'])} inliers used, median angle {math.degrees(math.acos(float(sk['cos_median']))):.3f} degrees; "
            f"{int(seeds.scores['candidate'].sum())} candidates of {len(pairs)} ok pairs; device {seeds.ms:.3f} ms")
        # 3
        use = np.zeros(len(pairs), np.uint8)
        use[k] = 1
        fine = S.RelRefine(**scene, use_pair=use, device=int(device)).results[k]
        took = int(fine["status"]) in (1, 3)
        R, t = (fine["R"], fine["t"]) if took else (scene["rel_R"][k], scene["rel_t"][k])
        log(f"Two-view refinement of the seed pair: status {int(fine['status'])}, {int(fine['n_used'])} points, cost "
            f"{float(fine['cost_initial']):g} -> {float(fine['cost']):g}" + ("" if took else "; the sample's pose is kept"))
        # 4, 5
        trk = S.Tracks(scene["view_off"], pairs, scene["offsets"], scene["match_i"], scene["match_j"], min_length=2,
                       device=int(device))
        log(f"Tracks: {trk.counts[0]} components, {trk.counts[1]} dropped for conflict, {trk.counts[2]} dropped for length, "
            f"{trk.counts[3]} kept")
        a = track_arrays(arrays, feats, trk.off, trk.view, trk.feat)
        a["pose_valid"], a["pose_R"], a["pose_C"] = seed_poses(arrays, vi, vj, R, t)
        h = S.Sfm(**a, params=S.sfm_default_params(device=int(device)))
        # 6
        rep = h.triangulate(mode=S.TRI_ROBUST, residual_px=RESIDUAL_PX)
        log(f"Triangulation from the seed pair: {rep.landmarks_kept} of {rep.landmarks_in} tracks kept")
        rst = S.BA_ROTATION | S.BA_TRANSLATION | S.BA_STRUCTURE

        def clean(rm_unstable=False):
            counts = h.clean(RESIDUAL_PX, ANGLE_DEG, rm_unstable)
            log(f"Cleanup: {counts[0]} points, {counts[1]} after the residual filter, {counts[2]} after the angle filter, "
                f"{counts[3]} kept")

        def adjust(what, names):
            jr = h.adjust_joint(what)
            log(f"Bundle adjustment over {names}: cost {jr.cost_initial:g} -> {jr.cost_final:g}, {jr.steps_accepted} of "
                f"{jr.steps_tried} steps")
        clean()
        adjust(rst, "rotations, translations, structure")
        clean()
        # 7
        total = [0, 0, 0]
        for _ in range(MAX_ROUNDS):
            unposed = ~h.read(masks=False)["pose_valid"][arrays["view_pose"]]
            if not unposed.any():
                break
            best = int(h.register_counts()[unposed].max())
            rr = h.register(max_rounds=1, min_points=growth_min_points(best), residual_px=RESIDUAL_PX)
            if rr.rounds == 0:
                break
            log(f"Registration round {total[0]}: best view has {best} tracks, {rr.views_tried} views tried, "
                f"{rr.views_registered} registered, {rr.obs_extended} observations extended, {rr.landmarks_added} of "
                f"{rr.landmarks_tried} landmarks added")
            total = [total[0] + 1, total[1] + rr.views_tried, total[2] + rr.views_registered]
            if rr.views_registered == 0:
                break
            adjust(rst, "rotations, translations, structure")
            clean()
        log(f"Registration: {total[0]} rounds, {total[2]} views registered in {total[1]} tries")
        # 8
        if refine_intrinsics:
            adjust(rst | S.BA_INTRINSICS, "rotations, translations, structure, intrinsics")
        else:
            adjust(rst, "rotations, translations, structure")
        clean(rm_unstable=True)
        q = h.read(masks=True)
        X = h.read_structure()
        K = h.read_intrinsics() if refine_intrinsics else None
    except S.SfmlocError as e:
        print(f"{NAME}: {e.message}", file=sys.stderr)
        return 1
    finally:
        if h is not None:
            h.close()
    # 9
    out = dict(doc)
    out["structure"] = structure_entries(arrays["view_id"], trk.off, trk.view, trk.feat, a["obs_x"], X, q["landmark_keep"],
                                         q["obs_keep"])
    out["extrinsics"] = [{"key": p, "value": {"rotation": [[float(x) for x in row] for row in q["pose_R"][i]],
                                              "center": [float(x) for x in q["pose_C"][i]]}}
                         for i, p in enumerate(pose_id) if q["pose_valid"][i]]
    if K is not None:
        out["intrinsics"] = _intrinsics(doc, arrays, K)
    out["control_points"] = []
    log(f"#views with a pose: {len(out['extrinsics'])} of {len(doc['views'])}; #landmark found: {len(out['structure'])}")
    with open(os.path.join(out_dir, "sfm_data.json"), "w") as fh:
        json.dump(out, fh)
    return 0


def parse_args(argv):
    """-> the keyword arguments of run(), or None for a bad command line"""
    opt = {"-i": "", "-m": "", "-o": "", "-a": "", "-b": "", "-f": "0", "--min-seed-inliers": "100", "--device": "0"}
    long_names = {"--input_file": "-i", "--matchdir": "-m", "--outdir": "-o", "--initialPairA": "-a", "--initialPairB": "-b",
                  "--refineIntrinsics": "-f"}
    i = 0
    while i < len(argv):
        a = argv[i]
        if "=" in a and a.split("=", 1)[0] in ("--min-seed-inliers", "--device"):
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
        kw = dict(in_path=opt["-i"], match_dir=opt["-m"], out_dir=opt["-o"], min_seed_inliers=int(opt["--min-seed-inliers"]),
                  device=int(opt["--device"]))
    except ValueError:
        return None
    if not kw["in_path"] or not kw["match_dir"] or not kw["out_dir"] or opt["-f"] not in ("0", "1") or \
            not 1 <= kw["min_seed_inliers"] <= 0xFFFFFFFF or kw["device"] < 0 or bool(opt["-a"]) != bool(opt["-b"]):
        return None
    if opt["-a"]:
        if os.path.basename(opt["-a"]) == os.path.basename(opt["-b"]):
            return None
        kw["pair_a"], kw["pair_b"] = opt["-a"], opt["-b"]
    if opt["-f"] == "1":
        kw["refine_intrinsics"] = True
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
