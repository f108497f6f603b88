"""openMVG_main_ComputeStructureFromKnownPoses over the C ABI: the structure of a map rebuilt from its poses and the
pairwise matches -- the last stage of openMVG_main_GlobalSfM (PyReconstruct/src/reconstructGraph.py:171), which no other
tool here can stand in for: feature tracks from matches.f.txt, every track triangulated from the views' known poses.

    python -m sfmlocalization_amd.structure -i <sfm_data.json> -m <matchDir> [-f <match file = matches.f.txt>]
                                            -o <out sfm_data.json> [-r <residual px = 4.0>] [-a <min angle deg = 2.0>]
                                            [-b] [--blind] [--register] [--device=0]

The views, intrinsics and extrinsics come from the input; its own structure is ignored.  <matchDir>/<stem>.feat of every
view gives the view's features and their pixels, the match file (relative to <matchDir> unless absolute) the pairs.
Views without a pose are masked out of the tracks.  Then, on one resident sfmloc_sfm: sfmloc_sfm_triangulate (robust, or
the N-view solve alone with --blind), sfmloc_sfm_clean(r, a, 0), and with -b the structure adjustment (OpenMVG_BA -c=s)
followed by a second cleanup.  The output is the input document with `structure` replaced -- the kept landmarks with
keys 0, 1, 2, ... in track order, every kept observation with its id_feat and the .feat pixel -- and control_points [],
written with json.dump.  bin/openMVG_main_ComputeStructureFromKnownPoses (csrc/structure_cli.cpp) is the same program
and writes the same bytes.  The semantics are stated in include/sfmloc.h.

--register grows the map to the views without a pose (sfmloc_sfm_register): the tracks are built over ALL views, and after
the triangulation and its cleanup every view without a pose is resected against the kept structure, the structure takes in
its observations and the landmarks it makes triangulable, round after round (at most 16), and the structure is cleaned
again; -b and its cleanup follow.  The output's `extrinsics` are then written from the handle: every valid pose, the new
ones included.  A difference to the masked build: with the unposed views in the tracks, the conflict rule sees their
features too, so a wrong match of an unposed view can drop a component that the masked build would have kept.
"""
import json
import os
import sys

import numpy as np

from . import fileio
from .adjust import sfm_arrays

NAME = "openMVG_main_ComputeStructureFromKnownPoses"
REGISTER_ROUNDS = 16          # sfmloc_register_options.max_rounds' default
USAGE = (f"Usage: {NAME}\n"
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
         "             built over all views: a wrong match of an unposed view can drop a track the masked build keeps)\n")


def view_files(doc):
    """-> the .feat stem of every view, in view order (the view's filename without directory and extension)"""
    return [os.path.splitext(os.path.basename(e["value"]["ptr_wrapper"]["data"]["filename"]))[0] for e in doc["views"]]


def track_arrays(arrays, feats, off, view, feat):
    """the arrays of sfmloc_sfm_desc for tracks: landmark ids 0, 1, 2, ..., X zero, the observations' .feat pixels"""
    out = dict(arrays)
    n = len(off) - 1
    out["landmark_id"] = np.arange(n, dtype=np.uint32)
    out["landmark_X"] = np.zeros((n, 3))
    out["obs_off"] = np.asarray(off, np.uint64)
    out["obs_view"] = np.asarray(view, np.uint32)
    x = np.zeros((len(view), 2))
    for k in range(len(feats)):
        sel = np.nonzero(out["obs_view"] == k)[0]
        if len(sel):
            x[sel] = feats[k][np.asarray(feat)[sel], :2].astype(np.float64)
    out["obs_x"] = x
    return out


def structure_entries(view_id, off, view, feat, obs_x, X, landmark_keep, obs_keep):
    """the `structure` list of the output: kept landmarks, keys 0, 1, 2, ... in track order"""
    out = []
    for l in range(len(off) - 1):
        if not landmark_keep[l]:
            continue
        obs = [{"key": int(view_id[view[o]]), "value": {"id_feat": int(feat[o]), "x": [float(obs_x[o][0]), float(obs_x[o][1])]}}
               for o in range(int(off[l]), int(off[l + 1])) if obs_keep[o]]
        out.append({"key": len(out), "value": {"X": [float(x) for x in X[l]], "observations": obs}})
    return out


def run(in_path, match_dir, out_path, match_file="matches.f.txt", residual_px=4.0, angle_deg=2.0, adjust=False,
        blind=False, device=0, log=print, joint=False, register=False):
    """The tool's body.  Returns 0, or 1 after an error message on stderr.  joint (no command-line switch: what
    sfmlocalization_amd.globalsfm asks for): after the cleanup, rotations, translations and structure adjusted as one
    problem on the same resident handle (sfmloc_sfm_adjust_joint), cleaned again, and the poses written from it.
    register: the --register switch."""
    from . import capi as S
    try:
        with open(in_path) as fh:
            doc = json.load(fh)
        arrays, pose_id, _ = sfm_arrays({**doc, "structure": []})
        stems = view_files(doc)
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nThe input SfM_Data file \"{in_path}\" cannot be read. ({e})", file=sys.stderr)
        return 1
    try:
        feats = [fileio.read_feat(os.path.join(match_dir, s + ".feat")) for s in stems]
    except (OSError, ValueError) as e:
        print(f"\nInvalid features. ({e})", file=sys.stderr)
        return 1
    path = match_file if os.path.isabs(match_file) else os.path.join(match_dir, match_file)
    try:
        matches = fileio.read_matches_txt(path)
        index = {int(v): k for k, v in enumerate(arrays["view_id"])}
        pairs, offsets, mi, mj = S.pair_arrays(matches, index)
    except (OSError, ValueError, KeyError, IndexError) as e:
        print(f"\nInvalid matches file. ({path}: {e})", file=sys.stderr)
        return 1
    view_off = np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64)
    view_use = arrays["pose_valid"][arrays["view_pose"]].astype(np.uint8)
    log(f"#views: {len(stems)}, with a pose: {int(view_use.sum())}; #pairs: {len(pairs)}, #matches: {len(mi)}")
    h = None
    try:
        t = S.Tracks(view_off, pairs, offsets, mi, mj, view_use=None if register else view_use, min_length=2,
                     device=int(device))
        log(f"Tracks: {t.counts[0]} components, {t.counts[1]} dropped for conflict, {t.counts[2]} dropped for length, "
            f"{t.counts[3]} kept")
        a = track_arrays(arrays, feats, t.off, t.view, t.feat)
        h = S.Sfm(**a, params=S.sfm_default_params(device=int(device)))
        rep = h.triangulate(mode=S.TRI_BLIND if blind else S.TRI_ROBUST, residual_px=float(residual_px))
        log(f"Triangulation: {rep.landmarks_in} tracks, {rep.landmarks_kept} kept; failed: {rep.failed_posed} too few "
            f"posed observations, {rep.failed_hypothesis} no valid hypothesis, {rep.failed_inliers} too few inliers; "
            f"{rep.obs_kept} of {rep.obs_in} observations kept; {rep.rounds} rounds")

        def clean():
            counts = h.clean(float(residual_px), float(angle_deg), False)
            log(f"Number of points before cleanup : {counts[0]}")
            log(f"Number of points residual error : {counts[1]}")
            log(f"Number of points angle error : {counts[2]}")
            log(f"Number of points after cleanup : {counts[3]}")
        clean()
        if register:
            total = [0, 0, 0, 0, 0]
            for _ in range(REGISTER_ROUNDS):        # (one round per call: the handle numbers them on)
                rr = h.register(max_rounds=1, residual_px=float(residual_px))
                if rr.rounds == 0:
                    break
                log(f"Registration round {total[0]}: {rr.views_tried} views tried, {rr.views_registered} registered, "
                    f"{rr.obs_extended} observations extended, {rr.landmarks_added} of {rr.landmarks_tried} landmarks added")
                total = [total[0] + 1, total[1] + rr.views_tried, total[2] + rr.views_registered,
                         total[3] + rr.obs_extended, total[4] + rr.landmarks_added]
                if rr.views_registered == 0:
                    break
            log(f"Registration: {total[0]} rounds, {total[2]} views registered in {total[1]} tries, {total[3]} "
                f"observations extended, {total[4]} landmarks added")
            clean()
        if adjust:
            ba = h.adjust(S.BA_STRUCTURE)
            log(f"Bundle adjustment over structure: {ba.n_blocks} landmarks, cost {ba.cost_initial:g} -> {ba.cost_final:g}")
            clean()
        if joint:
            jr = h.adjust_joint(S.BA_ROTATION | S.BA_TRANSLATION | S.BA_STRUCTURE)
            log(f"Bundle adjustment over rotations, translations, structure: cost {jr.cost_initial:g} -> "
                f"{jr.cost_final:g}, {jr.steps_accepted} of {jr.steps_tried} steps")
            clean()
        q = h.read(masks=True)
        X = h.read_structure()
    except S.SfmlocError as e:
        print(f"{NAME}: {e.message}", file=sys.stderr)
        return 1
    finally:
        if h is not None:
            h.close()
    out = dict(doc)
    out["structure"] = structure_entries(arrays["view_id"], t.off, t.view, t.feat, a["obs_x"], X, q["landmark_keep"],
                                         q["obs_keep"])
    if joint or register:
        out["extrinsics"] = [{"key": p, "value": {"rotation": [[float(x) for x in row] for row in q["pose_R"][i]],
                                                  "center": [float(x) for x in q["pose_C"][i]]}}
                             for i, p in enumerate(pose_id) if q["pose_valid"][i]]
    out["control_points"] = []
    log(f"#landmark found: {len(out['structure'])}")
    with open(out_path, "w") as fh:
        json.dump(out, fh)
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    opt = {"-i": "", "-m": "", "-o": "", "-f": "matches.f.txt", "-r": "4.0", "-a": "2.0"}
    long_names = {"--input_file": "-i", "--match_dir": "-m", "--output_file": "-o", "--match_file": "-f",
                  "--residual_threshold": "-r", "--min_angle": "-a"}
    adjust, blind, device, register = False, False, 0, False
    i = 0
    while i < len(argv):
        a = long_names.get(argv[i], argv[i])
        if a in opt:
            if i + 1 >= len(argv):
                sys.stderr.write(USAGE)
                return 1
            opt[a] = argv[i + 1]
            i += 1
        elif a in ("-b", "--bundle_adjustment"):
            adjust = True
        elif a == "--blind":
            blind = True
        elif a == "--register":
            register = True
        elif a.startswith("--device="):
            device = int(a.split("=", 1)[1])
        else:
            sys.stderr.write(USAGE)
            return 1
        i += 1
    try:
        residual_px, angle_deg = float(opt["-r"]), float(opt["-a"])
    except ValueError:
        sys.stderr.write(USAGE)
        return 1
    if not opt["-i"] or not opt["-m"] or not opt["-o"]:
        sys.stderr.write(USAGE)
        return 1

    def log(s):
        print(s, flush=True)
    return run(opt["-i"], opt["-m"], opt["-o"], match_file=opt["-f"], residual_px=residual_px, angle_deg=angle_deg,
               adjust=adjust, blind=blind, device=device, log=log, **({"register": True} if register else {}))


if __name__ == "__main__":
    sys.exit(main())
