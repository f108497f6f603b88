"""ComputeGlobalPoses over the C ABI: rotation and translation averaging over the relative poses of the view pairs -- the
middle stage of openMVG_main_GlobalSfM, between sfmlocalization_amd.relpose and sfmlocalization_amd.structure.

    python -m sfmlocalization_amd.globalposes -i <sfm_data.json> -p <relative_poses.json> -o <out sfm_data.json>
                                              [--triplet-angle 5] [--device 0] [-r <report.json>]
                                              [-s <pair_scales.json>]

The views come from the input as sfmlocalization_amd.relpose reads them; the poses file is the one that tool writes.  I
and J are view ids and are mapped to view indices; a pair carries its translation when every inlier lay in front of both
cameras (front[choice] == n_inliers: the advice of include/sfmloc.h "decision").  sfmloc_global_poses (include/sfmloc.h
"Global poses" states the semantics and the known limit on collinear cameras) runs on that.  The output is the input
document with `extrinsics` replaced by the poses of the component's views, keyed by id_pose, as rotation and center,
and `structure` and `control_points` emptied, written by the writer of sfmlocalization_amd.adjust.  -s: the wedge ratios
that `ComputeRelativePoses -s` wrote; a record's two pairs, named by view ids, are looked up in the poses file, and
sfmloc_global_poses_scaled ("Scaled global poses": the spacing along a line of cameras is fixed from the ratios; a pair
with no used wedge drops out of the translations) runs in place of sfmloc_global_poses; the report then also holds
`scale` (sfmloc_gpscale_report) and `baselines` (per pair, in the poses file's order).  One summary line:
views in the component, pairs kept, steps, device milliseconds.  No component (no triplet passes): a message, exit 1.
bin/ComputeGlobalPoses (csrc/globalposes_cli.cpp) is the same program and writes the same bytes.
"""
import json
import sys

import numpy as np

from .adjust import _write, sfm_arrays

NAME = "ComputeGlobalPoses"
USAGE = (f"Usage: {NAME}\n"
         "[-i|--input_file] path to a SfM_Data scene\n"
         "[-p|--poses_file] the relative poses of its view pairs (relative_poses.json of ComputeRelativePoses)\n"
         "[-o|--output_file] the SfM_Data scene to write\n"
         "\n[Optional]\n"
         "[--triplet-angle] largest angle of a triplet's cycle rotation in degrees (5)\n"
         "[-r|--report_file] the call's report as JSON\n"
         "[-s|--scales_file] the wedge ratios (pair_scales.json of ComputeRelativePoses -s): fix the pair baselines from them\n"
         "[--device] HIP device (0)\n")

REPORT_FIELDS = ("n_views", "n_pairs", "n_triplets", "n_triplets_ok", "n_pairs_kept", "n_component_views", "root",
                 "n_rotation_pairs", "n_translation_pairs", "chordal_pcg", "chordal_stop", "rot_steps_tried",
                 "rot_steps_accepted", "rot_pcg_total", "rot_stop", "trans_steps_tried", "trans_steps_accepted",
                 "trans_pcg_total", "trans_stop", "launches", "chordal_residual", "chordal_cost", "rot_cost_initial", "rot_cost_final",
                 "trans_cost_initial", "trans_cost_final", "graph_ms", "rotation_ms", "translation_ms", "device_ms")


SCALE_REPORT_FIELDS = ("n_wedges", "n_wedges_used", "n_scaled_pairs", "n_scaled_views", "first_pair", "steps_tried",
                       "steps_accepted", "pcg_total", "stop", "launches", "cost_initial", "cost_final", "scale_ms", "centre_ms")


def wedge_arrays(records, entries):
    """the records of fileio.read_pair_scales and the `relative_poses` list -> kl [W, 2] (positions in that list),
    ratio [W]; KeyError on a pair of view ids the list does not have"""
    index = {(int(e["I"]), int(e["J"])): k for k, e in enumerate(entries)}
    kl = np.array([[index[tuple(k)], index[tuple(l)]] for _, k, l, _, _ in records], np.uint32).reshape(-1, 2)
    return kl, np.array([q for _, _, _, _, q in records], np.float64)


def pose_arrays(entries, view_id):
    """the `relative_poses` list -> pairs [P, 2] (view indices), rel_R [P, 3, 3], rel_t [P, 3], use_t [P]; KeyError on a
    view id the scene does not have"""
    index = {int(v): k for k, v in enumerate(view_id)}
    pairs = np.array([[index[int(e["I"])], index[int(e["J"])]] for e in entries], np.uint32).reshape(-1, 2)
    rel_R = np.array([e["R"] for e in entries], np.float64).reshape(-1, 3, 3)
    rel_t = np.array([e["t"] for e in entries], np.float64).reshape(-1, 3)
    use_t = np.array([int(e["front"][int(e["choice"])]) == int(e["n_inliers"]) for e in entries], np.uint8)
    return pairs, rel_R, rel_t, use_t


def extrinsics(view_pose_id, in_component, R, C):
    """the `extrinsics` list: the component's poses in ascending id_pose (the first view of a shared pose gives it)"""
    poses = {}
    for v in np.nonzero(in_component)[0]:
        poses.setdefault(int(view_pose_id[v]), {"rotation": [[float(x) for x in row] for row in R[v]],
                                                "center": [float(x) for x in C[v]]})
    return [{"key": p, "value": poses[p]} for p in sorted(poses)]


def run(in_path, poses_path, out_path, triplet_angle=5.0, report_path=None, device=0, log=print, scales_path=None):
    """The tool's body.  Returns 0, or 1 after an error message on stderr."""
    from . import capi as S
    from . import fileio
    try:
        with open(in_path) as fh:
            doc = json.load(fh)
        arrays, _, _ = sfm_arrays({**doc, "structure": []})
        view_pose_id = [int(e["value"]["ptr_wrapper"]["data"]["id_pose"]) for e in doc["views"]]
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nThe input SfM_Data file \"{in_path}\" cannot be read. ({e})", file=sys.stderr)
        return 1
    try:
        with open(poses_path) as fh:
            entries = json.load(fh)["relative_poses"]
        pairs, rel_R, rel_t, use_t = pose_arrays(entries, arrays["view_id"])
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nInvalid relative poses file. ({poses_path}: {e})", file=sys.stderr)
        return 1
    wedges = None
    if scales_path:
        try:
            wedges = wedge_arrays(fileio.read_pair_scales(scales_path)[0], entries)
        except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
            print(f"\nInvalid pair scales file. ({scales_path}: {e})", file=sys.stderr)
            return 1
    log(f"#views: {len(view_pose_id)}; #pairs: {len(pairs)}, with a translation: {int(use_t.sum())}")
    try:
        g = S.GlobalPoses(len(view_pose_id), pairs, rel_R, rel_t, use_t, device=int(device),
                          wedges=wedges, triplet_angle_deg=float(triplet_angle))
    except S.SfmlocError as e:
        print(f"{NAME}: {e.message}", file=sys.stderr)
        return 1
    rep = g.report
    if report_path:
        with open(report_path, "w") as fh:
            out = {k: getattr(rep, k) for k in REPORT_FIELDS}
            if wedges is not None:
                out["scale"] = {k: getattr(g.scale_report, k) for k in SCALE_REPORT_FIELDS}
                out["baselines"] = [float(b) for b in g.baselines]
            json.dump(out, fh)
    if not rep.n_component_views:
        why = "no triplet" if wedges is None or not rep.n_pairs_kept else "no wedge"
        print(f"{NAME}: {why} of the {len(pairs)} pairs passes: no view can be posed", file=sys.stderr)
        return 1
    if wedges is not None:
        sr = g.scale_report
        log(f"Pair scales: {sr.n_wedges_used} of {sr.n_wedges} wedges used; {sr.n_scaled_pairs} pairs, {sr.n_scaled_views} "
            f"views; steps {sr.steps_accepted}/{sr.steps_tried}")
    log(f"Global poses: {rep.n_component_views} of {rep.n_views} views; {rep.n_pairs_kept} of {rep.n_pairs} pairs kept; "
        f"steps: rotation {rep.rot_steps_accepted}/{rep.rot_steps_tried}, translation "
        f"{rep.trans_steps_accepted}/{rep.trans_steps_tried}; device {rep.device_ms:.3f} ms")
    out = dict(doc)
    out["extrinsics"] = extrinsics(view_pose_id, g.in_component, g.R, g.C)
    out["structure"] = []
    out["control_points"] = []
    _write(out_path, out)
    return 0


def parse_args(argv):
    """-> the keyword arguments of run(), or None for a bad command line"""
    opt = {"-i": "", "-p": "", "-o": "", "-r": "", "-s": "", "--triplet-angle": "5", "--device": "0"}
    long_names = {"--input_file": "-i", "--poses_file": "-p", "--output_file": "-o", "--report_file": "-r",
                  "--scales_file": "-s"}
    i = 0
    while i < len(argv):
        a = argv[i]
        if "=" in a and a.split("=", 1)[0] in ("--triplet-angle", "--device"):
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
        kw = dict(in_path=opt["-i"], poses_path=opt["-p"], out_path=opt["-o"], triplet_angle=float(opt["--triplet-angle"]),
                  report_path=opt["-r"] or None, device=int(opt["--device"]))
        if opt["-s"]:
            kw["scales_path"] = opt["-s"]    # (only when given: without the switch the call is what it was)
    except ValueError:
        return None
    if not kw["in_path"] or not kw["poses_path"] or not kw["out_path"] or not 0.0 < kw["triplet_angle"] < 180.0:
        return None
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
