"""Fixing a map to world coordinates: PyEvaluateAccuracy/src/localizeGlobalCoordinate.py (reference images) and
localizeGlobalCoordinateRefPoint.py (reference landmarks, --reduce-points) over the C ABI -- the step of the reference's
map pipeline between OpenMVG_BA and the server, which reads the Amat.yml written here (LocalizeEngine's AmatFile).

    python -m sfmlocalization_amd.globalcoord <project_dir> <matches_dir> <sfm_data_dir> [-t test_project_dir]
                                              [-o loc_global.json] [--bow] [--reduce-points] [--ref-points]
                                              [--model=similarity|affine] [--seed=N] [--device=0] [--ply]

  1. Amat (3 x 4, world ~ Amat [map; 1]) by RANSAC (sfmloc_merge_ransac, 1000 rounds) over <project_dir>/Ref: with
     --ref-points the landmarks of Ref/refpoints.json ({"refpoints": [{"key": landmark, "X": world}, ...]}) against
     their X in sfm_data.json; otherwise Ref/inputImg is localised into Ref/loc and the centres of the frames named in
     Ref/refcoor.txt ("name x y z" per line) are the map side.  Ref/Amat.txt (np.savetxt) and Ref/Amat.yml are written;
     an Amat.txt already there is loaded and nothing is refitted.
  2. --reduce-points: landmarks closer than 1 cm in world coordinates are folded into the one of lowest index
     (sfmloc_reduce_points); sfm_data.json is rewritten, the original kept as sfm_data_b4rp.json.
  3. sfm_data_global.json: the map in world coordinates (sfmloc_merge_transform).
     --ply: colorized_global.ply, colorized_global_camera.ply and colorized_global_structure.ply beside it
     (localizeGlobalCoordinate.py:229-231, through sfmlocalization_amd.colorize); the images of the map must be readable.
  4. -t: every <test_project_dir>/<folder>/inputImg is localised into <folder>/loc (center.txt, <test_project_dir>/log.txt)
     and <folder>/loc/<-o> holds every result with t and R in world coordinates (t_relative, R_relative: the map's).

The fit, the transform and the thinning run on the device; the dictionary work is host Python.  Every function takes
`ops`, as sfmlocalization_amd.merge does (default: the C ABI; there is no host fallback in this package).

The PLY files are opt-in (--ply): without the flag nothing is coloured, and PlyUtils.addPointToPly, which appends
the localised centres to colorized_global_structure.ply, runs only where that file already exists.  --beacon is
refused, as elsewhere.
"""
import argparse
import glob
import json
import os
import shutil
import sys

import numpy as np

from . import colorize, hulo, merge

REDUCE_THRES, REDUCE_KNN = 0.01, 1000        # localizeGlobalCoordinateRefPoint.py:221
RANSAC_ROUNDS = 1000                         # :192, localizeGlobalCoordinate.py:210


class DeviceOps(merge.DeviceOps):
    def reduce_points(self, X, A=None, thres=REDUCE_THRES, knn=REDUCE_KNN):
        return self._capi.reduce_points(X, A, thres, knn, self.params)


def _ops(ops, seed=None, device=0):
    return ops if ops is not None else DeviceOps(seed=seed, device=device)


def load_ref_points(path):
    """FileUtils.loadRefPointsJson (FileUtils.py:70-82) -> {landmark key: world X}, in file order"""
    return {p["key"]: p["X"] for p in hulo.load_json(path)["refpoints"]}


def load_image_locations(path, delimit=" "):
    """FileUtils.loadImageLocationListTxt (FileUtils.py:52-66) -> {file name: [x, y, z]}; a line without exactly three
    numbers is reported and skipped"""
    out = {}
    with open(path) as fh:
        for line in fh:
            line = line.strip().split(delimit)
            loc = [float(x) for x in line[1:] if len(x) > 0]
            if len(loc) == 3:
                out[line[0]] = loc
            else:
                print("File " + line[0] + " has invalid location " + str(loc))
    return out


def fit_world_transform(world, loc, thres, rounds=RANSAC_ROUNDS, model="similarity", ops=None, device=0, log=print):
    """localizeGlobalCoordinateRefPoint.py:184-200 / localizeGlobalCoordinate.py:204-218: mergeSfM.ransacTransform(world,
    loc, thres, ransacRound=1000) -> (Amat [3, 4], inlier indices), or (None, inliers) with the reference's message when
    there are fewer than 4 pairs or fewer than 4 inliers.  No ratio test (svdRatio = the largest float, mergeSfM.py:394)."""
    world = np.asarray(world, np.float64).reshape(-1, 3)
    loc = np.asarray(loc, np.float64).reshape(-1, 3)
    if len(world) < 4:
        log("Cannot fix to world coordinate because of less than 4 reference points")
        return None, np.zeros(0, np.uint32)
    res = _ops(ops, device=device).merge_ransac(world, loc, thres, rounds, sys.float_info.max, merge.MODELS[model])
    if res["M"] is None or len(res["inliers"]) < 4:
        log("Cannot estimate transformation matrix to world coordinate")
        log(str(res["M"]))
        return None, res["inliers"]
    log("Transformation matrix has " + str(len(res["inliers"])) + "inliers")
    log(str(res["M"]))
    return res["M"], res["inliers"]


def write_amat(ref_folder, Amat):
    """:202-204: Amat.txt as np.savetxt writes it, then FileUtils.convertNumpyMatTxt2OpenCvMatYml (FileUtils.py:85-114)
    from the text file just written: the YAML holds str() of each value loadtxt returns."""
    txt, yml = os.path.join(ref_folder, "Amat.txt"), os.path.join(ref_folder, "Amat.yml")
    with open(txt, "w") as fh:
        np.savetxt(fh, np.asarray(Amat, np.float64).reshape(3, 4))
    mat = np.loadtxt(txt, dtype="double")
    with open(yml, "w") as fh:
        fh.write("%YAML:1.0\nA: !!opencv-matrix\n   rows: 3\n   cols: 4\n   dt: d\n   data: [ ")
        fh.write(", ".join(str(v) for v in mat.ravel()))
        fh.write(" ]\n")
    return txt, yml


def save_global_sfm(in_sfm, amat_txt, out_sfm, ops=None, device=0):
    """SfmDataUtils.saveGlobalSfM (SfmDataUtils.py:29-44): centres and X become A [.; 1], rotations A[:, :3] R (for a
    similarity s R: the reference's quirk, kept)."""
    doc = hulo.load_json(in_sfm)
    merge.transform_sfm_data(doc, np.loadtxt(amat_txt), ops=_ops(ops, device=device))
    with open(out_sfm, "w") as fh:
        json.dump(doc, fh)


def reduce_close_points(sfm_data, Amat, thres=REDUCE_THRES, knn=REDUCE_KNN, ops=None, device=0):
    """reduceClosePointsKDTree (localizeGlobalCoordinateRefPoint.py:81-118), in place: one device call, then each
    absorbed landmark's observations are appended to its keeper's in the device's order and the absorbed landmarks are
    dropped.  Keys and the order of the keepers stay.  -> the device's result."""
    st = sfm_data["structure"]
    res = _ops(ops, device=device).reduce_points(np.array([s["value"]["X"] for s in st], np.float64).reshape(-1, 3),
                                                 np.asarray(Amat, np.float64), thres, knn)
    for j in res["order"]:
        st[int(res["owner"][j])]["value"]["observations"].extend(st[int(j)]["value"]["observations"])
    sfm_data["structure"] = [s for i, s in enumerate(st) if res["owner"][i] == i]
    return res


def localize_folder(input_dir, sfm_data_dir, matches_dir, out_dir, use_bow):
    """:255-331 (and localizeGlobalCoordinate.py:98-176): a fresh out_dir, the localiser with the reference's arguments
    (-f -r; -k -a -p under --bow; -gm from ReconstructParam.bGuidedMatchingLocalize), center.txt
    -> (result files, image files)"""
    if os.path.isdir(out_dir):
        shutil.rmtree(out_dir)
    os.mkdir(out_dir)
    hulo.localize_images(input_dir, sfm_data_dir, matches_dir, out_dir, param=hulo.LocalizeParam,
                         bow_param=hulo.LocalizeBOWParam if use_bow else None,
                         guided=hulo.ReconstructParam.bGuidedMatchingLocalize)
    n_results, _ = hulo.write_center_txt(out_dir)
    images = []
    for ext in ("*.jpg", "*.JPG", "*.jpeg", "*.JPEG", "*.png", "*.PNG"):
        images.extend(glob.glob(os.path.join(input_dir, ext)))
    return n_results, len(images)


def to_global(result, Amat):
    """:358-362 on one result document, in place: t = A [t; 1], R = R A[:, :3]^T; a failed frame stays as it is"""
    if "t" in result:
        Amat = np.asarray(Amat, np.float64)
        result["t_relative"] = result["t"]
        result["R_relative"] = result["R"]
        result["t"] = np.dot(Amat, np.concatenate([result["t"], [1]])).tolist()
        result["R"] = np.dot(result["R"], Amat[:, 0:3].T).tolist()
    return result


def write_loc_global(loc_folder, Amat, out_name):
    """:349-368 -> the world centres of the localised frames"""
    out, points = {"locGlobal": []}, []
    for name in sorted(os.listdir(loc_folder)):
        if name[-4:] != "json":
            continue
        r = to_global(hulo.load_json(os.path.join(loc_folder, name)), Amat)
        if "t" in r:
            points.append(r["t"])
        out["locGlobal"].append(r)
    with open(os.path.join(loc_folder, out_name), "w") as fh:
        json.dump(out, fh)
    return points


def add_points_to_ply(in_ply, points, out_ply):
    """PlyUtils.addPointToPly (PlyUtils.py:78-110): the structure PLY with the vertex count raised and the localised
    centres appended in red; header lines are copied stripped (empty ones too), body lines stripped and the empty ones
    dropped.  Called only where in_ply exists (see the module text)."""
    header = True
    with open(in_ply) as src, open(out_ply, "w") as fh:
        for line in src:
            line = line.strip()
            tok = line.split()
            if header and len(tok) == 3 and tok[:2] == ["element", "vertex"]:
                line = "element vertex " + str(int(tok[2]) + len(points))
            if header or len(line):
                fh.write(line + "\n")
            if line.lower() == "end_header":
                header = False
        for p in points:
            fh.write("".join(str(v) + " " for v in p) + "255 0 0\n")


def correspondences(ref_folder, sfm_data_dir, matches_dir, ref_points, use_bow, log=print):
    """-> (world [k, 3], map [k, 3], the threshold of the source)"""
    world, loc = [], []
    if ref_points:                                              # localizeGlobalCoordinateRefPoint.py:170-184
        refs = load_ref_points(os.path.join(ref_folder, "refpoints.json"))
        by_key = {}
        for s in hulo.load_json(os.path.join(sfm_data_dir, "sfm_data.json"))["structure"]:
            by_key.setdefault(s["key"], s)                      # ([...][0]: the first landmark with the key)
        for key, X in refs.items():
            log("relative coordinate : " + str(by_key[key]["value"]["X"]))
            log("world coordinate : " + str(X))
            loc.append(by_key[key]["value"]["X"])
            world.append(X)
        log("Number of reference points : " + str(len(world)))
        return world, loc, hulo.ReconstructParam.ransacThresTransformWorldCoordinateRefPoint
    ref_loc = os.path.join(ref_folder, "loc")                   # localizeGlobalCoordinate.py:98-202
    localize_folder(os.path.join(ref_folder, "inputImg"), sfm_data_dir, matches_dir, ref_loc, use_bow)
    names = load_image_locations(os.path.join(ref_folder, "refcoor.txt"))
    world, loc = image_correspondences(ref_loc, names)
    log("From " + str(len(names)) + " reference images, " + str(len(loc)) + " images has been localized.")
    return world, loc, hulo.ReconstructParam.ransacThresTransformWorldCoordinateRefImage


def image_correspondences(ref_loc, names):
    """localizeGlobalCoordinate.py:182-200 -> (world, map) of the localised frames whose image is in `names`; the
    reference walks os.listdir order (unpinned), here the files are sorted"""
    world, loc = [], []
    for entry in sorted(os.listdir(ref_loc)):
        if entry[-4:] != "json":
            continue
        r = hulo.load_json(os.path.join(ref_loc, entry))
        name = os.path.basename(r["filename"])
        if name in names and "t" in r:
            loc.append(r["t"])
            world.append(names[name])
    return world, loc


def run(project_dir, matches_dir, sfm_data_dir, test_project_dir=None, output_json_filename="loc_global.json",
        use_bow=False, reduce_points=False, ref_points=False, model="similarity", seed=None, device=0, ops=None, log=print,
        ply=False):
    """main() of the two scripts -> 0, or 1 when nothing could be fitted (the reference returns silently)"""
    ops = _ops(ops, seed=seed, device=device)
    ref_folder = project_dir + "/Ref"
    sfm_json = os.path.join(sfm_data_dir, "sfm_data.json")
    amat_txt = os.path.join(ref_folder, "Amat.txt")
    if use_bow and not os.path.isfile(os.path.join(matches_dir, "BOWfile.yml")):
        log("Use BOW flag is set, but cannot find BOW model file")
        return 1
    if not os.path.isfile(amat_txt):
        world, loc, thres = correspondences(ref_folder, sfm_data_dir, matches_dir, ref_points, use_bow, log)
        Amat, _ = fit_world_transform(world, loc, thres, model=model, ops=ops, log=log)
        if Amat is None:
            return 1
        write_amat(ref_folder, Amat)
    Amat = np.loadtxt(amat_txt)
    if reduce_points:                                           # localizeGlobalCoordinateRefPoint.py:209-230
        log("start reducing 3D points...")
        doc = hulo.load_json(sfm_json)
        log("point size before reducing : " + str(len(doc["structure"])))
        reduce_close_points(doc, Amat, ops=ops)
        log("point size after reducing : " + str(len(doc["structure"])))
        shutil.copyfile(sfm_json, os.path.join(sfm_data_dir, "sfm_data_b4rp.json"))
        with open(sfm_json, "w") as fh:
            json.dump(doc, fh)
        log("finish reducing 3D points.")
    sfm_global = os.path.join(sfm_data_dir, "sfm_data_global.json")
    save_global_sfm(sfm_json, amat_txt, sfm_global, ops=ops)
    if ply:                                                     # localizeGlobalCoordinate.py:229-231
        if (colorize.run(sfm_global, os.path.join(sfm_data_dir, "colorized_global.ply"), device)
                or colorize.save_camera_ply(sfm_global, os.path.join(sfm_data_dir, "colorized_global_camera.ply"), device)
                or colorize.save_structure_ply(sfm_global, os.path.join(sfm_data_dir, "colorized_global_structure.ply"),
                                               device)):
            return 1
    if not test_project_dir:
        return 0
    total = done = 0                                            # :239-378
    log_txt = os.path.join(test_project_dir, "log.txt")
    if os.path.exists(log_txt):
        os.remove(log_txt)
    for folder in sorted(os.listdir(test_project_dir)):
        test_dir = os.path.join(test_project_dir, folder)
        if not os.path.exists(os.path.join(test_dir, "inputImg")):
            continue
        loc_dir = os.path.join(test_dir, "loc")
        if not os.path.isfile(os.path.join(loc_dir, "center.txt")):
            n_loc, n_img = localize_folder(os.path.join(test_dir, "inputImg"), sfm_data_dir, matches_dir, loc_dir, use_bow)
            with open(log_txt, "a") as fh:
                fh.write("result for : " + test_dir + "\n")
                fh.write("number of localized frame : " + str(n_loc) + "/" + str(n_img) + "\n")
                fh.write("ratio of localized frame : " + str(float(n_loc) / n_img) + "\n")
            total += n_img
            done += n_loc
        points = write_loc_global(loc_dir, Amat, output_json_filename)
        ply = os.path.join(sfm_data_dir, "colorized_global_structure.ply")
        if os.path.isfile(ply):
            add_points_to_ply(ply, points, os.path.join(loc_dir, "colorized_global_localize.ply"))
    with open(log_txt, "a") as fh:
        fh.write("total result" + "\n")
        fh.write("number of localized frame : " + str(done) + "/" + str(total) + "\n")
        if total:                                               # (the reference divides by zero when every folder was done)
            fh.write("ratio of localized frame : " + str(float(done) / total) + "\n")
    return 0


def parse_args(argv):
    ap = argparse.ArgumentParser(prog="python -m sfmlocalization_amd.globalcoord", description=__doc__.split("\n\n")[0])
    ap.add_argument("project_dir")
    ap.add_argument("matches_dir")
    ap.add_argument("sfm_data_dir")
    ap.add_argument("-t", "--test-project-dir", nargs="?", default=None)
    ap.add_argument("-o", "--output-json-filename", nargs="?", default="loc_global.json")
    ap.add_argument("--bow", action="store_true")
    ap.add_argument("--beacon", action="store_true")
    ap.add_argument("--reduce-points", action="store_true")
    ap.add_argument("--ref-points", action="store_true")
    ap.add_argument("--model", choices=sorted(merge.MODELS), default="similarity")
    ap.add_argument("--seed", type=lambda s: int(s, 0), default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--ply", action="store_true")
    return ap.parse_args(argv)


def main(argv=None, ops=None):
    a = parse_args(sys.argv[1:] if argv is None else list(argv))
    if a.beacon:
        print("globalcoord: iBeacon view pre-selection is out of scope (--beacon)", file=sys.stderr)
        return 1
    from . import capi
    try:
        return run(a.project_dir, a.matches_dir, a.sfm_data_dir, a.test_project_dir, a.output_json_filename, a.bow,
                   a.reduce_points, a.ref_points, a.model, a.seed, a.device, ops=ops, log=lambda s: print(s, flush=True),
                   ply=a.ply)
    except capi.SfmlocError as e:
        print(f"globalcoord: {e.message}", file=sys.stderr)
        return 1


if __name__ == "__main__":
    sys.exit(main())
