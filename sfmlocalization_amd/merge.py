"""mergeSfM.mergeModel (hulo_sfm/mergeSfM.py) over the C ABI: the step of the reference's mergeOneModel
(hulo_sfm/sfmMergeGraph.py:213-422) between the localiser (:243-252, hulo.localize_images) and OpenMVG_BA (:297,
adjust.run) -- model B's landmarks matched to model A's through the localisation results, a RANSAC over the 3D-3D
matches for the map B -> A, and the merged sfm_data.

    python -m sfmlocalization_amd.merge <sfmA> <sfmB> <locFolderB> <out> --ransac-thres=T --merge-thres=T
                                        [--model=similarity|affine] [--round-mul=100] [--min-limit=4] [--svd-ratio=1.75]
                                        [--img-dir=DIR] [--seed=N] [--device=0]

The RANSAC, the inlier lists, the nearest-neighbour medians of the threshold functions and the transforms run on the
device (sfmloc_merge_*, csrc/merge.hip; include/sfmloc.h states the arithmetic); the dictionary work and the document
merge are host NumPy.  Every function takes `ops`: the object whose merge_ransac / merge_inliers / merge_median_nn /
merge_transform do the device's part (default: the C ABI on `device`; there is no host fallback in this package).
"""
import json
import os
import sys

import numpy as np

from . import hulo

MODELS = {"similarity": 0, "affine": 1}
RANSAC_ROUND_MUL = 100                       # ReconstructParam.ransacRoundMul (ReconstructParam.py:148)


class DeviceOps:
    """The device entry points over the C ABI (capi.merge_*) with one seed and device."""

    def __init__(self, seed=None, device=0, rounds_per_launch=0):
        from . import capi
        self._capi = capi
        over = {"device": int(device), "rounds_per_launch": int(rounds_per_launch)}
        if seed is not None:
            over["seed"] = int(seed)
        self.params = capi.merge_default_params(**over)
        self.seed = int(self.params.seed)

    def merge_ransac(self, A, B, thres, rounds, svd_ratio, model, stream=0):
        return self._capi.merge_ransac(A, B, thres, rounds, svd_ratio, model, stream, self.params)

    def merge_inliers(self, A, B, M, thres):
        return self._capi.merge_inliers(A, B, M, thres, self.params)

    def merge_median_nn(self, X):
        return self._capi.merge_median_nn(X, self.params)

    def merge_transform(self, M, R=None, X=None):
        return self._capi.merge_transform(M, R, X, self.params)


def _ops(ops, seed=None, device=0):
    return ops if ops is not None else DeviceOps(seed=seed, device=device)


def _view_data(view):
    return view["value"]["ptr_wrapper"]["data"]


def imgname_to_view_id(imgname, sfm_data):
    """mergeSfM.imgnameToViewID (:69-85): the id_view of each image name, -1 for a name no view carries.  Two views with
    one file name: the last wins; a name listed twice: only its first entry gets the id (list.index)."""
    by_name = {}
    for view in sfm_data["views"]:
        by_name[_view_data(view)["filename"]] = _view_data(view)["id_view"]
    out, seen = [], set()
    for name in imgname:
        out.append(by_name.get(name, -1) if name not in seen else -1)
        seen.add(name)
    return out


def consistent_3d_match(view_id, match_list, sfm_data_b):
    """mergeSfM.getViewFeatTo3DMap + getConsistent3DMatch (:89-166) -> int64 [k, 2] of (landmark B, landmark A).
    Each pair (feature of a B view, landmark of A) goes through B's (view, feature) -> landmark table (a later structure
    entry overwrites an earlier one, as the dict does; pairs of view -1 or of a feature without a landmark are skipped);
    a B landmark that meets two different A landmarks is dropped, then every A landmark claimed by more than one
    surviving B landmark is dropped with all its claimants.  The reference returns a list in dict order (unpinned in
    Python 2): here the rows are in ascending B landmark id."""
    if len(view_id) != len(match_list):
        raise ValueError("lengths of viewID and matchList are not the same")
    keys, lms = [], []
    for lm in sfm_data_b["structure"]:
        for ob in lm["value"]["observations"]:
            keys.append((int(ob["key"]) << 32) | int(ob["value"]["id_feat"]))
            lms.append(int(lm["key"]))
    keys, lms = np.array(keys, np.int64), np.array(lms, np.int64)
    order = np.argsort(keys, kind="stable")
    keys, lms = keys[order], lms[order]
    last = np.ones(len(keys), bool)
    last[:-1] = keys[1:] != keys[:-1]          # of equal keys the last in structure order stays
    keys, lms = keys[last], lms[last]
    q, a = [], []
    for v, pairs in zip(view_id, match_list):
        if v < 0 or len(pairs) == 0:
            continue
        p = np.array(pairs, np.int64).reshape(-1, 2)
        q.append((np.int64(v) << 32) | p[:, 0])
        a.append(p[:, 1])
    if not q or len(keys) == 0:
        return np.zeros((0, 2), np.int64)
    q, a = np.concatenate(q), np.concatenate(a)
    pos = np.minimum(np.searchsorted(keys, q), len(keys) - 1)
    hit = keys[pos] == q
    ba = np.unique(np.stack([lms[pos[hit]], a[hit]], 1), axis=0)     # distinct (B, A), ascending B then A
    if len(ba) == 0:
        return np.zeros((0, 2), np.int64)
    _, inv, cnt = np.unique(ba[:, 0], return_inverse=True, return_counts=True)
    ba = ba[cnt[inv.ravel()] == 1]                                      # one A per B
    _, inv, cnt = np.unique(ba[:, 1], return_inverse=True, return_counts=True)
    return ba[cnt[inv.ravel()] == 1]                                    # one B per A


def point_locations(sfm_data, ids):
    """mergeSfM.get3DPointloc (:169-183): X of each landmark id, inf for an id the structure does not have"""
    index = {lm["key"]: j for j, lm in enumerate(sfm_data["structure"])}
    out = np.full((len(ids), 3), np.inf)
    for k, i in enumerate(ids):
        j = index.get(int(i))
        if j is not None:
            out[k] = sfm_data["structure"][j]["value"]["X"]
    return out


def _median_thres(points, k, ops):
    X = np.asarray(points, np.float64).reshape(-1, 3)
    if X.shape[0] < 2:
        return 0
    return k * ops.merge_median_nn(X)


def findMedianThres(sfm_data, k, ops=None, device=0):
    """mergeSfM.findMedianThres (:262-279): k x the median over the camera centres of the distance to the nearest other
    centre; 0 for fewer than 2."""
    return _median_thres([e["value"]["center"] for e in sfm_data["extrinsics"]], k, _ops(ops, device=device))


def findMedianStructurePointsThres(sfm_data, k, ops=None, device=0):
    """mergeSfM.findMedianStructurePointsThres (:284-301): the same over the structure points"""
    return _median_thres([s["value"]["X"] for s in sfm_data["structure"]], k, _ops(ops, device=device))


def transform_sfm_data(sfm_data, M, ops=None, device=0):
    """mergeSfM.transform_sfm_data (:419-442), in place: rotations become M[:, :3] R (for a similarity s R: the
    reference's quirk), centres and points M [X; 1]."""
    ops = _ops(ops, device=device)
    ext, st = sfm_data["extrinsics"], sfm_data["structure"]
    R = [e["value"]["rotation"] for e in ext]
    X = [e["value"]["center"] for e in ext] + [s["value"]["X"] for s in st]
    Rn, Xn = ops.merge_transform(np.asarray(M, np.float64), R if R else None, X if X else None)
    for j, e in enumerate(ext):
        e["value"]["rotation"] = Rn[j].tolist()
        e["value"]["center"] = Xn[j].tolist()
    for j, s in enumerate(st):
        s["value"]["X"] = Xn[len(ext) + j].tolist()


def merge_sfm_data(sfm_dataA, sfm_dataB, M, inlierMapBA, ops=None, device=0):
    """mergeSfM.merge_sfm_data (:446-534): B into A, in place.  B's views, poses and observations are renumbered from
    firstViewB = A's last id_view + 1 and its views take intrinsic 0; B's poses and unmatched points are transformed by M;
    a B landmark in inlierMapBA only appends its observations to A's landmark; the others get new keys from A's largest
    key + 1, in B's structure order."""
    ops = _ops(ops, device=device)
    first = _view_data(sfm_dataA["views"][-1])["id_view"] + 1
    for view in sfm_dataB["views"]:
        d = _view_data(view)
        view["key"] = first + d["id_view"]
        d["id_intrinsic"] = 0
        d["id_view"] = first + d["id_view"]
        d["id_pose"] = first + d["id_pose"]
        sfm_dataA["views"].append(view)
    extB = sfm_dataB["extrinsics"]
    fresh = [s for s in sfm_dataB["structure"] if s["key"] not in inlierMapBA]
    R = [e["value"]["rotation"] for e in extB]
    X = [e["value"]["center"] for e in extB] + [s["value"]["X"] for s in fresh]
    Rn, Xn = ops.merge_transform(np.asarray(M, np.float64), R if R else None, X if X else None)
    for j, e in enumerate(extB):
        e["key"] = first + e["key"]
        e["value"]["rotation"] = Rn[j].tolist()
        e["value"]["center"] = Xn[j].tolist()
        sfm_dataA["extrinsics"].append(e)
    index, next_key = {}, 0
    for i, s in enumerate(sfm_dataA["structure"]):
        index[s["key"]] = i
        next_key = max(next_key, s["key"])
    next_key += 1
    j = len(extB)
    for s in sfm_dataB["structure"]:
        for ob in s["value"]["observations"]:
            ob["key"] = first + ob["key"]
        if s["key"] in inlierMapBA:
            sfm_dataA["structure"][index[inlierMapBA[s["key"]]]]["value"]["observations"].extend(s["value"]["observations"])
        else:
            s["key"] = next_key
            next_key += 1
            s["value"]["X"] = Xn[j].tolist()
            j += 1
            sfm_dataA["structure"].append(s)


def mergeModel(sfm_data_dirA, sfm_data_dirB, locFolderB, outfile, ransacThres, mergePointThres,
               ransacRoundMul=RANSAC_ROUND_MUL, inputImgDir="", minLimit=4, svdRatio=1.75, model="similarity", seed=None,
               device=0, ops=None, log=None):
    """mergeSfM.mergeModel (:540-612) -> (number of consistent matches, number of RANSAC inliers, M): M a 3 x 4 array,
    or empty when there are too few matches or no model (the second count is then the first, as there).  `outfile` is
    written (json.dump of the merged document) only when the merge goes through.  model: "similarity" (what the
    reference runs with transformations.py installed) or "affine" (its in-tree fallback); seed: the sampling key
    (default: the library's).  The RANSAC runs len(matches) x ransacRoundMul rounds on sampling stream 0."""
    log = log if log is not None else (lambda s: None)
    ops = _ops(ops, seed=seed, device=device)
    log("Loading sfm_data")
    docB = hulo.load_json(sfm_data_dirB)
    names, pairs = hulo.read_match(locFolderB)
    match = consistent_3d_match(imgname_to_view_id(names, docB), pairs, docB)
    n = len(match)
    log("Found " + str(n) + " consistent matches")
    if n <= 4 or n <= minLimit:
        return n, n, np.asarray([])
    docA = hulo.load_json(sfm_data_dirA)
    A = point_locations(docA, match[:, 1])
    B = point_locations(docB, match[:, 0])
    rounds = n * ransacRoundMul
    log("Number of RANSAC round : " + str(rounds))
    res = ops.merge_ransac(A, B, ransacThres, rounds, svdRatio, MODELS[model])
    if res["M"] is None:
        return n, n, np.asarray([])
    M, n_inl = res["M"], len(res["inliers"])
    log("Number of ransac inliers: " + str(res["count"]))
    s = np.linalg.svd(M[:, :3], compute_uv=False)
    if n_inl <= minLimit or s[0] / s[-1] > svdRatio:
        return n, n_inl, M
    keep = ops.merge_inliers(A, B, M, mergePointThres)
    log("Number of inliers for given transform : " + str(len(keep)))
    merge_sfm_data(docA, docB, M, {int(match[x, 0]): int(match[x, 1]) for x in keep}, ops=ops)
    if inputImgDir != "":
        docA["root_path"] = inputImgDir
    with open(outfile, "w") as fh:
        json.dump(docA, fh)
    return n, n_inl, M


def modelMergeCheckLocal(sfm_data_path, sfm_locOut, medThres):
    """mergeSfM.modelMergeCheckLocal (:626-659) -> (frames localised whose view has a pose in the model, those within
    medThres of it).  Host only."""
    doc = hulo.load_json(sfm_data_path)
    names, locs = [], []
    for entry in os.listdir(sfm_locOut):
        if entry[-4:] != "json":
            continue
        r = hulo.load_json(os.path.join(sfm_locOut, entry))
        if "t" in r:
            names.append(os.path.basename(r["filename"]))
            locs.append(r["t"])
    pose_of = {_view_data(v)["id_view"]: _view_data(v)["id_pose"] for v in doc["views"]}
    centre_of = {e["key"]: e["value"]["center"] for e in doc["extrinsics"]}
    n_file = n_agree = 0
    for vid, t in zip(imgname_to_view_id(names, doc), locs):
        c = centre_of.get(pose_of.get(vid))
        if c is None:
            continue
        d = np.linalg.norm(np.array(t, np.float64) - np.array(c, np.float64))
        if d < float("inf"):
            n_file += 1
            n_agree += bool(d < medThres)
    return n_file, n_agree


USAGE = ("Usage: python -m sfmlocalization_amd.merge <sfmA> <sfmB> <locFolderB> <out> --ransac-thres=T --merge-thres=T\n"
         "       [--model=similarity|affine] [--round-mul=100] [--min-limit=4] [--svd-ratio=1.75] [--img-dir=DIR]\n"
         "       [--seed=N] [--device=0]\n")


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    pos, opt = [], {}
    for a in argv:
        if a.startswith("--") and "=" in a:
            k, v = a[2:].split("=", 1)
            opt[k] = v
        elif a.startswith("-"):
            sys.stderr.write(USAGE)
            return 1
        else:
            pos.append(a)
    known = {"ransac-thres", "merge-thres", "model", "round-mul", "min-limit", "svd-ratio", "img-dir", "seed", "device"}
    if len(pos) != 4 or "ransac-thres" not in opt or "merge-thres" not in opt or set(opt) - known or \
            opt.get("model", "similarity") not in MODELS:
        sys.stderr.write(USAGE)
        return 1
    from . import capi
    try:
        out = mergeModel(pos[0], pos[1], pos[2], pos[3], float(opt["ransac-thres"]), float(opt["merge-thres"]),
                         ransacRoundMul=int(opt.get("round-mul", RANSAC_ROUND_MUL)), inputImgDir=opt.get("img-dir", ""),
                         minLimit=int(opt.get("min-limit", 4)), svdRatio=float(opt.get("svd-ratio", 1.75)),
                         model=opt.get("model", "similarity"), seed=int(opt["seed"], 0) if "seed" in opt else None,
                         device=int(opt.get("device", 0)), log=lambda s: print(s, flush=True))
    except capi.SfmlocError as e:
        print(f"merge: {e.message}", file=sys.stderr)
        return 1
    print((out[0], out[1], out[2].tolist()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
