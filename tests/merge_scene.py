"""Scenes of the map-merge tests: planted 3D-3D match sets (a similarity or an anisotropic affine map, inliers with
noise far below the threshold, outliers far above it) and a pair of small sfm_data documents with localisation results
whose consistent matches are such a set, plus the cases of the consistency filter."""
import json
import os

import numpy as np

THRES = 0.5


def rotation(rng):
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def planted(seed=7, n=48, n_in=30, scale=1.3, stretch=None, thres=THRES, spread=20.0):
    """-> (A [n, 3], B [n, 3], M [3, 4], inlier indices): A = M [B; 1] + noise uniform within thres / 100 per axis on
    the inliers; the outliers are displaced by 5..20 per axis.  stretch: per-axis factors applied before the rotation
    (an anisotropic affine map, singular values scale * stretch)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = scale * rotation(rng)
    if stretch is not None:
        L = L @ np.diag(stretch)
    t = rng.uniform(-30, 30, 3)
    M = np.hstack([L, t[:, None]])
    B = rng.uniform(-spread, spread, (n, 3))
    A = B @ L.T + t
    inl = np.sort(rng.permutation(n)[:n_in])
    out = np.setdiff1d(np.arange(n), inl)
    A[inl] += rng.uniform(-thres / 100, thres / 100, (len(inl), 3))
    A[out] += rng.uniform(5, 20, (len(out), 3)) * rng.choice([-1.0, 1.0], (len(out), 3))
    return A, B, M, inl


# ---- documents ---------------------------------------------------------------------------------------------------------
F, PP, W, H = 600.0, (320.0, 240.0), 640, 480


def _views(names, first_ptr):
    out = []
    for k, name in enumerate(names):
        v = {"key": k, "value": {"polymorphic_id": 1073741824 if k else 2147483649, "ptr_wrapper": {
            "id": first_ptr + k, "data": {"local_path": "/", "filename": name, "width": W, "height": H, "id_view": k,
                                          "id_intrinsic": 0, "id_pose": k}}}}
        if k == 0:
            v["value"]["polymorphic_name"] = "view"
        out.append(v)
    return out


def _intrinsics(ptr):
    return [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole", "ptr_wrapper": {
        "id": ptr, "data": {"width": W, "height": H, "focal_length": F, "principal_point": list(PP)}}}}]


def _doc(names, centres, points, keys, rng, obs_per_point=3, feat0=0):
    """cameras look down +z from `centres` (identity rotation); every point is seen by obs_per_point views"""
    ext = [{"key": k, "value": {"rotation": np.eye(3).tolist(), "center": [float(x) for x in c]}}
           for k, c in enumerate(centres)]
    st, feat = [], [feat0] * len(names)
    for key, X in zip(keys, points):
        obs = []
        for v in sorted(rng.permutation(len(names))[:obs_per_point].tolist()):
            Xc = X - centres[v]
            x = F * Xc[:2] / Xc[2] + np.array(PP)
            obs.append({"key": v, "value": {"id_feat": feat[v], "x": [float(x[0]), float(x[1])]}})
            feat[v] += 1
        st.append({"key": int(key), "value": {"X": [float(x) for x in X], "observations": obs}})
    return {"sfm_data_version": "0.3", "root_path": "/data/images", "views": _views(names, 2147483649),
            "intrinsics": _intrinsics(2147483700), "extrinsics": ext, "structure": st, "control_points": []}


def make_docs(seed=11, n=48, n_in=30, stretch=None, extra_a=25, extra_b=20):
    """-> dict(docA, docB, loc: [(file name, result document)], match: the consistent matches [k, 2] (B id, A id) in
    ascending B id, A, B: their points, M, inl).  Model B's landmarks 100 + 2 i (i < n) are the planted matches of A's
    landmarks 3 i; each is localised once, through its first observation.  The consistency cases ride on top:
      B 300 seen from two views with the same A 200 (kept: one more match, an inlier of the planted map)
      B 302 with A 201 and A 202 (dropped)
      B 304 and B 306 both on A 203 (both dropped)
      a pair whose feature 9999 has no landmark, a result for zz.jpg that model B does not have, a result without "t",
      B 308 and B 310 sharing (view 0, feature 7777): the later entry, 310, owns it -> (310, 204)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    A, B, M, inl = planted(seed, n, n_in, stretch=stretch)
    L, t = M[:, :3], M[:, 3]
    Linv = np.linalg.inv(L)
    names_a = [f"a{k}.jpg" for k in range(4)]
    names_b = [f"b{k}.jpg" for k in range(5)]
    keys_a = [3 * i for i in range(n)] + [200 + i for i in range(5)] + [1000 + i for i in range(extra_a)]
    special_a = rng.uniform(-20, 20, (5, 3)) @ L.T + t
    pts_a = np.vstack([A, special_a, rng.uniform(-20, 20, (extra_a, 3)) @ L.T + t])
    keys_b = [100 + 2 * i for i in range(n)] + [300, 302, 304, 306, 308, 310] + [2000 + i for i in range(extra_b)]
    special_b = np.vstack([(special_a[0] - t) @ Linv.T, rng.uniform(-20, 20, (5, 3))])
    pts_b = np.vstack([B, special_b, rng.uniform(-20, 20, (extra_b, 3))])
    cam_b = np.array([[-6.0 + 3 * k, 0.5 * k, -80.0] for k in range(5)])
    cam_a = cam_b[:4] @ L.T + t + np.array([0, 0, -150.0])
    docA = _doc(names_a, cam_a, pts_a, keys_a, rng)
    docB = _doc(names_b, cam_b, pts_b, keys_b, rng)
    by_key = {s["key"]: s for s in docB["structure"]}
    pairs = {k: [] for k in range(5)}
    for i in range(n):
        ob = by_key[100 + 2 * i]["value"]["observations"][0]
        pairs[ob["key"]].append([ob["value"]["id_feat"], 3 * i])
    for ob in by_key[300]["value"]["observations"][:2]:
        pairs[ob["key"]].append([ob["value"]["id_feat"], 200])
    o = by_key[302]["value"]["observations"]
    pairs[o[0]["key"]].append([o[0]["value"]["id_feat"], 201])
    pairs[o[1]["key"]].append([o[1]["value"]["id_feat"], 202])
    for key in (304, 306):
        ob = by_key[key]["value"]["observations"][0]
        pairs[ob["key"]].append([ob["value"]["id_feat"], 203])
    pairs[1].append([9999, 3])
    for key in (308, 310):
        by_key[key]["value"]["observations"].append({"key": 0, "value": {"id_feat": 7777, "x": [1.0, 2.0]}})
    pairs[0].append([7777, 204])
    loc = []
    for k in range(5):
        c = (cam_b[k] @ L.T + t).tolist()
        loc.append((f"b{k}.json", {"filename": f"/some/where/b{k}.jpg", "t": c, "R": np.eye(3).tolist(), "pair": pairs[k]}))
    loc.append(("zz.json", {"filename": "/some/where/zz.jpg", "t": [0.0, 0.0, 0.0], "R": np.eye(3).tolist(),
                            "pair": [[0, 6], [1, 9]]}))
    loc.append(("lost.json", {"filename": "/some/where/b1.jpg", "pair": [[0, 12]]}))
    match = [[100 + 2 * i, 3 * i] for i in range(n)] + [[300, 200], [310, 204]]
    match = np.array(sorted(match), np.int64)
    pa = dict(zip(keys_a, pts_a))
    pb = dict(zip(keys_b, pts_b))
    return {"docA": docA, "docB": docB, "loc": loc, "match": match, "M": M,
            "A": np.array([pa[a] for _, a in match]), "B": np.array([pb[b] for b, _ in match])}


def write_docs(scene, folder):
    """-> (sfmA path, sfmB path, loc folder) under `folder`"""
    os.makedirs(os.path.join(folder, "loc"), exist_ok=True)
    pa, pb = os.path.join(folder, "sfm_data_A.json"), os.path.join(folder, "sfm_data_B.json")
    for p, d in ((pa, scene["docA"]), (pb, scene["docB"])):
        with open(p, "w") as fh:
            json.dump(d, fh)
    for name, d in scene["loc"]:
        with open(os.path.join(folder, "loc", name), "w") as fh:
            json.dump(d, fh)
    return pa, pb, os.path.join(folder, "loc")
