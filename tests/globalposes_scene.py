"""Planted scenes for sfmloc_global_poses: cameras with known rotations and centres, their relative poses with noise, and
the planted faults the stage must deal with.  A scene is a dict: n_views, pairs [P, 2], rel_R [P, 3, 3], rel_t [P, 3],
use_t [P], R_true [n, 3, 3] (world to camera), C_true [n, 3], and the indices of what was planted."""
import numpy as np


def rodrigues(w):
    th = float(np.linalg.norm(w))
    if th == 0.0:
        return np.eye(3)
    k = w / th
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def random_rotation(rng, max_angle):
    w = rng.normal(size=3)
    return rodrigues(w / np.linalg.norm(w) * rng.uniform(0.0, max_angle))


def relative(R, C, i, j, rng, rot_noise, dir_noise):
    """X_J = R_ij X_I + t_ij from the planted poses, the rotation off by up to rot_noise and the direction by dir_noise
    (radians), |t| = 1 exactly to rounding"""
    Rij = rodrigues(rng.normal(size=3) * rot_noise / np.sqrt(3.0)) @ R[j] @ R[i].T
    t = R[j] @ (C[i] - C[j])
    t = t / np.linalg.norm(t) + rng.normal(size=3) * dir_noise / np.sqrt(3.0)
    return Rij, t / np.linalg.norm(t)


def ring_cameras(rng, n, radius, jitter):
    """n cameras around a circle, each off it by up to `jitter` in every axis (so that no stretch is collinear), looking
    roughly inwards"""
    th = 2.0 * np.pi * np.arange(n) / n
    C = np.stack([radius * np.cos(th), radius * np.sin(th), np.zeros(n)], 1) + rng.uniform(-jitter, jitter, (n, 3))
    R = np.stack([rodrigues(np.array([0.0, 0.0, t])) @ random_rotation(rng, 0.5) for t in th])
    return R, C


def ring_pairs(n, reach):
    return [(i, (i + k) % n) for i in range(n) for k in range(1, reach + 1)]


def build(R, C, pair_list, rng, rot_noise, dir_noise):
    rel = [relative(R, C, i, j, rng, rot_noise, dir_noise) for i, j in pair_list]
    return dict(n_views=len(R), pairs=np.array(pair_list, np.uint32), rel_R=np.stack([r for r, _ in rel]),
                rel_t=np.stack([t for _, t in rel]), use_t=np.ones(len(pair_list), np.uint8), R_true=R, C_true=C)


def scene_triplet(seed=1):
    """(a) three views, one triplet"""
    rng = np.random.default_rng(seed)
    R = np.stack([random_rotation(rng, 1.0) for _ in range(3)])
    C = np.array([[0.0, 0.0, 0.0], [2.0, 0.3, 0.1], [0.7, 1.9, -0.4]])
    return build(R, C, [(0, 1), (1, 2), (2, 0)], rng, np.radians(0.2), 0.005)


def scene_ring(seed=2):
    """(b) a 12-view ring, each view paired with its 3 nearest neighbours on either side (36 pairs), with three planted
    wrong pairs, one pure-rotation pair with use_t = 0, a pendant view 12 on a single pair and a separate component of
    the views 13, 14, 15"""
    rng = np.random.default_rng(seed)
    R, C = ring_cameras(rng, 12, 3.0, 0.6)
    R = np.concatenate([R, np.stack([random_rotation(rng, 1.0) for _ in range(4)])])
    C = np.concatenate([C, np.array([[5.0, 0.5, 0.2], [9.0, 0.0, 0.0], [10.0, 1.0, 0.3], [9.5, -1.0, 1.0]])])
    plist = ring_pairs(12, 3) + [(12, 0), (13, 14), (14, 15), (15, 13)]
    s = build(R, C, plist, rng, np.radians(0.4), 0.01)
    s["wrong"] = [4, 17, 29]
    for k in s["wrong"]:
        s["rel_R"][k] = rodrigues(np.array([0.3, -0.4, 0.35])) @ s["rel_R"][k]
        t = rng.normal(size=3)
        s["rel_t"][k] = t / np.linalg.norm(t)
    s["rotation_only"] = 10
    s["use_t"][s["rotation_only"]] = 0
    t = rng.normal(size=3)
    s["rel_t"][s["rotation_only"]] = t / np.linalg.norm(t)    # (what a pair without a baseline reports: noise)
    s["pendant"], s["other_component"] = 12, [13, 14, 15]
    return s


def scene_large(seed=3, n=1100, hub_pairs=300):
    """(c) n views, each paired with its 3 nearest ring neighbours on either side, plus one hub view paired with
    hub_pairs others: more than one workgroup of views, and one view above the wave-per-view threshold"""
    rng = np.random.default_rng(seed)
    R, C = ring_cameras(rng, n, 10.0, 0.15)
    R = np.concatenate([R, random_rotation(rng, 1.0)[None]])
    C = np.concatenate([C, np.array([[0.5, -0.3, 4.0]])])
    others = np.sort(rng.choice(n, hub_pairs, replace=False))
    plist = ring_pairs(n, 3) + [(n, int(v)) if q % 2 else (int(v), n) for q, v in enumerate(others)]
    s = build(R, C, plist, rng, np.radians(0.2), 0.005)
    s["hub"] = n
    return s


def errors(s, in_component, root, R, C):
    """-> (largest rotation error in degrees against the planted rotations in the root's gauge, largest centre error
    after the one similarity the gauge allows, as a fraction of the planted component's extent)"""
    import globalposes_np as tw
    v = np.nonzero(in_component)[0]
    Rt = s["R_true"][v] @ s["R_true"][root].T
    rot = float(np.max(tw.rotation_error_deg(R[v], Rt)))
    Ct = s["C_true"][v]
    extent = float(np.max(np.linalg.norm(Ct - Ct.mean(0), axis=1)))
    cen = float(np.max(np.linalg.norm(tw.align_similarity(C[v], Ct) - Ct, axis=1))) / extent
    return rot, cen


# ---- the end-to-end scene: files for the chain relpose -> globalposes -> structure ---------------------------------------

E2E_VIEW_ID = [3, 4, 7, 9, 12, 13]
E2E_W, E2E_H, E2E_K = 640, 480, (700.0, 320.0, 240.0)


def _look_at(C, target):
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def scene_files(folder=None, seed=4, n_points=300, seen=0.7, noise=0.1):
    """six views around a point cloud, every view seeing a random 70 % of its 300 points (about 150 matches per pair)
    with +-0.1 px of noise; with `folder`, written there as sfm_data.json, <stem>.feat and matches.f.txt -> dict(doc,
    feats, matches, R_true, C_true, path)"""
    import json
    import os
    from sfmlocalization_amd import fileio
    rng = np.random.default_rng(seed)
    n = len(E2E_VIEW_ID)
    X = rng.uniform(-1.0, 1.0, (n_points, 3))
    th = 2.0 * np.pi * np.arange(n) / n + rng.uniform(-0.2, 0.2, n)
    C = np.stack([6.0 * np.cos(th), 6.0 * np.sin(th), rng.uniform(-1.5, 1.5, n)], 1)
    R = np.stack([_look_at(c, rng.uniform(-0.2, 0.2, 3)) for c in C])
    feats, which = [], []
    for v in range(n):
        ids = np.nonzero(rng.uniform(size=n_points) < seen)[0]
        Xc = (X[ids] - C[v]) @ R[v].T
        px = E2E_K[0] * Xc[:, :2] / Xc[:, 2:] + np.array(E2E_K[1:]) + rng.uniform(-noise, noise, (len(ids), 2))
        assert (Xc[:, 2] > 1.0).all() and (px > 0).all() and (px[:, 0] < E2E_W).all() and (px[:, 1] < E2E_H).all()
        feats.append(np.array([[np.float32("%.6g" % x), np.float32("%.6g" % y), 0, 0] for x, y in px], np.float32))
        which.append({int(p): f for f, p in enumerate(ids)})
    matches = {}
    for a in range(n):
        for b in range(a + 1, n):
            both = sorted(set(which[a]) & set(which[b]))
            matches[(E2E_VIEW_ID[a], E2E_VIEW_ID[b])] = (np.array([which[a][p] for p in both], np.uint32),
                                                         np.array([which[b][p] for p in both], np.uint32))
    views = []
    for k in range(n):
        v = {"key": E2E_VIEW_ID[k], "value": {"polymorphic_id": 1073741824 if k else 2147483649, "ptr_wrapper": {
            "id": 2147483649 + k, "data": {"local_path": "/", "filename": f"frame{k:04d}.jpg", "width": E2E_W,
                                           "height": E2E_H, "id_view": E2E_VIEW_ID[k], "id_intrinsic": 0,
                                           "id_pose": E2E_VIEW_ID[k]}}}}
        if k == 0:
            v["value"]["polymorphic_name"] = "view"
        views.append(v)
    intr = [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole", "ptr_wrapper": {
        "id": 2147483709, "data": {"width": E2E_W, "height": E2E_H, "focal_length": E2E_K[0],
                                   "principal_point": list(E2E_K[1:])}}}}]
    doc = {"sfm_data_version": "0.3", "root_path": "/data/images", "views": views, "intrinsics": intr, "extrinsics": [],
           "structure": [], "control_points": []}
    out = dict(doc=doc, feats=feats, matches=matches, R_true=R, C_true=C, path=None)
    if folder is not None:
        for k, f in enumerate(feats):
            fileio.write_feat(os.path.join(folder, f"frame{k:04d}.feat"), f)
        fileio.write_matches_txt(os.path.join(folder, "matches.f.txt"), matches)
        out["path"] = os.path.join(folder, "sfm_data.json")
        with open(out["path"], "w") as fh:
            json.dump(doc, fh)
    return out


def relpose_call(s):
    """the arguments of capi.RelPoses / relpose_np.relative_poses for scene_files' scene"""
    from sfmlocalization_amd import capi
    index = {v: k for k, v in enumerate(E2E_VIEW_ID)}
    pairs, offsets, mi, mj = capi.pair_arrays(s["matches"], index)
    n = len(E2E_VIEW_ID)
    return dict(view_off=np.concatenate([[0], np.cumsum([len(f) for f in s["feats"]])]).astype(np.uint64),
                kpt_xy=np.concatenate([f[:, :2] for f in s["feats"]]).astype(np.float32),
                view_wh=np.tile(np.array([E2E_W, E2E_H], np.uint32), (n, 1)), view_intrinsic=np.zeros(n, np.uint32),
                intrinsics=np.array([list(E2E_K) + [0.0, 0.0, 0.0]]), intrinsic_type=np.zeros(1, np.uint32), pairs=pairs,
                offsets=offsets, match_i=mi, match_j=mj)
