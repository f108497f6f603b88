"""Scenes of the world-coordinate tests: small sfm_data documents whose landmarks form planted clusters in world
coordinates, built so that the reference's reduceClosePointsKDTree has one answer whatever cKDTree's rounding and tie
order: every pair of landmarks is at most 0.9 thres or at least 1.1 thres apart and no two distances from one landmark
are closer than thres / 1000 to each other.  Also the reference-point and reference-image inputs of the fit."""
import json
import os

import numpy as np

import merge_scene as MS

THRES = 0.01


def world(X, A):
    X = np.asarray(X, np.float64)
    return X @ A[:, :3].T + A[:, 3]


def well_separated(G, thres):
    d = np.sqrt(((G[:, None, :] - G[None, :, :]) ** 2).sum(2))
    if ((d > 0.9 * thres) & (d < 1.1 * thres)).any():
        return False
    for i in range(len(G)):
        row = np.sort(d[i][d[i] < 2 * thres])
        if (np.diff(row) < thres / 1000).any():
            return False
    return True


def clustered(seed, A, n_bg, sizes, thres=THRES, reach=0.8):
    """points in map coordinates whose images under A are n_bg scattered points and clusters of the given sizes around
    some of them (members within reach x thres of the centre, so not all within thres of one another), shuffled;
    seeds are tried in turn until the scene is well separated"""
    Ainv = np.linalg.inv(A[:, :3])
    while True:
        rng = np.random.Generator(np.random.PCG64(seed))
        G = [rng.uniform(-2.0, 2.0, (n_bg, 3))]
        for k, m in enumerate(sizes):
            v = rng.normal(size=(m, 3))
            v *= (rng.uniform(0.1, reach, m) * thres / np.linalg.norm(v, axis=1))[:, None]
            G.append(G[0][k] + v)
        G = np.vstack(G)[rng.permutation(n_bg + sum(sizes))]
        X = (G - A[:, 3]) @ Ainv.T
        if well_separated(world(X, A), thres):
            return X
        seed += 1000


def document(X, seed, first_key=10, key_step=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    names = [f"v{k}.jpg" for k in range(4)]
    cams = np.array([[-3.0 + 2 * k, 0.3 * k, -60.0] for k in range(4)])
    return MS._doc(names, cams, np.asarray(X), [first_key + key_step * i for i in range(len(X))], rng)


def amat(seed=21, scale=2.5):
    return MS.planted(seed=seed, scale=scale)[2]


def reduce_scenes():
    """-> {name: (document, Amat, thres, knn, whether knn binds)}"""
    A = amat()
    line = np.zeros((7, 3))
    line[:, 0] = np.array([0.0, 0.61, 1.27, 1.83, 2.52, 3.11, 3.64]) * THRES   # a chain: neighbours close, others not
    line = (line + [0.3, -0.2, 0.1] - A[:, 3]) @ np.linalg.inv(A[:, :3]).T
    fan = np.array([[0, 0, 0], [0.7, 0, 0], [0, 0.2, 0], [0, 0, -0.5], [300.0, 0, 0]]) * THRES   # 0 keeps 2, 3, 1
    six = np.array([[0, 0, 0], [0.3, 0, 0], [0.1, 0.05, 0], [0.45, 0.1, 0], [0.2, 0.2, 0.15], [0.05, 0.3, 0.2]]) * THRES
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    out = {
        "clusters": (document(clustered(1, A, 40, [1, 2, 3, 4, 2, 1, 3]), 1), A, THRES, 1000, False),
        "chain": (document(line, 2), A, THRES, 1000, False),
        "fan": (document(fan, 3), eye, THRES, 1000, False),
        "six_knn3": (document(six, 4), eye, THRES, 3, True),
        "clusters_knn2": (document(clustered(5, A, 30, [3, 4, 5, 2]), 5), A, THRES, 2, True),
    }
    for name, (doc, Am, thres, _, _) in out.items():
        assert well_separated(world([s["value"]["X"] for s in doc["structure"]], Am), thres), name
    return out


def ref_points(doc, A, n=6, outliers=(4,), seed=9):
    """Ref/refpoints.json for n landmarks of doc: world = A [X; 1] + noise far below the 0.1 threshold; the outliers
    are 5 m off"""
    rng = np.random.Generator(np.random.PCG64(seed))
    st = doc["structure"]
    pick = np.sort(rng.permutation(len(st))[:n])
    pts = []
    for k, i in enumerate(pick):
        X = world(st[i]["value"]["X"], A) + rng.uniform(-1e-3, 1e-3, 3)
        if k in outliers:
            X = X + 5.0
        pts.append({"key": st[i]["key"], "X": X.tolist()})
    return {"refpoints": pts}


def write_project(folder, doc, refpoints=None):
    """-> (project_dir, matches_dir, sfm_data_dir) under folder"""
    proj, sfm, matches = os.path.join(folder, "proj"), os.path.join(folder, "sfm"), os.path.join(folder, "matches")
    for d in (os.path.join(proj, "Ref"), sfm, matches):
        os.makedirs(d, exist_ok=True)
    with open(os.path.join(sfm, "sfm_data.json"), "w") as fh:
        json.dump(doc, fh)
    if refpoints is not None:
        with open(os.path.join(proj, "Ref", "refpoints.json"), "w") as fh:
            json.dump(refpoints, fh)
    return proj, matches, sfm
