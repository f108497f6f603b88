"""The path scene of the incremental-SfM tests, on register_scene.build: ten views on an arc (arc_pose, step 0.12), none
with a pose, 240 points each seen by four consecutive views, and a match file that holds the pairs (k, k + 1) alone -- a
walking video whose frames match only their neighbours.  The pair graph is a path: it has no triplet, so rotation and
translation averaging cannot pose it.  View 4 is on the pinhole_radial_k3 intrinsic.  The points that start at view
0 .. 6 number STARTS, so that the pairs in the middle of the path share more than 100 points (the default gate of the
seed choice) with some to spare for AC-RANSAC.

Beside the scene: the arguments of the pair-side calls from a register_scene scene (pair_call), the true relative
poses with every match an inlier (true_relative: what the CPU prototype seeds from), and the similarity alignment the
accuracy tests measure with (centre_errors)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import register_scene as RS  # noqa: E402

N_VIEWS = 10
STEP = 0.12
SPAN = 4                                    # consecutive views that see a point
STARTS = (28, 30, 42, 40, 42, 30, 28)       # points whose first view is 0 .. 6: 240 in all
RADIAL_VIEW = 4


def make_scene_path(seed=70, noise=None):
    """noise: the pixel noise in place of register_scene.NOISE (0: pixels at .feat precision)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    poses = [RS.arc_pose(k, N_VIEWS, step=STEP) for k in range(N_VIEWS)]
    X = RS.cloud(rng, sum(STARTS))
    first = np.repeat(np.arange(len(STARTS)), STARTS)
    first = first[rng.permutation(len(first))]
    sees = {p: [(int(first[p]) + i, RS.OK) for i in range(SPAN)] for p in range(len(first))}
    saved = RS.NOISE
    try:
        if noise is not None:
            RS.NOISE = noise
        sc = RS.build(rng, poses, [False] * N_VIEWS, {RADIAL_VIEW}, X, sees, pair_ok=lambda ka, kb: kb == ka + 1)
    finally:
        RS.NOISE = saved
    sc["first"] = first
    return sc


def pair_call(scene):
    """the arguments of capi.RelPoses for a register_scene scene (without view_wh: those of the other pair-side calls)"""
    from sfmlocalization_amd import capi
    a = scene["arrays"]
    index = {int(v): k for k, v in enumerate(a["view_id"])}
    pairs, offsets, mi, mj = capi.pair_arrays(scene["matches"], index)
    feats = scene["feats"]
    return dict(view_off=np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64),
                kpt_xy=np.concatenate([f[:, :2] for f in feats]).astype(np.float32),
                view_wh=np.tile(np.array([640, 480], np.uint32), (len(feats), 1)), view_intrinsic=a["view_intrinsic"],
                intrinsics=a["intrinsic"], intrinsic_type=a["intrinsic_type"], pairs=pairs, offsets=offsets, match_i=mi,
                match_j=mj)


def true_relative(scene, call):
    """the planted relative pose of every pair of the call (X_J = R X_I + t, |t| = 1) with all its matches as inliers ->
    dict(rel_R [P, 9], rel_t [P, 3], inl_off, inl_idx)"""
    Rs, ts = [], []
    for vi, vj in np.asarray(call["pairs"], np.int64):
        (Ri, Ci), (Rj, Cj) = scene["poses"][vi], scene["poses"][vj]
        t = Rj @ (Ci - Cj)
        Rs.append((Rj @ Ri.T).reshape(9))
        ts.append(t / np.linalg.norm(t))
    off = np.asarray(call["offsets"], np.int64)
    return dict(rel_R=np.array(Rs), rel_t=np.array(ts), inl_off=call["offsets"],
                inl_idx=np.concatenate([np.arange(off[k + 1] - off[k]) for k in range(len(off) - 1)]).astype(np.uint32))


def triplets(pairs):
    """the triangles of the pair graph"""
    e = {tuple(sorted((int(a), int(b)))) for a, b in pairs}
    v = sorted({x for p in e for x in p})
    return [(a, b, c) for a in v for b in v for c in v if a < b < c and (a, b) in e and (b, c) in e and (a, c) in e]


def centre_errors(C, C_true):
    """the similarity (scale, rotation, translation: Umeyama's closed form) that takes the centres C [n, 3] nearest to
    C_true, then every centre's distance to the truth in units of the mean distance between consecutive true centres"""
    C, T = np.asarray(C, float), np.asarray(C_true, float)
    mc, mt = C.mean(0), T.mean(0)
    A, B = C - mc, T - mt
    U, S, Vt = np.linalg.svd(B.T @ A / len(C))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U) * np.linalg.det(Vt))])
    R = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / (A * A).sum() * len(C)
    err = np.linalg.norm((s * (R @ A.T).T + mt) - T, axis=1)
    return err / np.linalg.norm(np.diff(T, axis=0), axis=1).mean()
