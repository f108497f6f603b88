"""The chain of sfmlocalization_amd.incrementalsfm without its adjustment and cleanup steps, composed from the NumPy twins:
the seed pair (seed_np), tracks over all views and the triangulation from the two seed views (structure_np), then growth
rounds (register_np, one round per pass on one State) under OpenMVG's rule -- resect the views with at least 0.75 of the
best view's tracks: min_points = max(10, ceil(0.75 best) - 1) under register's test ">".  The relative poses are the
caller's: the tests seed from the planted ones (incremental_scene.true_relative)."""
import math
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import register_np as RN  # noqa: E402
import seed_np  # noqa: E402
import structure_np as SN  # noqa: E402
from sfmlocalization_amd.structure import track_arrays  # noqa: E402

MAX_ROUNDS = 64


def growth_min_points(best):
    """the 0.75 rule as sfmloc_register_options.min_points (whose test is ">")"""
    return max(10, int(math.ceil(0.75 * best)) - 1)


def kept_counts(a, landmark_keep):
    """sfmloc.h "count" for every view: its observations whose landmark is kept"""
    off = a["obs_off"].astype(np.int64)
    obs_lm = np.repeat(np.arange(len(off) - 1), np.diff(off))
    return np.bincount(a["obs_view"][np.asarray(landmark_keep, bool)[obs_lm]], minlength=len(a["view_id"]))


def seed_poses(a, vi, vj, R, t):
    """the pose table with exactly two valid poses: (I, 0) for view vi and (R, -R^T t) for view vj"""
    n = len(a["pose_valid"])
    pv, pR, pC = np.zeros(n, bool), np.zeros((n, 9)), np.zeros((n, 3))
    R = np.asarray(R, float).reshape(3, 3)
    pi, pj = int(a["view_pose"][vi]), int(a["view_pose"][vj])
    pv[[pi, pj]] = True
    pR[pi], pR[pj] = np.eye(3).reshape(9), R.reshape(9)
    pC[pj] = -(R.T @ np.asarray(t, float))
    return pv, pR, pC


def run(scene, call, rel, oracle_c, use_pair=None, min_used=100, log=None):
    """scene: a register_scene scene; call: incremental_scene.pair_call(scene) without view_wh; rel: rel_R, rel_t,
    inl_off, inl_idx of its pairs -> dict(seed (pair index, -1: none), scores, arrays, pose_valid, pose_R, pose_C, X,
    obs_keep, landmark_keep, rounds [(best, min_points, views registered)], kept_after_seed)"""
    scores = seed_np.seed_scores(**call, **rel, use_pair=use_pair, min_used=min_used)
    k = seed_np.choose(scores, call["pairs"], scene["arrays"]["view_pose"])
    if k < 0:
        return dict(seed=-1, scores=scores)
    t = SN.tracks(call["view_off"], call["pairs"], call["offsets"], call["match_i"], call["match_j"])
    a = track_arrays(scene["arrays"], scene["feats"], t["off"], t["view"], t["feat"])
    vi, vj = (int(v) for v in call["pairs"][k])
    pv, pR, pC = seed_poses(a, vi, vj, rel["rel_R"][k], rel["rel_t"][k])
    tri = SN.triangulate(a, pv, pR, pC)
    X, ok, lk = tri["X"], tri["obs_keep"], tri["landmark_keep"]
    kept_after_seed = int(lk.sum())
    state, rounds = RN.State(len(a["view_id"])), []
    for _ in range(MAX_ROUNDS):
        unposed = ~pv[a["view_pose"]]
        if not unposed.any():
            break
        best = int(kept_counts(a, lk)[unposed].max())
        r = RN.register(a, pv, pR, pC, X, ok, lk, oracle_c, max_rounds=1, min_points=growth_min_points(best), state=state)
        if r["report"]["rounds"] == 0:
            break
        pv, pR, pC, X, ok, lk = (r[f] for f in ("pose_valid", "pose_R", "pose_C", "X", "obs_keep", "landmark_keep"))
        rounds.append((best, growth_min_points(best), list(r["rounds"][0]["registered"])))
        if log:
            log(f"round {len(rounds) - 1}: best {best}, registered {rounds[-1][2]}, {int(lk.sum())} landmarks")
        if not rounds[-1][2]:
            break
    return dict(seed=k, scores=scores, arrays=a, tracks=t, pose_valid=pv, pose_R=pR, pose_C=pC, X=X, obs_keep=ok,
                landmark_keep=lk, rounds=rounds, kept_after_seed=kept_after_seed)
