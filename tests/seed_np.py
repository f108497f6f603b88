"""NumPy restatement of sfmloc_seed_scores (include/sfmloc.h "Seed scores", csrc/seedpair.hip) and of the choice of the
seed pair (csrc/seed_host.h choose): the bearings of the inlier matches, their two-view points, the clamped cosine between
the two rays, its ordered 64-bit key, and the element of rank n_used // 2 of the keys in descending order.  Only
+ - * / sqrt in f64, elementwise and in the stated order (NumPy does not fuse), then integer comparisons: the records are
the device's bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from pairscales_np import two_view_depths  # noqa: E402
from relpose_np import bearings  # noqa: E402

MAX_COS = 0.9986295347545738        # cos 3 degrees
OPTIONS = dict(min_used=100, max_cos=MAX_COS, min_cos=0.5)
LO, HI = -1.0 + 1e-8, 1.0 - 1e-8
TOP = np.uint64(0x8000000000000000)


def cosines(R, b1, b2):
    """sfmloc.h "cosine": the clamped cosine between r1 = (a, b, 1) and r2 = R^T (u, v, 1) of every match; R [9]"""
    a, b, u, v = b1[:, 0], b1[:, 1], b2[:, 0], b2[:, 1]
    with np.errstate(all="ignore"):
        x = (R[0] * u + R[3] * v) + R[6]
        y = (R[1] * u + R[4] * v) + R[7]
        z = (R[2] * u + R[5] * v) + R[8]
        dot = (a * x + b * y) + z
        n1, n2 = np.sqrt((a * a + b * b) + 1.0), np.sqrt((x * x + y * y) + z * z)
        c = dot / (n1 * n2)
        m = np.where(HI < c, HI, c)             # max(LO, min(c, HI)): NaN -> LO
        return np.where(LO < m, m, LO)


def keys(c):
    """sfmloc.h "key": the doubles' bits as unsigned keys that order as the doubles do, -0.0 below +0.0"""
    u = np.ascontiguousarray(c, np.float64).view(np.uint64)
    return np.where(u >> np.uint64(63) != 0, ~u, u | TOP)


def unkeys(k):
    k = np.ascontiguousarray(k, np.uint64)
    return np.where(k >> np.uint64(63) != 0, k & ~TOP, ~k).view(np.float64)


def median_cosine(c):
    """sfmloc.h "median": of the keys in descending order the element of rank n // 2 -> its double; 0.0 for none"""
    if len(c) == 0:
        return 0.0
    k = np.sort(keys(c))[::-1]
    return float(unkeys(k[len(k) // 2: len(k) // 2 + 1])[0])


def pair_cosines(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j, rel_R,
                 rel_t, inl_off, inl_idx, k, cache=None):
    """the clamped cosines of pair k's used inliers, in the order of its inlier list -> (cosines, the number of inliers);
    cache: {view: its bearings}, shared by the pairs of one call"""
    view_off = np.asarray(view_off, np.int64)
    kpt_xy = np.asarray(kpt_xy, np.float32).reshape(-1, 2)
    intrinsics = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    vi, vj = (int(v) for v in np.asarray(pairs, np.int64).reshape(-1, 2)[k])
    R, t = np.asarray(rel_R, np.float64).reshape(-1, 9)[k], np.asarray(rel_t, np.float64).reshape(-1, 3)[k]
    cache = {} if cache is None else cache

    def view_bearings(v, f):
        if v not in cache:
            ii = int(view_intrinsic[v])
            cache[v] = bearings(kpt_xy[view_off[v]:view_off[v + 1]], intrinsics[ii], intrinsic_type[ii])
        return cache[v][f]
    pos = int(offsets[k]) + np.asarray(inl_idx[int(inl_off[k]):int(inl_off[k + 1])], np.int64)
    b1 = view_bearings(vi, np.asarray(match_i, np.int64)[pos])
    b2 = view_bearings(vj, np.asarray(match_j, np.int64)[pos])
    if len(pos) == 0:
        return np.zeros(0), 0
    zi, zj, ok = two_view_depths(R, t, b1, b2)
    with np.errstate(all="ignore"):
        ok = ok & np.isfinite(zj) & (zi > 0.0) & (zj > 0.0)
    return cosines(R, b1[ok], b2[ok]), len(pos)


def seed_scores(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j, rel_R,
                rel_t, inl_off, inl_idx, use_pair=None, min_used=100, max_cos=MAX_COS, min_cos=0.5):
    """The whole call -> [dict(n_inliers, n_used, candidate, cos_median)] per pair; all zero where use_pair is 0"""
    out, cache = [], {}
    for k in range(len(np.asarray(pairs).reshape(-1, 2))):
        if use_pair is not None and not use_pair[k]:
            out.append(dict(n_inliers=0, n_used=0, candidate=0, cos_median=0.0))
            continue
        c, n = pair_cosines(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j,
                            rel_R, rel_t, inl_off, inl_idx, k, cache)
        cm = median_cosine(c)
        out.append(dict(n_inliers=n, n_used=len(c), cos_median=cm,
                        candidate=int(len(c) >= min_used and cm < max_cos and cm > min_cos)))
    return out


def choose(scores, pairs, view_pose):
    """csrc/seed_host.h choose: among the candidates whose two views have different id_pose the smallest cos_median, then
    the larger n_used, then the smaller pair index -> the pair's index, or -1"""
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    ok = [k for k, s in enumerate(scores) if s["candidate"] and view_pose[pairs[k, 0]] != view_pose[pairs[k, 1]]]
    return min(ok, key=lambda k: (scores[k]["cos_median"], -scores[k]["n_used"], k)) if ok else -1
