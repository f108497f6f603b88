"""The synthetic scene of the sfmloc_seed_scores tests: four views of one pool of points, every point a feature of every
view (feature i is point i), and a pair list that is fed R, t and inlier lists directly -- no AC-RANSAC stands before it.

    view 0   the I of every pair (pinhole)
    view 1   pinhole, a step along the arc          view 2   pinhole_radial_k3, two steps along the arc
    view 3   pinhole, 1e-3 of a step from view 0 and turned by 0.1 rad: next to a pure rotation

Every third point (i % 3 == 2) is mirrored through view 0's centre: its two rays meet behind the cameras, so it is not
used, and the points that are used and those that are not interleave.  The pairs, by name:

    n<c>a    c inliers, the points 0 .. c - 1 in a shuffled order, J = view 1
    n<c>b    the same with the last point swapped for one of the other kind (in front <-> behind), so that n_used has the
             other parity, J = view 2 (the radial intrinsic); c = 0 has no b
    rot      200 inliers against view 3: the median cosine is not below max_cos
    dup      4 points in front, each listed 30 times: 120 used inliers, equal keys
    low      two points in front whose cosines were made to agree in all but the lowest byte of their keys by turning the
             pair's R about the y axis (bisection on the angle); listed p q p q q, the median is q's
    off      n256a again with use_pair = 0
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import seed_np as tw  # noqa: E402
from register_scene import PINHOLE, RADIAL, arc_pose, project  # noqa: E402

COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2048, 2049, 5000)
POOL = 5004                       # 5001 and 5003: the points the b pairs swap in, one in front and one behind
FRONT_EXTRA, BEHIND_EXTRA = 5001, 5003


def rot_y(th):
    c, s = np.cos(th), np.sin(th)
    return np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]])


def relative(pose_i, pose_j):
    """X_J = R X_I + t with |t| = 1 from two world poses (R, C)"""
    (Ri, Ci), (Rj, Cj) = pose_i, pose_j
    R = Rj @ Ri.T
    t = Rj @ (Ci - Cj)
    return R, t / np.linalg.norm(t)


def make_scene(seed=60):
    """-> dict(call = the arguments of capi.SeedScores / seed_np.seed_scores, names = the pairs' names, low = (the two
    points of pair `low`, its angle))"""
    rng = np.random.Generator(np.random.PCG64(seed))
    poses = [arc_pose(k, 4) for k in (0, 1, 2)]
    R0, C0 = poses[0]
    poses.append((rot_y(0.1) @ R0, C0 + 1e-3 * 0.15 * 10.0 * R0[0]))
    X = np.stack([rng.uniform(-2, 2, POOL), rng.uniform(-2, 2, POOL), rng.uniform(-1.5, 1.5, POOL)], 1)
    behind = np.arange(POOL) % 3 == 2
    X[behind] = 2.0 * C0 - X[behind]
    K_of = [PINHOLE, PINHOLE, RADIAL, PINHOLE]
    kpt = np.concatenate([np.array([project(K_of[v], X[i], *poses[v]) for i in range(POOL)]) for v in range(4)])
    kpt = kpt.astype(np.float32)
    view_off = np.arange(5, dtype=np.uint64) * POOL
    rel = {j: relative(poses[0], poses[j]) for j in (1, 2, 3)}
    names, pairs, Rs, ts, match, inl, use = [], [], [], [], [], [], []

    def add(name, j, points, R=None, used=1, shuffle=True):
        """a pair (0, j) whose match list is `points` and three more, its inliers the places of `points`"""
        names.append(name)
        pairs.append((0, j))
        Rs.append(rel[j][0] if R is None else R)
        ts.append(rel[j][1])
        pts = np.asarray(points, np.int64)
        extra = np.array([7, 11, 13], np.int64)
        order = rng.permutation(len(pts) + 3) if shuffle else np.arange(len(pts) + 3)
        m = np.concatenate([pts, extra])[order]                    # the match list
        place = np.argsort(order)[:len(pts)]                      # where points[i] went: the inlier list keeps the order
        match.append(m)
        inl.append(place)
        use.append(used)

    for c in COUNTS:
        pts = rng.permutation(c)
        add(f"n{c}a", 1, pts)
        if c:
            swapped = pts.copy()
            swapped[-1] = FRONT_EXTRA if behind[pts[-1]] else BEHIND_EXTRA
            add(f"n{c}b", 2, swapped)
    add("rot", 3, np.arange(200))
    front = np.nonzero(~behind)[0]
    add("dup", 1, np.tile(front[:4], 30))
    low = low_byte_pair(kpt, view_off, rel[1], front[:60])
    add("low", 1, [low[0], low[1], low[0], low[1], low[1]], R=(rot_y(low[2]) @ rel[1][0]), shuffle=False)
    add("off", 1, np.arange(256), used=0)

    offsets = np.concatenate([[0], np.cumsum([len(m) for m in match])]).astype(np.uint64)
    inl_off = np.concatenate([[0], np.cumsum([len(i) for i in inl])]).astype(np.uint64)
    mi = np.concatenate(match).astype(np.uint32)
    call = dict(view_off=view_off, kpt_xy=kpt, view_intrinsic=np.array([0, 0, 1, 0], np.uint32),
                intrinsics=np.array([list(PINHOLE) + [0.0, 0.0, 0.0], list(RADIAL)]),
                intrinsic_type=np.array([0, 3], np.uint32), pairs=np.array(pairs, np.uint32), offsets=offsets,
                match_i=mi, match_j=mi.copy(), rel_R=np.array(Rs).reshape(-1, 9), rel_t=np.array(ts),
                inl_off=inl_off, inl_idx=np.concatenate(inl).astype(np.uint32), use_pair=np.array(use, np.uint8))
    return dict(call=call, names=names, low=low, behind=behind)


def low_byte_pair(kpt, view_off, rel, points):
    """two of `points` and an angle th such that under R = rot_y(th) rel_R their clamped cosines' keys agree in the upper
    seven bytes and differ in the lowest -> (p, q, th) with q's key the smaller.  The cosines of two points that are
    neighbours in cosine order cross as R turns; bisection on th ends where they are a few units in the last place
    apart, and the angles next to that end are tried until the keys differ in the lowest byte alone."""
    K = np.array(list(PINHOLE) + [0.0, 0.0, 0.0])
    b1 = tw.bearings(kpt[int(view_off[0]):int(view_off[1])][points], K, 0)
    b2 = tw.bearings(kpt[int(view_off[1]):int(view_off[2])][points], K, 0)
    R0 = rel[0]

    def cos_at(th, sel):
        return tw.cosines((rot_y(th) @ R0).reshape(9), b1[sel], b2[sel])
    order = np.argsort(cos_at(0.0, np.arange(len(points))))
    span = 0.02
    for a, b in zip(order[:-1], order[1:]):
        sel = np.array([a, b])

        def g(th):
            c = cos_at(th, sel)
            return c[0] - c[1]
        lo, hi = -span, span
        if not g(lo) * g(hi) < 0.0:
            continue
        for _ in range(200):
            mid = 0.5 * (lo + hi)
            if mid == lo or mid == hi:
                break
            if g(lo) * g(mid) <= 0.0:
                hi = mid
            else:
                lo = mid
        th = lo
        for _ in range(64):
            k = tw.keys(cos_at(th, sel))
            if k[0] != k[1] and (k[0] >> np.uint64(8)) == (k[1] >> np.uint64(8)):
                p, q = (a, b) if k[0] > k[1] else (b, a)
                return int(points[p]), int(points[q]), float(th)
            th = np.nextafter(th, -1.0)
    raise AssertionError("no two points whose keys differ in the lowest byte alone")


def sub_call(call, ks):
    """the call with the pairs ks alone (each with its own matches and inliers)"""
    out = dict(call)
    ks = np.asarray(ks, np.int64)
    off, ioff = call["offsets"].astype(np.int64), call["inl_off"].astype(np.int64)
    none = [np.zeros(0, np.uint32)]                                # (so that no pairs at all is a call too)
    out["pairs"] = call["pairs"][ks]
    out["offsets"] = np.concatenate([[0], np.cumsum([off[k + 1] - off[k] for k in ks])]).astype(np.uint64)
    for f in ("match_i", "match_j"):
        out[f] = np.concatenate(none + [call[f][off[k]:off[k + 1]] for k in ks])
    out["inl_off"] = np.concatenate([[0], np.cumsum([ioff[k + 1] - ioff[k] for k in ks])]).astype(np.uint64)
    out["inl_idx"] = np.concatenate(none + [call["inl_idx"][ioff[k]:ioff[k + 1]] for k in ks])
    out["rel_R"], out["rel_t"] = call["rel_R"][ks], call["rel_t"][ks]
    out["use_pair"] = call["use_pair"][ks]
    return out
