"""The sequential twin of sfmloc_reduce_points (include/sfmloc.h "Thinning a map fixed to world coordinates") and of
the device entry points sfmlocalization_amd.globalcoord uses: the plain greedy loop of reduceClosePointsKDTree
(PyEvaluateAccuracy/src/localizeGlobalCoordinateRefPoint.py:81-118) over all-pairs distances, one row at a time, with
exactly the header's arithmetic (f64, unfused, one expression per value).  No grid, no passes: the GPU tests compare the
device's bits with this."""
import numpy as np

import merge_np as MN

NONE = 0xFFFFFFFF
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def global_coords(X, A=None):
    """G_i = ((a_i0 x0 + a_i1 x1) + a_i2 x2) + a_i3; A = None is the identity through the same expression"""
    X = np.ascontiguousarray(X, np.float64).reshape(-1, 3)
    A = IDENTITY if A is None else np.asarray(A, np.float64).reshape(3, 4)
    G = np.empty_like(X)
    for i in range(3):
        G[:, i] = ((A[i, 0] * X[:, 0] + A[i, 1] * X[:, 1]) + A[i, 2] * X[:, 2]) + A[i, 3]
    return G


def distances(G, i):
    d = G[i] - G
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def close_sets(G, thres, knn):
    """C(i) with its distances, in N(i)'s order: N(i) = the min(knn, n) nearest by (d, index), i included"""
    n = len(G)
    rows = []
    for i in range(n):
        d = distances(G, i)
        idx = np.arange(n)
        near = np.lexsort((idx, d))[:min(knn, n)]
        near = near[(near > i) & (d[near] < thres)]
        rows.append((near, d[near]))
    return rows


def reduce_points(X, A=None, thres=0.01, knn=1000):
    """-> the dict capi.reduce_points returns"""
    if not (np.isfinite(thres) and thres > 0):
        raise ValueError("threshold")
    G = global_coords(X, A)
    if not (np.isfinite(np.asarray(X, np.float64)).all() and (A is None or np.isfinite(np.asarray(A, np.float64)).all())):
        raise ValueError("not finite")
    n = len(G)
    owner = np.arange(n, dtype=np.uint32)
    dist = np.zeros(n)
    if n < 2:
        return {"owner": owner, "order": np.zeros(0, np.uint32), "dist": dist, "n_keep": n, "n_absorbed": 0, "n_pairs": 0,
                "rounds": 0}
    rows = close_sets(G, thres, knn)
    absorbed = np.zeros(n, bool)
    level = np.ones(n, np.int64)          # the pass that decides i: one after the last of the points that list it
    order = []
    for i in range(n):                    # the reference's loop
        for j in rows[i][0]:
            level[j] = max(level[j], level[i] + 1)
        if absorbed[i]:
            continue
        for j, d in zip(*rows[i]):
            if not absorbed[j]:
                absorbed[j] = True
                owner[j] = i
                dist[j] = d
                order.append(j)
    return {"owner": owner, "order": np.array(order, np.uint32), "dist": dist, "n_keep": int(n - absorbed.sum()),
            "n_absorbed": int(absorbed.sum()), "n_pairs": int(sum(len(r[0]) for r in rows)), "rounds": int(level.max())}


class Ops(MN.Ops):
    """The device entry points of sfmlocalization_amd.globalcoord on the host."""

    def reduce_points(self, X, A=None, thres=0.01, knn=1000):
        return reduce_points(X, A, thres, knn)
