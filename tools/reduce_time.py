"""Time sfmloc_reduce_points at 10^4, 10^5 and 10^6 synthetic landmarks: uniform in a 50 m cube, 5 % of them planted
within 8 mm of another landmark; thres 0.01, knn 1000 (what --reduce-points runs).

    timeout -k 10 900 python tools/reduce_time.py [--runs 5] [--out profiles/reduce_times.json]

One process.  Each figure is the median of --runs calls after one warm-up call of the same shape: `device_ms` is the
time between HIP events around the call's kernels and the host checks between them (params.profile = 1), `call_ms` the
host clock around the whole call (allocation, upload and read-back included).  `rounds` and `n_pairs` are the call's.
Beside each, for orientation only, a host run of the same rule on scipy's cKDTree.query_pairs (pairs within thres, then
the greedy loop over them in index order; knn does not bind on this data, asserted): it must return the same owners."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sfmlocalization_amd import capi as S  # noqa: E402

THRES, KNN = 0.01, 1000


def landmarks(n, seed=8):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.uniform(0.0, 50.0, (n, 3))
    k = n // 20
    at = rng.permutation(n)
    X[at[:k]] = X[at[k:2 * k]] + rng.uniform(-0.0045, 0.0045, (k, 3))
    return X


def host_rule(X):
    from scipy.spatial import cKDTree
    pairs = cKDTree(X).query_pairs(THRES, output_type="ndarray")
    d = X[pairs[:, 0]] - X[pairs[:, 1]]
    d = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
    pairs, d = pairs[d < THRES], d[d < THRES]
    order = np.lexsort((pairs[:, 1], d, pairs[:, 0]))
    owner = np.arange(len(X), dtype=np.uint32)
    for i, j in pairs[order]:
        if owner[i] == i and owner[j] == j:
            owner[j] = i
    return owner, len(pairs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_times.json"))
    a = ap.parse_args()
    if S.device_count() < 1:
        raise SystemExit("reduce_time needs a HIP device: nothing here is a CPU figure of the product")
    p = S.merge_default_params(profile=1)
    out = {"runs": a.runs, "thres": THRES, "knn": KNN, "reduce_points": []}
    for n in (10000, 100000, 1000000):
        X = landmarks(n)
        res = S.reduce_points(X, None, THRES, KNN, params=p)                  # warm-up
        dev, call = [], []
        for _ in range(a.runs):
            t = time.perf_counter()
            res = S.reduce_points(X, None, THRES, KNN, params=p)
            call.append((time.perf_counter() - t) * 1e3)
            dev.append(S.reduce_last_ms())
        rec = {"n": n, "device_ms": statistics.median(dev), "call_ms": statistics.median(call), "device_ms_all": dev,
               "rounds": res["rounds"], "n_pairs": res["n_pairs"], "n_absorbed": res["n_absorbed"]}
        t = time.perf_counter()
        owner, n_pairs = host_rule(X)
        rec["ckdtree_query_pairs_host_s"] = time.perf_counter() - t
        assert n_pairs == res["n_pairs"] and np.array_equal(owner, res["owner"]), "the host rule disagrees"
        out["reduce_points"].append(rec)
        print(json.dumps(rec), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
