"""Time the device half of the map merge (sfmloc_merge_*): the RANSAC over 3D-3D matches at n = 1 000 and 10 000 with
n x 100 rounds (what mergeModel runs), both models, and the nearest-other-point median at 10^5 and 10^6 points.

    timeout -k 10 900 python tools/merge_time.py [--runs 5] [--out profiles/merge_times.json]

One process.  Each figure is the median of --runs calls after one warm-up call of the same shape: `device_ms` is the
time between HIP events around the call's kernels (params.profile = 1: the round launches, the winner, the inlier list
and the final fit; for the median the all-pairs kernel and the radix select with its 16 small read-backs), `call_ms`
the host clock around the whole call (allocation, upload and read-back included; the call ends synchronised).  Beside
each, for orientation only, the same workload in the NumPy restatement (tests/merge_np.py) on this host: timed on a
slice (--cpu-rounds rounds, --cpu-rows rows of the all-pairs matrix) and scaled linearly, which is what the key says."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import merge_np as MN  # noqa: E402
import merge_scene as MS  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402


def timed(fn, runs):
    fn()                                                   # warm-up: code objects, the first allocations
    dev, call = [], []
    for _ in range(runs):
        t = time.perf_counter()
        fn()
        call.append((time.perf_counter() - t) * 1e3)
        dev.append(S.merge_last_ms())
    return {"device_ms": statistics.median(dev), "call_ms": statistics.median(call), "device_ms_all": dev}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--cpu-rounds", type=int, default=2048)
    ap.add_argument("--cpu-rows", type=int, default=1024)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_times.json"))
    a = ap.parse_args()
    if S.device_count() < 1:
        raise SystemExit("merge_time needs a HIP device: nothing here is a CPU figure of the product")
    p = S.merge_default_params(profile=1)
    seed = int(p.seed)
    out = {"runs": a.runs, "ransac": [], "median_nn": []}
    for n in (1000, 10000):
        A, B, _, inl = MS.planted(seed=21, n=n, n_in=(6 * n) // 10)
        rounds = n * 100
        for name, model in (("similarity", MN.SIMILARITY), ("affine", MN.AFFINE)):
            res = {}

            def call():
                res["r"] = S.merge_ransac(A, B, MS.THRES, rounds, 1.75, model, params=p)
            rec = {"n": n, "rounds": rounds, "model": name}
            rec.update(timed(call, a.runs))
            assert np.array_equal(res["r"]["inliers"], inl), "the planted inlier set did not come back"
            rec["pair_tests_per_s"] = n * rounds / (rec["device_ms"] * 1e-3)
            t = time.perf_counter()
            MN.ransac(A, B, MS.THRES, a.cpu_rounds, 1.75, model, seed)
            rec["merge_np_host_s_scaled_from_rounds"] = a.cpu_rounds
            rec["merge_np_host_s"] = (time.perf_counter() - t) * rounds / a.cpu_rounds
            out["ransac"].append(rec)
            print(json.dumps(rec), flush=True)
    rng = np.random.Generator(np.random.PCG64(4))
    for n in (100000, 1000000):
        X = rng.uniform(-200, 200, (n, 3))
        rec = {"n": n}
        rec.update(timed(lambda: S.merge_median_nn(X, params=p), a.runs))
        rec["pairs_per_s"] = n * n / (rec["device_ms"] * 1e-3)
        t = time.perf_counter()
        rows = X[:a.cpu_rows]
        for i0 in range(0, a.cpu_rows, 64):
            P = rows[i0:i0 + 64]
            d2 = ((P[:, None, 0] - X[None, :, 0]) ** 2 + (P[:, None, 1] - X[None, :, 1]) ** 2) + \
                (P[:, None, 2] - X[None, :, 2]) ** 2
            d2.min(1)
        rec["merge_np_host_s_scaled_from_rows"] = a.cpu_rows
        rec["merge_np_host_s"] = (time.perf_counter() - t) * n / a.cpu_rows
        out["median_nn"].append(rec)
        print(json.dumps(rec), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
