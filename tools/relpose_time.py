"""Device time of sfmloc_relative_poses on the synthetic corridor of tools/structure_time.py (10 000 views by default):
device ms from sfmloc_relpose_last_ms, pairs/s, the rounds (of the restatement's subset, which carries the device's bits:
the C record has no rounds field) and the pairs that end ok, written to profiles/relpose_time.json.  OpenMVG
was not run and the reference has no number for this stage; the NumPy figure beside it is the restatement
(tests/relpose_np.py) on a 1 % subset of the pairs, not a competing implementation.

    python tools/relpose_time.py [--views 10000] [--repeats 3] [--out profiles/relpose_time.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import relpose_np as tw  # noqa: E402
from structure_time import corridor  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-pairs", type=int, default=0, help="pairs of the restatement's subset (default: 1 %%, at most 50)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relpose_time.json"))
    ap.add_argument("--commit", default=None)
    a = ap.parse_args()
    view_off, pairs, offsets, mi, mj, arrays, px = corridor(7, a.views)
    n_views = len(view_off) - 1
    args = dict(view_off=view_off, kpt_xy=px.astype(np.float32), view_wh=np.tile(np.array([640, 480], np.uint32), (n_views, 1)),
                view_intrinsic=arrays["view_intrinsic"], intrinsics=arrays["intrinsic"], intrinsic_type=arrays["intrinsic_type"],
                pairs=pairs, offsets=offsets, match_i=mi, match_j=mj)
    ms, wall = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        r = capi.RelPoses(**args)
        wall.append(time.perf_counter() - t0)
        ms.append(r.ms)
    per = np.diff(offsets.astype(np.int64))
    rec = {"what": "sfmloc_relative_poses on the synthetic corridor of tools/structure_time.py, one MI355X; device_ms = "
                   "sfmloc_relpose_last_ms (HIP events around the call's kernels and copies), best of the repeats",
           "commit": a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True,
                                                 text=True).stdout.strip(),
           "views": n_views, "feature_rows": int(view_off[-1]), "pairs": len(pairs), "matches": int(offsets[-1]),
           "matches_per_pair": {"min": int(per.min()), "median": float(np.median(per)), "max": int(per.max())},
           "max_iteration": 256, "device_ms": {"all": ms, "best": min(ms)}, "call_s": {"all": wall, "best": min(wall)},
           "pairs_per_s_device": len(pairs) / (min(ms) * 1e-3), "pairs_ok": int(r.results["ok"].sum()),
           "inliers": int(r.results["n_inliers"].sum()),
           "note": "OpenMVG was not run; the reference has no number for this stage"}
    n_np = a.numpy_pairs or min(50, max(1, len(pairs) // 100))
    sel = np.linspace(0, len(pairs) - 1, n_np).astype(np.int64)
    off = offsets.astype(np.int64)
    sub = dict(args, pairs=pairs[sel], offsets=np.concatenate([[0], np.cumsum(per[sel])]).astype(np.uint64),
               match_i=np.concatenate([mi[off[k]:off[k + 1]] for k in sel]),
               match_j=np.concatenate([mj[off[k]:off[k + 1]] for k in sel]))
    t0 = time.perf_counter()
    res = tw.relative_poses(**sub)
    t_np = time.perf_counter() - t0
    rounds = [x["rounds"] for x in res]
    same = all(int(x["n_inliers"]) == int(r.results[k]["n_inliers"]) and
               np.array_equal(np.asarray(x["R"]).view(np.uint64), r.results[k]["R"].view(np.uint64)) for x, k in zip(res, sel))
    rec["numpy_restatement"] = {"pairs": int(n_np), "seconds": t_np, "pairs_per_s": n_np / t_np,
                                "same_bits_as_device": bool(same)}
    # (sfmloc_relpose_result has no rounds field: the rounds are the restatement's on the subset, which are the device's
    # when its results carry the device's bits -- the loop's trip count is a function of the same comparisons)
    rec["rounds"] = {"per_pair": {"min": int(min(rounds)), "max": int(max(rounds)), "mean": float(np.mean(rounds))},
                     "pairs_counted": int(n_np), "all_pairs_estimate": float(np.mean(rounds)) * len(pairs),
                     "source": "the restatement on the subset; the device's when same_bits_as_device"}
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
