"""Times sfmloc_seed_scores at two pair sizes and writes profiles/seedpair_time.json: device milliseconds
(sfmloc_seed_last_ms) of 1 000 pairs of 1 000 inliers and of 1 000 pairs of 20 inliers, every repeat recorded after a
warm-up call, and whether the NumPy restatement (tests/seed_np.py) gives the same bits on a sample of the pairs.  The
second size is the question DESIGN section 8 asks: a pair of 20 inliers leaves most of its workgroup of 256 idle, and
whether a one-wave form for small pairs would pay is read off these two rows.  No threshold is set: the record is the
deliverable.

    python tools/seedpair_time.py [--pairs 1000] [--repeats 5] [--out profiles/seedpair_time.json]
                                  [--commit LABEL] [--device-name LABEL]

The scene: two pinhole views 1.2 apart looking at 4 000 points 8 to 12 in front of them, every point a feature of both
views; a pair is the view pair (0, 1) with its own random choice of the points as matches, all of them inliers, under
the planted relative pose."""
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

from sfmlocalization_amd import capi  # noqa: E402

F, PPX, PPY, POOL, BASELINE = 700.0, 320.0, 240.0, 4000, 1.2


def make_call(n_pairs, n_inliers, seed=3):
    rng = np.random.default_rng(seed)
    X = np.stack([rng.uniform(-2, 2, POOL), rng.uniform(-2, 2, POOL), rng.uniform(8, 12, POOL)], 1)
    C = np.array([BASELINE, 0.0, 0.0])
    px = [F * Xc[:, :2] / Xc[:, 2:] + np.array([PPX, PPY]) for Xc in (X, X - C)]
    m = np.stack([rng.permutation(POOL)[:n_inliers] for _ in range(n_pairs)]).astype(np.uint32).reshape(-1)
    off = (np.arange(n_pairs + 1) * n_inliers).astype(np.uint64)
    return dict(view_off=np.array([0, POOL, 2 * POOL], np.uint64), kpt_xy=np.concatenate(px).astype(np.float32),
                view_intrinsic=np.zeros(2, np.uint32), intrinsics=np.array([[F, PPX, PPY, 0.0, 0.0, 0.0]]),
                intrinsic_type=np.zeros(1, np.uint32), pairs=np.tile(np.array([[0, 1]], np.uint32), (n_pairs, 1)),
                offsets=off, match_i=m, match_j=m.copy(), rel_R=np.tile(np.eye(3).reshape(1, 9), (n_pairs, 1)),
                rel_t=np.tile(np.array([[-1.0, 0.0, 0.0]]), (n_pairs, 1)), inl_off=off,
                inl_idx=np.tile(np.arange(n_inliers, dtype=np.uint32), n_pairs))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seedpair_time.json"))
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    ap.add_argument("--device-name", default="HIP device 0", help="the record's device label, written as given")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("seedpair_time.py needs a HIP device: a time taken without one says nothing")
    import seed_np
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    rows = []
    for n_inliers in (1000, 20):
        call = make_call(a.pairs, n_inliers)
        capi.SeedScores(**call, min_used=10)                              # (the first call pays the code object's load)
        ms, wall = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            s = capi.SeedScores(**call, min_used=10)
            wall.append(time.perf_counter() - t0)
            ms.append(s.ms)
        sample = [0, a.pairs // 2, a.pairs - 1]
        same = True
        for k in sample:
            c, _ = seed_np.pair_cosines(*[call[f] for f in ("view_off", "kpt_xy", "view_intrinsic", "intrinsics",
                                                            "intrinsic_type", "pairs", "offsets", "match_i", "match_j",
                                                            "rel_R", "rel_t", "inl_off", "inl_idx")], k)
            same = same and len(c) == int(s.scores["n_used"][k]) and \
                np.float64(seed_np.median_cosine(c)).tobytes() == s.scores["cos_median"][k].tobytes()
        rows.append({"pairs": a.pairs, "inliers_per_pair": n_inliers, "device_ms": {"all": ms, "best": min(ms)},
                     "wall_s_best": min(wall), "microseconds_per_pair_best": 1000.0 * min(ms) / a.pairs,
                     "candidates": int(s.scores["candidate"].sum()), "n_used_total": int(s.scores["n_used"].sum()),
                     "numpy_restatement": {"pairs_compared": sample, "same_bits_as_device": bool(same)}})
    doc = {"commit": commit, "device": a.device_name, "rows": rows,
           "note": "device_ms holds the uploads of the scene and the read-back of the records beside the one kernel"}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
