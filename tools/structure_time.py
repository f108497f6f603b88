"""Times the tracks and the triangulation of structure-from-known-poses on synthetic corridors and writes
profiles/structure_time.json: the device time of sfmloc_tracks_build (sfmloc_tracks_last_ms: its kernels and copies) and
of sfmloc_sfm_triangulate (the report's device_ms), robust and blind, at 10^2, 10^3 and 10^4 views, about 2 000 features
per view, every view matched to its next 5 neighbours -- and beside them the NumPy restatement (tests/structure_np.py)
at the sizes it finishes within a budget.  No speed-up is promised; the file holds the numbers.

    python tools/structure_time.py [--sizes 100,1000,10000] [--out profiles/structure_time.json] [--numpy-budget 60]

The corridor: cameras 0.5 m apart on a line, all looking the same way, every world point seen by 2..10 consecutive
cameras at 0.3 px noise (so a view holds about 2 000 features and a track has 2 to 10 observations).  Each call is
repeated after a warm-up call (the first one pays the code object's load); every repeat is recorded."""
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

import structure_np as tw  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

F, PPX, PPY = 700.0, 320.0, 240.0
NEIGHBOURS = 5


def corridor(seed, n_views, feats_per_view=2000):
    """-> (view_off, pairs, offsets, match_i, match_j, arrays without structure, pixel of every feature row [rows, 2])"""
    rng = np.random.Generator(np.random.PCG64(seed))
    n_pts = int(n_views * feats_per_view / 6.0)
    L = rng.integers(2, 11, n_pts)
    start = rng.integers(-4, n_views - 1, n_pts)
    lo, hi = np.maximum(start, 0), np.minimum(start + L, n_views)
    ok = hi - lo >= 1
    lo, hi = lo[ok], hi[ok]
    n_pts = len(lo)
    cnt = hi - lo
    off = np.concatenate([[0], np.cumsum(cnt)])
    pt = np.repeat(np.arange(n_pts), cnt)
    view = (np.arange(off[-1]) - np.repeat(off[:-1], cnt) + np.repeat(lo, cnt)).astype(np.int64)
    X = np.stack([(lo + hi - 1) * 0.25 + rng.uniform(-1.5, 1.5, n_pts), rng.uniform(-2, 2, n_pts),
                  rng.uniform(5, 15, n_pts)], 1)
    px = np.stack([F * (X[pt, 0] - 0.5 * view) / X[pt, 2] + PPX, F * X[pt, 1] / X[pt, 2] + PPY], 1) \
        + rng.normal(0, 0.3, (len(pt), 2))
    order = np.argsort(view, kind="stable")                     # feature rows: view-major, point order inside a view
    row_of_obs = np.empty(len(order), np.int64)
    row_of_obs[order] = np.arange(len(order))
    view_off = np.concatenate([[0], np.cumsum(np.bincount(view, minlength=n_views))]).astype(np.uint64)
    feat_of_obs = row_of_obs - view_off[view].astype(np.int64)
    key, mi, mj = [], [], []
    o = np.arange(off[-1])
    for d in range(1, NEIGHBOURS + 1):                          # obs o and o + d of one point: views v and v + d
        sel = o[(o + d) < np.repeat(off[1:], cnt)]
        key.append(view[sel] * NEIGHBOURS + (d - 1))
        mi.append(feat_of_obs[sel])
        mj.append(feat_of_obs[sel + d])
    key, mi, mj = np.concatenate(key), np.concatenate(mi), np.concatenate(mj)
    srt = np.argsort(key, kind="stable")
    key, mi, mj = key[srt], mi[srt].astype(np.uint32), mj[srt].astype(np.uint32)
    uniq, counts = np.unique(key, return_counts=True)
    pairs = np.stack([uniq // NEIGHBOURS, uniq // NEIGHBOURS + uniq % NEIGHBOURS + 1], 1).astype(np.uint32)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    R = np.tile(np.eye(3).reshape(9), (n_views, 1))
    C = np.zeros((n_views, 3))
    C[:, 0] = 0.5 * np.arange(n_views)
    ids = np.arange(n_views, dtype=np.uint32)
    arrays = dict(view_id=ids, view_intrinsic=np.zeros(n_views, np.uint32), view_pose=ids,
                  intrinsic_type=np.zeros(1, np.uint32), intrinsic=np.array([[F, PPX, PPY, 0, 0, 0]]),
                  pose_valid=np.ones(n_views, np.uint8), pose_R=R, pose_C=C)
    row_px = np.empty_like(px)
    row_px[row_of_obs] = px
    return view_off, pairs, offsets, mi, mj, arrays, row_px


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100,1000,10000")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_time.json"))
    ap.add_argument("--numpy-budget", type=float, default=60.0)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("structure_time.py needs a HIP device: a time taken without one says nothing")
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    rows, numpy_ok = [], True
    for n_views in [int(x) for x in a.sizes.split(",")]:
        t0 = time.perf_counter()
        view_off, pairs, offsets, mi, mj, arrays, row_px = corridor(1, n_views)
        gen_s = time.perf_counter() - t0
        row = {"views": n_views, "feature_rows": int(view_off[-1]), "pairs": int(len(pairs)), "matches": int(len(mi)),
               "generate_s": gen_s}
        capi.Tracks(view_off, pairs, offsets, mi, mj)                                # warm-up
        calls = []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            t = capi.Tracks(view_off, pairs, offsets, mi, mj)
            calls.append({"device_ms": t.ms, "wall_ms": (time.perf_counter() - t0) * 1e3})
        row.update(tracks=t.counts[3], components=t.counts[0], observations=int(t.off[-1]), tracks_calls=calls)
        arr = dict(arrays)
        arr.update(landmark_id=np.arange(t.n_tracks, dtype=np.uint32), landmark_X=np.zeros((t.n_tracks, 3)),
                   obs_off=t.off, obs_view=t.view, obs_x=row_px[view_off[t.view].astype(np.int64) + t.feat])
        t0 = time.perf_counter()
        h = capi.Sfm(**arr)
        row["sfm_create_s"] = time.perf_counter() - t0
        try:
            for mode, name in ((capi.TRI_ROBUST, "robust"), (capi.TRI_BLIND, "blind")):
                h.triangulate(mode=mode)                                              # warm-up
                reps = [h.triangulate(mode=mode) for _ in range(a.repeats)]
                row["triangulate_" + name] = {"device_ms": [r.device_ms for r in reps], "kept": int(reps[-1].landmarks_kept),
                                              "rounds": int(reps[-1].rounds), "obs_kept": int(reps[-1].obs_kept)}
            X = h.read_structure()
        finally:
            h.close()
        if numpy_ok:
            t0 = time.perf_counter()
            e = tw.tracks(view_off, pairs, offsets, mi, mj)
            row["numpy_tracks_s"] = time.perf_counter() - t0
            row["numpy_tracks_equal"] = bool(e["counts"] == t.counts and np.array_equal(e["view"], t.view)
                                             and np.array_equal(e["feat"], t.feat))
            t0 = time.perf_counter()
            r = tw.triangulate(arr, arrays["pose_valid"], arrays["pose_R"], arrays["pose_C"], mode=tw.BLIND)
            row["numpy_triangulate_blind_s"] = time.perf_counter() - t0
            row["numpy_triangulate_blind_equal"] = bool(np.array_equal(
                np.ascontiguousarray(r["X"]).view(np.uint64), np.ascontiguousarray(X).view(np.uint64)))
            # the robust restatement loops over landmarks in Python: run only where it fits the budget
            if row["numpy_triangulate_blind_s"] * 8 < a.numpy_budget:
                t0 = time.perf_counter()
                tw.triangulate(arr, arrays["pose_valid"], arrays["pose_R"], arrays["pose_C"])
                row["numpy_triangulate_robust_s"] = time.perf_counter() - t0
            numpy_ok = (row["numpy_tracks_s"] + row["numpy_triangulate_blind_s"]) * 10 < a.numpy_budget
        print(json.dumps(row), flush=True)
        rows.append(row)
        with open(a.out, "w") as fh:                                                   # (kept up to date size by size)
            json.dump({"commit": commit, "features_per_view": 2000, "neighbours": NEIGHBOURS, "sizes": rows}, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
