"""Time sfmloc_sfm_register (the growth step: unposed views resected against the structure, the structure extended) on
synthetic maps of 100 / 1 000 / 10 000 views with one fifth of the views without a pose.

    timeout -k 10 900 python tools/register_time.py [--views 100,1000,10000] [--runs 3] [--out profiles/register_time.json]

One process.  The maps are tools/ba_separable_time.py's (cameras on a ring around a cube of landmarks, 25 landmarks per
view and 4 observations per landmark, every second view on a pinhole_radial_k3 intrinsic, 0.5 px pixel noise) with the
exact poses; every fifth view loses its pose.  Per run, on a fresh handle: sfmloc_sfm_triangulate (not timed), then one
sfmloc_sfm_register with the default options.  `wall_ms` is the median of --runs host-clock times around that call after
one warm-up of the same shape, `device_ms` the report's figure of the median run.  Nothing is asserted: the figures are
recorded.  The split between K5 and the new kernels comes from a run of this tool under a kernel trace (one size, one
run), summed by kernel name with --trace-stats <the trace's kernel_stats.csv>."""
import argparse
import csv
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import ba_separable_time as BT  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

FIELDS = ("rounds", "views_unposed_in", "views_tried", "views_registered", "obs_extended", "landmarks_tried",
          "landmarks_added")


def make_map(n_views, seed):
    a = BT.make_map(n_views, 25 * n_views, 4, seed, "structure")
    a["pose_valid"] = a["pose_valid"].copy()
    a["pose_valid"][::5] = 0
    return a


def time_case(a, runs):
    out = []
    for k in range(runs + 1):                                  # the first is the warm-up
        h = S.Sfm(**a)
        try:
            tri = h.triangulate()
            t = time.perf_counter()
            rep = h.register()
            dt = (time.perf_counter() - t) * 1e3
            if k:
                out.append((dt, rep.device_ms, {f: int(getattr(rep, f)) for f in FIELDS}, int(tri.landmarks_kept)))
        finally:
            h.close()
    out.sort(key=lambda r: r[0])
    dt, dev, rep, kept = out[len(out) // 2]
    return {"wall_ms": dt, "wall_ms_all": [r[0] for r in out], "device_ms": dev, "landmarks_kept_before": kept, **rep}


def trace_split(path):
    """kernel_stats.csv of a kernel trace -> device microseconds by group: K5 (the P3P kernels), the new kernels
    (k_reg_*, the gang form of the fill), the selective triangulation (k_tri_*), everything else"""
    groups = {"k5_p3p": 0.0, "register_new": 0.0, "triangulate": 0.0, "other": 0.0}
    with open(path) as fh:
        for row in csv.DictReader(fh):
            name, ns = row["Name"], float(row["TotalDurationNs"])
            if "k_reg_" in name or "SfmFillBody" in name or "k_sfm_fill" in name:
                groups["register_new"] += ns
            elif "k_tri_" in name:
                groups["triangulate"] += ns
            elif "p3p" in name.lower() or "P3p" in name:
                groups["k5_p3p"] += ns
            else:
                groups["other"] += ns
    return {k: v / 1e3 for k, v in groups.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", default="100,1000,10000")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "register_time.json"))
    ap.add_argument("--trace-stats", default=None)
    ap.add_argument("--commit", default="")
    args = ap.parse_args()
    if args.trace_stats:
        print(json.dumps(trace_split(args.trace_stats)))
        return 0
    doc = {"commit": args.commit, "runs": args.runs, "cases": []}
    for n in [int(x) for x in args.views.split(",")]:
        a = make_map(n, 7)
        r = {"views": n, "landmarks": len(a["landmark_id"]), "observations": len(a["obs_view"]), **time_case(a, args.runs)}
        print(json.dumps(r), flush=True)
        doc["cases"].append(r)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
