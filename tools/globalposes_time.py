"""Times sfmloc_global_poses on the pair graph of the corridor of tools/structure_time.py and writes
profiles/globalposes_time.json: device milliseconds per phase (triplets + component, chordal + IRLS, translation), PCG
iterations, steps and launches from the call's report, every repeat recorded after a warm-up call -- and beside them the
time of the NumPy restatement (tests/globalposes_np.py) on the same arrays where it finishes within a budget: a
restatement, not a competitor.  No threshold is set: nobody has measured this stage, the record is the deliverable.

    python tools/globalposes_time.py [--views 10000] [--repeats 3] [--numpy-views 1000] [--out profiles/globalposes_time.json]
                                     [--commit LABEL] [--device-name LABEL]

The two labels are written as given (the library has no getter for a device's name; a commit label that ends in "+"
is that commit with the change that adds this tool on top, as in `git describe --dirty`).  profiles/globalposes_time.json is
the run at 10 000 views, profiles/globalposes_time_1000.json the one at 1 000 views, where the restatement runs too.

The corridor: cameras 0.5 m apart on a line, all looking the same way, every view paired with its next 5 neighbours; the
relative poses are the planted ones with 0.2 degrees of rotation noise and 0.005 rad of direction noise.  The cameras
are collinear: the spacing along the line is the case include/sfmloc.h "Known limit" describes, and the record shows
what the translation stage costs and leaves there (centre error after the similarity alignment, over the extent)."""
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

import globalposes_np as tw  # noqa: E402
import globalposes_scene as sc  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402
from sfmlocalization_amd.globalposes import REPORT_FIELDS  # noqa: E402

NEIGHBOURS = 5


def corridor_poses(n_views, seed=11):
    """the scene dict of tests/globalposes_scene.py for the corridor's pair graph"""
    rng = np.random.default_rng(seed)
    R = np.tile(np.eye(3), (n_views, 1, 1))
    C = np.zeros((n_views, 3))
    C[:, 0] = 0.5 * np.arange(n_views)
    plist = [(v, v + d) for v in range(n_views) for d in range(1, NEIGHBOURS + 1) if v + d < n_views]
    return sc.build(R, C, plist, rng, np.radians(0.2), 0.005)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-views", type=int, default=1000, help="the restatement runs when --views is at most this")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "globalposes_time.json"))
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    ap.add_argument("--device-name", default="HIP device 0", help="the record's device label, written as given")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("globalposes_time.py needs a HIP device: a time taken without one says nothing")
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    s = corridor_poses(a.views)

    def call():
        t0 = time.perf_counter()
        g = capi.GlobalPoses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"])
        return g, time.perf_counter() - t0
    call()                                                      # (the first call pays the code object's load)
    runs = []
    for _ in range(a.repeats):
        g, wall = call()
        row = {k: getattr(g.report, k) for k in REPORT_FIELDS}
        row["wall_s"] = wall
        row["rotation_error_deg"], row["centre_error"] = sc.errors(s, g.in_component, int(g.report.root), g.R, g.C)
        runs.append(row)
    doc = {"commit": commit, "device": a.device_name,
           "views": a.views, "pairs": int(len(s["pairs"])), "neighbours": NEIGHBOURS, "runs": runs,
           "numpy": None, "numpy_note": "a restatement, not a competitor"}
    if a.views <= a.numpy_views:
        t0 = time.perf_counter()
        o = tw.global_poses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"])
        doc["numpy"] = {"wall_s": time.perf_counter() - t0, "rot_pcg_total": o["rot_pcg_total"],
                        "trans_pcg_total": o["trans_pcg_total"], "trans_steps_tried": o["trans_steps_tried"]}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: doc[k] for k in ("views", "pairs", "numpy")}), json.dumps(runs[-1]))


if __name__ == "__main__":
    main()
