"""Time sfmloc_sfm_adjust_joint (the joint bundle adjustment) on synthetic maps of 100 / 1 000 / 10 000 views with 25
landmarks per view and 4 observations per landmark, for rst and rsti at the default options, beside the only
joint-capable recipe of the separable path: rt, s repeated until a pass lowers the cost by less than 1e-6 of it.

    timeout -k 10 900 python tools/ba_joint_time.py [--runs 3] [--out profiles/ba_joint_time.json]

One process.  The maps are tools/ba_separable_time.py's (cameras on a ring around a cube of landmarks, every second view
on a pinhole_radial_k3 intrinsic, 0.5 px pixel noise), here with the poses off by 5 cm / 0.5 degrees and the landmarks by
5 cm at once.  `call_ms` is the median of --runs host-clock times around one call on a fresh handle each time, after one
warm-up of the same shape; the call ends in a device synchronise and the read-back of the poses, so the host clock sees
all of it (creating the handle is not in it).  Nothing is asserted: the figures are recorded."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import adjust_joint_np as JN  # noqa: E402
import ba_separable_time as BT  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402


def make_map(n_views, seed):
    a = BT.make_map(n_views, 25 * n_views, 4, seed, "poses")
    rng = np.random.Generator(np.random.PCG64(seed + 1000))
    a["landmark_X"] = a["landmark_X"] + rng.normal(0.0, 0.05 / np.sqrt(3.0), a["landmark_X"].shape)
    return a


def time_joint(a, what, runs):
    times, rep = [], None
    for k in range(runs + 1):                                  # the first is the warm-up
        h = S.Sfm(**a)
        try:
            t = time.perf_counter()
            rep = h.adjust_joint(what)
            if k:
                times.append((time.perf_counter() - t) * 1e3)
        finally:
            h.close()
    return {"call_ms": statistics.median(times), "call_ms_all": times, "steps_tried": int(rep.steps_tried),
            "steps_accepted": int(rep.steps_accepted), "pcg_total": int(rep.pcg_total), "pcg_max": int(rep.pcg_max),
            "stop": int(rep.stop), "cost_initial": rep.cost_initial, "cost_final": rep.cost_final}


def time_alternation(a, runs, max_passes=20000):
    """rt, s until a pass lowers the cost by less than 1e-6 of it (max_passes only guards against a loop that never ends)"""
    times, passes, cost, converged = [], 0, 0.0, False
    for k in range(runs + 1):
        h = S.Sfm(**a)
        try:
            t = time.perf_counter()
            passes, last, converged = 0, None, False
            while passes < max_passes:
                h.adjust(3)
                cost = h.adjust(8).cost_final            # (every observation belongs to one landmark: the total cost)
                passes += 1
                if last is not None and (last - cost) <= 1e-6 * last:
                    converged = True
                    break
                last = cost
            if k:
                times.append((time.perf_counter() - t) * 1e3)
        finally:
            h.close()
    return {"call_ms": statistics.median(times), "call_ms_all": times, "passes": passes, "converged": converged,
            "cost_final": cost}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--views", type=int, nargs="*", default=[100, 1000, 10000])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_joint_time.json"))
    o = ap.parse_args()
    if S.device_count() < 1:
        raise SystemExit("ba_joint_time needs a HIP device: nothing here is a CPU figure of the product")
    out = {"runs": o.runs, "cases": []}
    for n in o.views:
        a = make_map(n, 21)
        rec = {"n_views": n, "n_landmarks": 25 * n, "n_obs": int(len(a["obs_view"])),
               "cost_initial": JN.total_cost(a, a["pose_R"], a["pose_C"], a["intrinsic"], a["landmark_X"]),
               "rst": time_joint(a, 11, o.runs), "rsti": time_joint(a, 15, o.runs),
               "alternation_rt_s": time_alternation(a, o.runs)}
        out["cases"].append(rec)
        print(json.dumps(rec), flush=True)
    with open(o.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
