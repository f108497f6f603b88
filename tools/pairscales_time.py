"""Times sfmloc_wedge_scales on the corridor of tools/globalposes_time.py with planted depths and writes
profiles/pairscales_time.json: device milliseconds of the wedge stage, its launches, candidates, records and depths, every
repeat recorded after a warm-up call, the error of the ratios against the planted baselines -- and beside them the
figures of sfmloc_global_poses' translation stage on the same pair graph in the same run, which does not read the
ratios, and of sfmloc_global_poses_scaled, which does: its scale and centre phases in device milliseconds, launches, PCG
iterations and both calls' centre errors.  No threshold is set: the record is the deliverable.

    python tools/pairscales_time.py [--views 10000] [--repeats 3] [--out profiles/pairscales_time.json]
                                    [--commit LABEL] [--device-name LABEL]

The two labels are written as given; a commit label that ends in "+" is that commit with the change that adds this
tool on top, as in tools/globalposes_time.py.

The corridor: cameras 0.5 m apart on a line, all looking the same way, every view paired with its next 5 neighbours, the
relative poses the planted ones with 0.2 degrees of rotation noise and 0.005 rad of direction noise
(globalposes_time.corridor_poses).  The depths: 20 points per camera step, 4 to 9 m in front of the line; a view has a
feature for each point within 5 steps of it (200 features), 0.3 px of noise at f = 800; a pair matches the points both
views see (100 to 180), and every match is an inlier."""
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

from globalposes_time import NEIGHBOURS, corridor_poses  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

PER_BLOCK, REACH = 20, 5            # points per camera step; a view sees the blocks of the steps v - 5 .. v + 4
F, PPX, PPY, NOISE_PX = 800.0, 640.0, 480.0, 0.3


def corridor_depths(s, seed=12):
    """the arguments of capi.WedgeScales for the scene of corridor_poses"""
    rng = np.random.default_rng(seed)
    n = s["n_views"]
    nb = n + 2 * REACH
    bx = 0.5 * (np.arange(nb) - REACH)                                       # block b lies in front of step b - REACH
    X = np.stack([bx[:, None] + rng.uniform(0.0, 0.5, (nb, PER_BLOCK)), rng.uniform(-1.5, 1.5, (nb, PER_BLOCK)),
                  rng.uniform(4.0, 9.0, (nb, PER_BLOCK))], 2)                # [block, point, 3]
    blocks = np.arange(n)[:, None] + np.arange(2 * REACH)[None, :]            # view v sees the blocks v .. v + 9
    Xc = X[blocks] - s["C_true"][:, None, None, :]                            # (every rotation is the identity)
    px = F * Xc[..., :2] / Xc[..., 2:] + np.array([PPX, PPY]) + rng.normal(size=Xc[..., :2].shape) * NOISE_PX
    per_view = 2 * REACH * PER_BLOCK
    pairs = s["pairs"].astype(np.int64)
    d = pairs[:, 1] - pairs[:, 0]
    mi, mj, counts = [], [], (2 * REACH - d) * PER_BLOCK
    for k in range(len(pairs)):                                               # the blocks v + d .. v + 9 of view v
        m = np.arange(counts[k])
        mi.append(m + d[k] * PER_BLOCK)
        mj.append(m)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    inl = np.concatenate([np.arange(c) for c in counts]).astype(np.uint32)
    return dict(view_off=(per_view * np.arange(n + 1)).astype(np.uint64), kpt_xy=px.reshape(-1, 2).astype(np.float32),
                view_intrinsic=np.zeros(n, np.uint32), intrinsics=np.array([[F, PPX, PPY, 0.0, 0.0, 0.0]]),
                intrinsic_type=np.zeros(1, np.uint32), pairs=s["pairs"], offsets=offsets,
                match_i=np.concatenate(mi).astype(np.uint32), match_j=np.concatenate(mj).astype(np.uint32),
                rel_R=s["rel_R"], rel_t=s["rel_t"], inl_off=offsets, inl_idx=inl)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pairscales_time.json"))
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    ap.add_argument("--device-name", default="HIP device 0", help="the record's device label, written as given")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("pairscales_time.py needs a HIP device: a time taken without one says nothing")
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    s = corridor_poses(a.views)
    call = corridor_depths(s)
    b = 0.5 * (s["pairs"][:, 1].astype(np.float64) - s["pairs"][:, 0])
    capi.WedgeScales(**call)                                                # (the first call pays the code object's load)
    runs = []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        w = capi.WedgeScales(**call)
        row = {k: getattr(w.report, k) for k, _ in capi.WscalesReport._fields_ if k != "reserved"}
        row["wall_s"] = time.perf_counter() - t0
        err = np.abs(np.log(w.records["ratio"] * b[w.records["k"]] / b[w.records["l"]]))
        row["ratio_log_error"] = {"median": float(np.median(err)), "p99": float(np.quantile(err, 0.99)), "max": float(err.max())}
        runs.append(row)
    g = capi.GlobalPoses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"])
    unscaled = {k: getattr(g.report, k) for k in ("n_translation_pairs", "trans_steps_tried", "trans_steps_accepted",
                                                  "trans_pcg_total", "trans_stop", "translation_ms", "launches", "device_ms")}
    import globalposes_scene as gs
    h = capi.GlobalPoses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"], wedges=w.records)
    scaled = {k: getattr(h.report, k) for k in unscaled}
    scaled["scale"] = {k: getattr(h.scale_report, k) for k, _ in capi.GpscaleReport._fields_}
    for row, x in ((unscaled, g), (scaled, h)):
        row["centre_error"] = gs.errors(s, x.in_component, int(g.report.root), x.R, x.C)[1] if x.in_component.any() else None
        row["n_component_views"] = int(x.in_component.sum())
    doc = {"commit": commit, "device": a.device_name, "views": a.views, "pairs": int(len(s["pairs"])),
           "matches": int(len(call["match_i"])), "neighbours": NEIGHBOURS, "runs": runs, "global_poses_same_run": unscaled,
           "global_poses_scaled_same_run": scaled,
           "note": "sfmloc_global_poses does not read the ratios; sfmloc_global_poses_scaled on the same arrays with the "
                   "last run's records is beside it: scale.scale_ms and translation_ms (= scale.centre_ms) are its two "
                   "phases, scale.pcg_total and trans_pcg_total their iterations"}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps({k: doc[k] for k in ("views", "pairs", "matches")}), json.dumps(runs[-1]), json.dumps(unscaled),
          json.dumps(scaled))


if __name__ == "__main__":
    main()
