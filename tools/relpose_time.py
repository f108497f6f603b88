"""Device time of sfmloc_relative_poses on the synthetic corridor of tools/structure_time.py (10 000 views by default):
device ms from sfmloc_relpose_last_ms, pairs/s, the rounds (of the restatement's subset, which carries the device's bits:
the C record has no rounds field) and the pairs that end ok, written to profiles/relpose_time.json.  OpenMVG
was not run and the reference has no number for this stage; the NumPy figure beside it is the restatement
(tests/relpose_np.py) on a 1 % subset of the pairs, not a competing implementation.

    python tools/relpose_time.py [--views 10000] [--repeats 3] [--out profiles/relpose_time.json]
                                 [--refine [--parity-out profiles/relrefine_parity.json]]

--refine: sfmloc_refine_relative_poses runs on the ok pairs of the same run; the record (then profiles/relrefine_time.json
by default) gains "refine": its device ms beside the relative poses', the steps per pair, the count per status, and the
restatement (tests/relrefine_np.py) on the same subset.  --parity-out: the rotation errors against the corridor's
planted poses per pair and after sfmloc_global_poses, without and with the refinement.
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


def refine_record(a, args, r, sel):
    """--refine: sfmloc_refine_relative_poses on the ok pairs of the relative poses r (the run whose device_ms stands
    beside it), a.repeats times; the restatement on the subset sel.  "_results" is for parity_record, not for the file."""
    import relrefine_np as rtw
    call = {k: v for k, v in args.items() if k != "view_wh"}
    call.update(rel_R=r.results["R"], rel_t=r.results["t"], inl_off=r.inl_off, inl_idx=r.inl_idx, use_pair=r.results["ok"])
    ms, wall = [], []
    for _ in range(a.repeats):
        t0 = time.perf_counter()
        f = capi.RelRefine(**call)
        wall.append(time.perf_counter() - t0)
        ms.append(f.ms)
    res = f.results
    ran = res["status"] != 0
    steps = res["steps"][ran & (res["status"] != 2)]
    moved = np.isin(res["status"], (1, 3)) & (res["cost_initial"] > 0.0)
    ioff, off = r.inl_off.astype(np.int64), args["offsets"].astype(np.int64)
    per = np.diff(off)
    sub = dict(call, pairs=args["pairs"][sel], offsets=np.concatenate([[0], np.cumsum(per[sel])]).astype(np.uint64),
               match_i=np.concatenate([args["match_i"][off[k]:off[k + 1]] for k in sel]),
               match_j=np.concatenate([args["match_j"][off[k]:off[k + 1]] for k in sel]),
               rel_R=call["rel_R"][sel], rel_t=call["rel_t"][sel], use_pair=call["use_pair"][sel],
               inl_off=np.concatenate([[0], np.cumsum(np.diff(ioff)[sel])]).astype(np.uint64),
               inl_idx=np.concatenate([r.inl_idx[ioff[k]:ioff[k + 1]] for k in sel]))
    t0 = time.perf_counter()
    twin = rtw.refine_relative_poses(**sub)
    t_np = time.perf_counter() - t0
    same = all(int(x["status"]) == int(res[k]["status"]) and int(x["steps"]) == int(res[k]["steps"]) and
               int(x["n_used"]) == int(res[k]["n_used"]) and
               all(np.array_equal(np.asarray(x[n], np.float64).reshape(-1).view(np.uint64),
                                  np.ascontiguousarray(res[k][n]).reshape(-1).view(np.uint64))
                   for n in ("R", "t", "E", "cost_initial", "cost")) for x, k in zip(twin, sel))
    return {"what": "sfmloc_refine_relative_poses on the ok pairs of the last sfmloc_relative_poses above; device_ms = "
                    "sfmloc_relrefine_last_ms (HIP events around the call's kernel and copies)",
            "device_ms": {"all": ms, "best": min(ms)}, "call_s": {"all": wall, "best": min(wall)},
            "relative_poses_device_ms": r.ms, "pairs_asked": int(ran.sum()), "inliers": int(r.inl_off[-1]),
            "pairs_per_s_device": int(ran.sum()) / (min(ms) * 1e-3),
            "status_count": {str(s): int((res["status"] == s).sum()) for s in range(5)},
            "steps_per_pair": ({"min": int(steps.min()), "median": float(np.median(steps)), "max": int(steps.max())}
                               if len(steps) else None),
            "cost_ratio_median": float(np.median(res["cost"][moved] / res["cost_initial"][moved])) if moved.any() else None,
            "numpy_restatement": {"pairs": int(len(sel)), "seconds": t_np, "same_bits_as_device": bool(same)},
            "_results": res}


def parity_record(rec, n_views, pairs, r, fine):
    """the corridor's planted poses are R = I for every view, so a pair's rotation error is the angle of its rel_R, and a
    view's after sfmloc_global_poses the angle of its R in the root's gauge"""
    import globalposes_np as gtw
    ok = r.results["ok"] != 0
    took = np.isin(fine["status"], (1, 3))
    eye = np.tile(np.eye(3), (int(ok.sum()), 1, 1))
    out = {"what": "rotation errors in degrees against the planted poses of the corridor of tools/structure_time.py (R = "
                   "I in every view), over the ok pairs, without and with sfmloc_refine_relative_poses; drift = the "
                   "largest rotation error of a view after sfmloc_global_poses on those pairs",
           "commit": rec["commit"], "views": int(n_views), "pairs_ok": int(ok.sum()), "pairs_refined": int(took.sum())}
    for name, R, t in (("sample", r.results["R"], r.results["t"]),
                       ("refined", np.where(took[:, None], fine["R"], r.results["R"]),
                        np.where(took[:, None], fine["t"], r.results["t"]))):
        e = gtw.rotation_error_deg(R[ok].reshape(-1, 3, 3), eye)
        tdir = np.degrees(np.arccos(np.clip(-t[ok][:, 0], -1.0, 1.0)))          # planted direction: (-1, 0, 0)
        g = capi.GlobalPoses(n_views, pairs[ok], R[ok].reshape(-1, 3, 3), t[ok], None)
        v = np.nonzero(g.in_component)[0]
        drift = gtw.rotation_error_deg(g.R[v] @ g.R[int(g.report.root)].T, np.tile(np.eye(3), (len(v), 1, 1)))
        out[name] = {"pair_rotation_error_deg": {"median": float(np.median(e)), "max": float(e.max())},
                     "pair_direction_error_deg": {"median": float(np.median(tdir)), "max": float(tdir.max())},
                     "views_in_component": int(len(v)), "rotation_drift_deg": float(drift.max()),
                     "global_poses_device_ms": float(g.ms)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--numpy-pairs", type=int, default=0, help="pairs of the restatement's subset (default: 1 %%, at most 50)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None)
    ap.add_argument("--refine", action="store_true", help="time sfmloc_refine_relative_poses on the same run's ok pairs too")
    ap.add_argument("--parity-out", default=None, help="with --refine: the rotation errors against the planted poses, per "
                                                       "pair and after sfmloc_global_poses, with and without the refinement")
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, "profiles", "relrefine_time.json" if a.refine else "relpose_time.json")
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
    if a.refine:
        rec["refine"] = refine_record(a, args, r, sel)
        if a.parity_out:
            with open(a.parity_out, "w") as fh:
                json.dump(parity_record(rec, n_views, pairs, r, rec["refine"].pop("_results")), fh, indent=1)
                fh.write("\n")
        rec["refine"].pop("_results", None)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
