"""Writes tests/golden/relrefine/expected.json: what the independent two-view refinement
(tests/relrefine_independent.py, SciPy's least_squares) reaches on the relative-pose scene, for the cost comparison of
tests/test_relrefine_cpu.py.  Run from the repository root on the CPU: python tests/golden/make_relrefine_fixtures.py

Per pair that ends ok under tests/relpose_np.py, from that restatement's pose and inlier list (the inputs the device
call gets) and the bearings of relpose_np.bearings:
    ref_cost          the reference's final cost at tolerances 1e-14 (ftol = xtol = gtol)
    ref_cost_initial  its cost at the start: the cost of the sample's pose with SVD-triangulated points
    ref_dR, ref_dt    the max-norm distance of its pose to the planted one; sample_dR, sample_dt the sample's
    repro             the reference's own reproducibility: |cost(1e-12) - cost(1e-15)| / cost(1e-14), two more runs
    margin            max(10 x repro, 1e-12): both the reference and the device stop on a relative-decrease rule and
                      neither reaches the exact minimum, so the comparison allows the reference's own spread, ten-fold,
                      and never less than 1e-12.  Measured on the reference alone; nothing here runs the code under test.
    n_used, nfev      for the record
Data only."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

import relpose_np as relpose_twin  # noqa: E402
import relpose_scene as scene_mod  # noqa: E402
import relrefine_independent as ind  # noqa: E402

MARGIN_FLOOR = 1e-12


def pair_inputs(scene, args, k, r):
    """-> (R0 [3, 3], t0 [3], b [n, 4], f_I, f_J) of pair k under the restatement's result r"""
    vi, vj = (int(v) for v in args["pairs"][k])
    off = np.asarray(scene["view_off"], np.int64)
    pos = int(args["offsets"][k]) + np.asarray(r["inliers"], np.int64)
    ii, ij = int(args["view_intrinsic"][vi]), int(args["view_intrinsic"][vj])
    K = np.asarray(args["intrinsics"], np.float64).reshape(-1, 6)
    bi = relpose_twin.bearings(args["kpt_xy"][off[vi] + args["match_i"][pos].astype(np.int64)], K[ii], args["intrinsic_type"][ii])
    bj = relpose_twin.bearings(args["kpt_xy"][off[vj] + args["match_j"][pos].astype(np.int64)], K[ij], args["intrinsic_type"][ij])
    return np.asarray(r["R"]).reshape(3, 3), np.asarray(r["t"]).reshape(3), np.concatenate([bi, bj], 1), K[ii, 0], K[ij, 0]


def main():
    scene = scene_mod.make_scene()
    args, names = scene_mod.call_arrays(scene)
    res = relpose_twin.relative_poses(**args)
    out = {}
    for k, (name, r) in enumerate(zip(names, res)):
        if not r["ok"]:
            continue
        R0, t0, b, fi, fj = pair_inputs(scene, args, k, r)
        Rp, tp = scene_mod.planted_pose(scene, int(args["pairs"][k][0]), int(args["pairs"][k][1]))
        ref = ind.refine(R0, t0, b, fi, fj, tol=1e-14)
        lo, hi = ind.refine(R0, t0, b, fi, fj, tol=1e-12), ind.refine(R0, t0, b, fi, fj, tol=1e-15)
        repro = abs(lo["cost"] - hi["cost"]) / ref["cost"]
        out[name] = {"ref_cost": ref["cost"], "ref_cost_initial": ref["cost_initial"],
                     "ref_dR": float(np.abs(ref["R"] - Rp).max()), "ref_dt": float(np.abs(ref["t"] - tp).max()),
                     "sample_dR": float(np.abs(R0 - Rp).max()), "sample_dt": float(np.abs(t0 - tp).max()),
                     "repro": repro, "margin": max(10.0 * repro, MARGIN_FLOOR), "n_used": ref["n_used"],
                     "nfev": [lo["nfev"], ref["nfev"], hi["nfev"]], "scipy_status": ref["status"]}
        print(name, json.dumps(out[name]), flush=True)
    os.makedirs(os.path.join(HERE, "relrefine"), exist_ok=True)
    with open(os.path.join(HERE, "relrefine", "expected.json"), "w") as fh:
        json.dump({"margin_floor": MARGIN_FLOOR, "pairs": out}, fh, indent=1)


if __name__ == "__main__":
    main()
