"""Time sfmloc_sfm_adjust (the separable bundle adjustment) on synthetic maps: the structure command at 10^4, 10^5 and
10^6 landmarks (4 observations each, 1 000 views), the rt command at 10^2, 10^3 and 10^4 poses (100 observations each).

    timeout -k 10 900 python tools/ba_separable_time.py [--runs 3] [--out profiles/ba_separable_time.json]

One process.  Cameras on a ring around a cube of landmarks, every second view on a pinhole_radial_k3 intrinsic, 0.5 px
pixel noise, the adjusted side off by 5 cm (and 0.5 degrees).  `call_ms` is the median of --runs host-clock times around
one sfmloc_sfm_adjust call (it ends in a device synchronise and the read-back of the per-block report) on a fresh handle
each time, after one warm-up of the same shape; creating the handle (upload, transpose) is not in it.  Beside it, for
orientation only, the NumPy twin's Levenberg-Marquardt (tests/adjust_ba_np.solve_lm) on the host over a sample of
--sample blocks of the same map: `twin_ms_per_block` and its extrapolation to all blocks, `twin_s_all_blocks`.  The
sample's solutions must agree with the device's to 1e-6."""
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

import adjust_ba_np as BN  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402


def rotations(w):
    th = np.sqrt((w * w).sum(1))[:, None, None]
    K = np.zeros((len(w), 3, 3))
    K[:, 0, 1], K[:, 0, 2], K[:, 1, 0], K[:, 1, 2], K[:, 2, 0], K[:, 2, 1] = -w[:, 2], w[:, 1], w[:, 2], -w[:, 0], -w[:, 1], w[:, 0]
    return np.eye(3) + np.sin(th) / th * K + (1.0 - np.cos(th)) / (th * th) * (K @ K)


def make_map(n_views, n_lm, per_lm, seed, move):
    """-> (arrays of sfmloc_sfm_desc with the start values, the seed's generator)"""
    rng = np.random.Generator(np.random.PCG64(seed))
    ang = 2.0 * np.pi * np.arange(n_views) / n_views
    C = np.stack([10.0 * np.cos(ang), 10.0 * np.sin(ang), rng.uniform(-2.0, 2.0, n_views)], 1)
    z = -C / np.sqrt((C * C).sum(1))[:, None]
    x = np.cross(np.array([0.0, 0.0, 1.0]), z)
    x = x / np.sqrt((x * x).sum(1))[:, None]
    R = np.stack([x, np.cross(z, x), z], 1)
    X = rng.uniform(-2.0, 2.0, (n_lm, 3))
    first = rng.integers(0, n_views, n_lm)
    step = max(1, n_views // (3 * per_lm))
    obs_view = ((first[:, None] + step * np.arange(per_lm)[None, :]) % n_views).astype(np.uint32)
    obs_view.sort(1)
    obs_view = obs_view.reshape(-1)
    lm = np.repeat(np.arange(n_lm), per_lm)
    intr = np.array([[800.0, 320.0, 240.0, 0.0, 0.0, 0.0], [760.0, 331.5, 236.25, -0.08, 0.02, 0.0]])
    view_intr = (np.arange(n_views) % 2).astype(np.uint32)
    a = dict(view_id=np.arange(n_views, dtype=np.uint32), view_intrinsic=view_intr,
             view_pose=np.arange(n_views, dtype=np.uint32), intrinsic_type=np.array([0, 3], np.uint32), intrinsic=intr,
             pose_valid=np.ones(n_views, np.uint8), pose_R=R.reshape(-1, 9), pose_C=C,
             landmark_id=np.arange(n_lm, dtype=np.uint32), landmark_X=X,
             obs_off=(np.arange(n_lm + 1) * per_lm).astype(np.uint64), obs_view=obs_view,
             obs_x=np.zeros((len(obs_view), 2)))
    r, _, _ = BN.terms(a, np.arange(len(obs_view)), R[obs_view], BN.t_of(R.reshape(-1, 9), C)[obs_view], X[lm], False)
    a["obs_x"] = r + rng.normal(0.0, 0.5, r.shape)            # (obs.x was 0: r is the projection)
    if move == "structure":
        a["landmark_X"] = X + rng.normal(0.0, 0.05 / np.sqrt(3.0), X.shape)
    else:
        w = rng.normal(0.0, 1.0, (n_views, 3))
        w = w / np.sqrt((w * w).sum(1))[:, None] * np.radians(0.5)
        a["pose_R"] = (rotations(w) @ R).reshape(-1, 9)
        a["pose_C"] = C + rng.normal(0.0, 0.05 / np.sqrt(3.0), C.shape)
    return a


def time_case(a, what, runs, sample):
    times, rep, got, X = [], None, None, None
    for k in range(runs + 1):                                  # the first is the warm-up
        h = S.Sfm(**a)
        try:
            t = time.perf_counter()
            rep = h.adjust(what)
            dt = (time.perf_counter() - t) * 1e3
            if k:
                times.append(dt)
            else:
                got, X = h.read(masks=False), h.read_structure()
        finally:
            h.close()
    n_blocks = int(rep.n_blocks)
    rng = np.random.Generator(np.random.PCG64(1))
    pick = np.sort(rng.choice(len(a["landmark_id"]) if what == 8 else len(a["pose_valid"]), min(sample, n_blocks), replace=False))
    enter = BN.entering(a)
    t0 = BN.t_of(a["pose_R"], a["pose_C"])
    aa = np.array([BN.angle_axis(a["pose_R"][p]) for p in pick]) if what != 8 else None
    order = np.argsort(a["obs_view"], kind="stable")
    bounds = np.searchsorted(a["obs_view"][order], np.arange(len(a["view_id"]) + 1))
    t = time.perf_counter()
    worst = 0.0
    for i, b in enumerate(pick):
        if what == 8:
            x = BN.solve_lm(BN.structure_problem(a, int(b), enter, a["pose_R"], t0, a["landmark_X"]))[0]
            worst = max(worst, float(np.abs(x - X[b]).max()))
        else:
            x = BN.solve_lm(BN.pose_problem(a, int(b), what, enter, {int(b): aa[i]}, t0, a["landmark_X"],
                                            idx=order[bounds[b]:bounds[b + 1]]))[0]
            R = got["pose_R"][b]
            worst = max(worst, float(np.abs(BN.rodrigues(x[:3]) - R).max()),
                        float(np.abs(BN.c_of(R.reshape(1, 9), x[3:])[0] - got["pose_C"][b]).max()))
    twin = time.perf_counter() - t
    assert worst < 1e-6, f"the twin's sample disagrees with the device by {worst}"
    return {"n_blocks": n_blocks, "n_obs": int(len(a["obs_view"])), "call_ms": statistics.median(times), "call_ms_all": times,
            "max_iterations": int(rep.max_iterations), "n_at_cap": int(rep.n_at_cap), "cost_initial": rep.cost_initial,
            "cost_final": rep.cost_final, "twin_sample": int(len(pick)), "twin_ms_per_block": twin * 1e3 / len(pick),
            "twin_s_all_blocks": twin / len(pick) * n_blocks, "sample_distance": worst}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--sample", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ba_separable_time.json"))
    a = ap.parse_args()
    if S.device_count() < 1:
        raise SystemExit("ba_separable_time needs a HIP device: nothing here is a CPU figure of the product")
    out = {"runs": a.runs, "structure": [], "rt": []}
    for n in (10000, 100000, 1000000):
        rec = {"n_landmarks": n, "n_views": 1000, **time_case(make_map(1000, n, 4, 11, "structure"), 8, a.runs, a.sample)}
        out["structure"].append(rec)
        print(json.dumps(rec), flush=True)
    for n in (100, 1000, 10000):
        rec = {"n_poses": n, "n_landmarks": 25 * n, **time_case(make_map(n, 25 * n, 4, 12, "poses"), 3, a.runs, a.sample)}
        out["rt"].append(rec)
        print(json.dumps(rec), flush=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
