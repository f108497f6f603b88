"""Times the landmark colouring on a synthetic map and writes profiles/colorize_time.json: the plan's device time
(sfmloc_sfm_color_last_ms) and the wall time of the whole tool (python -m sfmlocalization_amd.colorize: JSON in, plan,
images, PLY out) on 10 000 views and 2 M landmarks, and beside them the NumPy restatement (tests/colorize_np.py, the
loop that recounts every view in every iteration) on the largest of a ladder of sizes it finishes in about a minute.

    python tools/colorize_time.py [--views 10000] [--landmarks 2000000] [--out profiles/colorize_time.json]

The map: views on a line, every landmark seen by 2..8 views out of a window of 40 neighbours (so the cover needs many
iterations, as a walked corridor does); 64 distinct 64 x 48 PPM images shared by the views.  The tool's wall time
includes Python's json.load of the document, which is reported on its own."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import colorize_np as CN  # noqa: E402
import colorize_scene as CS  # noqa: E402
from sfmlocalization_amd import capi, colorize  # noqa: E402


def structure(seed, n_views, n_lm, window=40):
    rng = np.random.Generator(np.random.PCG64(seed))
    k = rng.integers(2, 9, n_lm)
    base = rng.integers(0, max(1, n_views - window), n_lm)
    off = np.concatenate([[0], np.cumsum(k)]).astype(np.uint64)
    view = np.empty(int(off[-1]), np.uint32)
    step = window // 8
    for j in range(8):                       # observation j of a landmark: a view in the j-th slice of its window
        sel = np.flatnonzero(k > j)
        view[off[sel].astype(np.int64) + j] = np.minimum(base[sel] + j * step + rng.integers(0, step, len(sel)), n_views - 1)
    return off, view


def arrays_of(n_views, off, view, seed=1):
    a = CS.sfm_arrays(n_views, [], seed)
    rng = np.random.Generator(np.random.PCG64(seed))
    n_lm = len(off) - 1
    a.update(landmark_id=np.arange(n_lm, dtype=np.uint32), landmark_X=rng.uniform(-50, 50, (n_lm, 3)), obs_off=off,
             obs_view=view, obs_x=rng.uniform(0, 1, (len(view), 2)) * [CS.W - 1, CS.H - 1])
    return a


def write_project(folder, a, n_images=64):
    rng = np.random.Generator(np.random.PCG64(9))
    for k in range(n_images):
        CS.write_ppm(os.path.join(folder, f"i{k:02d}.ppm"), rng.integers(0, 256, (CS.H, CS.W, 3), dtype=np.uint8))
    n_views = len(a["view_id"])
    off, view, x = a["obs_off"].astype(np.int64), a["obs_view"], a["obs_x"]
    lms = [(a["landmark_X"][l], [(int(view[o]), x[o, 0], x[o, 1]) for o in range(off[l], off[l + 1])])
           for l in range(len(off) - 1)]
    doc = CS.document(folder, [f"i{k % n_images:02d}.ppm" for k in range(n_views)], [(CS.W, CS.H)] * n_views,
                      {k: a["pose_C"][k] for k in range(n_views)}, lms)
    path = os.path.join(folder, "sfm_data.json")
    with open(path, "w") as fh:
        json.dump(doc, fh)
    return path


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--landmarks", type=int, default=2000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "colorize_time.json"))
    ap.add_argument("--numpy-budget", type=float, default=60.0)
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    a = ap.parse_args()
    off, view = structure(1, a.views, a.landmarks)
    arrays = arrays_of(a.views, off, view)
    t0 = time.perf_counter()
    h = capi.Sfm(**arrays)
    t_create = time.perf_counter() - t0
    plans = []
    for _ in range(3):                       # the first call pays the code object's load
        t0 = time.perf_counter()
        order, it, ob = h.color_plan()
        plans.append({"device_ms": capi.sfm_color_last_ms(), "wall_ms": (time.perf_counter() - t0) * 1e3})
    h.close()
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    print("plan:", plans, flush=True)
    out = {"commit": commit,
           "map": {"views": a.views, "landmarks": a.landmarks, "observations": int(off[-1]), "iterations": int(len(order))},
           "sfm_create_s": t_create, "plan_calls": plans}
    with tempfile.TemporaryDirectory() as td:
        t0 = time.perf_counter()
        sfm = write_project(td, arrays)
        out["write_project_s"] = time.perf_counter() - t0
        print("project written", flush=True)
        t0 = time.perf_counter()
        with open(sfm) as fh:
            json.load(fh)
        out["json_load_s"] = time.perf_counter() - t0
        print("document loaded once", flush=True)
        t0 = time.perf_counter()
        rc = colorize.main(["-i", sfm, "-o", os.path.join(td, "colorized.ply")])
        out["tool_wall_s"] = time.perf_counter() - t0
        out["tool_status"] = rc
        out["ply_bytes"] = os.path.getsize(os.path.join(td, "colorized.ply")) if rc == 0 else 0
    ladder = []
    for n_views, n_lm in ((100, 20000), (300, 60000), (1000, 200000), (2000, 400000), (4000, 800000), (10000, 2000000)):
        o, v = structure(1, n_views, n_lm)
        t0 = time.perf_counter()
        e_order, e_it, e_ob = CN.plan(n_views, o, v)
        dt = time.perf_counter() - t0
        hh = capi.Sfm(**arrays_of(n_views, o, v))
        d_order, d_it, d_ob = hh.color_plan()
        hh.close()
        ladder.append({"views": n_views, "landmarks": n_lm, "observations": int(o[-1]), "iterations": int(len(e_order)),
                       "numpy_s": dt, "device_ms": capi.sfm_color_last_ms(),
                       "equal": bool(np.array_equal(e_order, d_order) and np.array_equal(e_it, d_it)
                                     and np.array_equal(e_ob, d_ob))})
        print(ladder[-1], flush=True)
        if dt * 4 > a.numpy_budget:          # the next size is ~2.5-5x the work
            break
    out["numpy_restatement"] = ladder
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps({k: v for k, v in out.items() if k != "numpy_restatement"}))


if __name__ == "__main__":
    main()
