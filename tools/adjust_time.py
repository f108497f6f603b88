"""Time the OpenMVG_BA twin on a large map: 10 000 views x about 250 observations (synthdata.make_map).

    python tools/adjust_time.py [--views 10000] [--obs 250] [--cpu-views 400] [--out profiles/adjust_time.json]

Records the device resection rate (views/s), the cleanup time, the whole tool's wall time split into JSON I/O and device
work (bin/OpenMVG_BA's stages timed from Python: json load + array build, create + resect + clean, the two json.dump),
and the CPU restatement on the same inputs and box: oracle_c.p3p_localize over 16 threads (on --cpu-views views,
scaled) plus adjust_np's cleanup.  No speedup is promised; the numbers are what they are."""
import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adjust_np as AN  # noqa: E402
import adjust_scene as AS  # noqa: E402
import synthdata  # noqa: E402
from sfmlocalization_amd import adjust  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402


def big_doc(n_views, obs):
    m = synthdata.make_map(7, n_views=n_views, desc_per_view=obs + 10, views_per_place=20, landmarks_per_place=600,
                           obs_per_view=obs, kpt_noise=0.3)
    slot_view = np.searchsorted(m.view_off, np.arange(m.n_rows), side="right") - 1
    rows = np.nonzero(m.row_landmark >= 0)[0]
    order = np.lexsort((slot_view[rows], m.row_landmark[rows]))
    rows = rows[order]
    f, ppx, ppy = m.intrinsic
    views = [{"key": int(v), "value": {"polymorphic_id": 1073741824 if k else 2147483649, "ptr_wrapper": {
        "id": 2147483649 + k, "data": {"local_path": "/", "filename": f"img{k:06d}.jpg", "width": 640, "height": 480,
                                       "id_view": int(v), "id_intrinsic": 0, "id_pose": int(v)}}}}
             for k, v in enumerate(m.view_id)]
    views[0]["value"]["polymorphic_name"] = "view"
    intr = [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole", "ptr_wrapper": {
        "id": 2147483649 + n_views, "data": {"width": 640, "height": 480, "focal_length": float(f),
                                             "principal_point": [float(ppx), float(ppy)]}}}}]
    ext = [{"key": int(v), "value": {"rotation": m.view_R[k].tolist(), "center": m.view_C[k].tolist()}}
           for k, v in enumerate(m.view_id)]
    st = []
    lm = m.row_landmark[rows]
    bounds = np.searchsorted(lm, np.arange(len(m.landmark_id) + 1))
    for s in range(len(m.landmark_id)):
        rr = rows[bounds[s]:bounds[s + 1]]
        if len(rr) == 0:
            continue
        st.append({"key": int(m.landmark_id[s]), "value": {"X": [float(x) for x in m.landmark_X[s]], "observations": [
            {"key": int(m.view_id[slot_view[r]]), "value": {"id_feat": int(r - m.view_off[slot_view[r]]),
                                                            "x": [float(m.kpt_xy[r, 0]), float(m.kpt_xy[r, 1])]}}
            for r in rr]}})
    return {"sfm_data_version": "0.3", "root_path": "/data", "views": views, "intrinsics": intr, "extrinsics": ext,
            "structure": st, "control_points": []}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=10000)
    ap.add_argument("--obs", type=int, default=250)
    ap.add_argument("--cpu-views", type=int, default=400)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adjust_time.json"))
    ap.add_argument("--workdir", default="/tmp/adjust_time")
    args = ap.parse_args()
    os.makedirs(args.workdir, exist_ok=True)
    t0 = time.perf_counter()
    doc = big_doc(args.views, args.obs)
    src = os.path.join(args.workdir, "sfm_data.json")
    with open(src, "w") as fh:
        json.dump(doc, fh)
    t_gen = time.perf_counter() - t0
    print(f"generated {args.views} views in {t_gen:.1f} s", flush=True)
    # the tool's stages as adjust.run performs them
    t = time.perf_counter()
    with open(src) as fh:
        d2 = json.load(fh)
    a, pose_id, pose_src = adjust.sfm_arrays(d2)
    t_load = time.perf_counter() - t
    t = time.perf_counter()
    h = S.Sfm(**a)
    t_create = time.perf_counter() - t
    t = time.perf_counter()
    ran, ok = h.resect()
    t_resect = time.perf_counter() - t
    t = time.perf_counter()
    counts = h.clean(4.0, 2.0, True)
    t_clean = time.perf_counter() - t
    t = time.perf_counter()
    h.read()
    h.close()
    t_read = time.perf_counter() - t
    print(f"device: resect {t_resect:.3f} s, cleanup {t_clean:.3f} s", flush=True)
    # the whole program, twice (C++ and Python), wall clock
    import subprocess
    walls = {}
    for name, prog in (("cpp", [os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVG_BA")]),
                       ("py", [sys.executable, "-m", "sfmlocalization_amd.adjust"])):
        t = time.perf_counter()
        r = subprocess.run(prog + [src, os.path.join(args.workdir, f"out_{name}.json"), "-r=1"], cwd=ROOT,
                           capture_output=True, text=True)
        walls[name] = time.perf_counter() - t
        print(f"{name} tool {walls[name]:.1f} s", flush=True)
        assert r.returncode == 0, r.stderr
    t = time.perf_counter()
    with open(os.path.join(args.workdir, "out_py.json")) as fh:
        out = json.load(fh)
    with open(os.path.join(args.workdir, "dump.json"), "w") as fh:
        json.dump(out, fh)
    t_dump = time.perf_counter() - t
    # CPU restatement on the same inputs: the oracle's P3P over 16 threads on a sample of views, scaled, + adjust_np
    from oracle import oracle_c
    oracle_c.build()
    lists = AS.view_lists(a)
    obs_lm = np.repeat(np.arange(len(a["landmark_id"])), np.diff(a["obs_off"].astype(np.int64)))
    K = a["intrinsic"][0]
    sample = [k for k in range(0, len(lists), max(1, len(lists) // args.cpu_views)) if len(lists[k]) > 10][:args.cpu_views]

    def one(k):
        idx = lists[k]
        return oracle_c.p3p_localize(a["obs_x"][idx], a["landmark_X"][obs_lm[idx]], K[0], K[1], K[2], 4096, AS.SEED,
                                     stream=int(a["view_id"][k]))["n"]
    t = time.perf_counter()
    with ThreadPoolExecutor(16) as ex:
        list(ex.map(one, sample))
    t_cpu_sample = time.perf_counter() - t
    t = time.perf_counter()
    AN.clean(a, a["pose_valid"], a["pose_R"], a["pose_C"], rm_unstable=True)
    t_cpu_clean = time.perf_counter() - t
    rec = {
        "map": {"views": int(len(a["view_id"])), "observations": int(len(a["obs_view"])),
                "landmarks": int(len(a["landmark_id"])), "json_bytes": os.path.getsize(src)},
        "device": {"views_resected": ran, "views_ok": ok, "create_s": t_create, "resect_s": t_resect,
                   "resect_views_per_s": ran / t_resect if t_resect > 0 else None, "cleanup_s": t_clean,
                   "read_s": t_read, "counts": counts},
        "tool_wall_s": {"cpp": walls["cpp"], "py": walls["py"]},
        "py_split_s": {"json_load_and_arrays": t_load, "device_work": t_create + t_resect + t_clean + t_read,
                       "json_reload_and_dump_output": t_dump},
        "cpu_restatement": {"p3p_threads": 16, "p3p_sample_views": len(sample), "p3p_sample_s": t_cpu_sample,
                            "p3p_views_per_s": len(sample) / t_cpu_sample if t_cpu_sample > 0 else None,
                            "p3p_all_views_est_s": t_cpu_sample * ran / max(1, len(sample)),
                            "adjust_np_cleanup_s": t_cpu_clean},
        "generate_s": t_gen,
    }
    print(json.dumps(rec, indent=1))
    with open(args.out, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
