"""Times sfmloc_bow_knn at the benchmark map's size and writes profiles/bowpairs_time.json: n = 10 000 views, dim = 500,
k = 20 and 100, window 0, seeded uniform vectors.  Per k: the device milliseconds of the call (sfmloc_bowknn_last_ms:
the passes' kernels and the copies of their results), the wall time of the call (upload, finite check and result
copies included), and the wall time of the only way to the same lists without it: Map.bow_select once per view on
the same matrix (k + 1 nearest of all views, the view itself among them).  Every repeat is recorded after a warm-up
call.  No threshold is set: the record is the deliverable.

The share of the f32 VALU issue floor: the distance kernel subtracts and multiply-adds once per element of every
(query row, bank row) pair, n^2 * dim elements.  At MI355X_MICROARCH's rate (a wave64 VALU instruction issues in 2 cycles
on a SIMD; 4 SIMDs x 256 CUs x 2.4 GHz) two instructions per element are the floor the issue of this work names; the
library is built unfused (-ffp-contract=off, the oracle's arithmetic), so the kernel issues three (subtract, multiply,
add), and that floor is recorded too.  device_ms over either is a whole call's share, not the kernel's alone.

    python tools/bowpairs_time.py [--n 10000] [--dim 500] [--repeats 5] [--out profiles/bowpairs_time.json]
                                  [--commit LABEL] [--device-name LABEL]
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

import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

WAVE_INSTRUCTIONS_PER_SECOND = 256 * 4 * 2.4e9 / 2        # CUs x SIMDs x clock / (2 cycles per wave64 VALU instruction)


def floor_ms(n, dim, issues_per_element):
    return 1000.0 * (float(n) * n * dim / 64.0) * issues_per_element / WAVE_INSTRUCTIONS_PER_SECOND


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10000)
    ap.add_argument("--dim", type=int, default=500)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bowpairs_time.json"))
    ap.add_argument("--commit", default=None, help="the commit measured (default: git rev-parse HEAD)")
    ap.add_argument("--device-name", default="HIP device 0", help="the record's device label, written as given")
    a = ap.parse_args()
    if capi.device_count() < 1:
        raise SystemExit("bowpairs_time.py needs a HIP device: a time taken without one says nothing")
    import bow_cases
    commit = a.commit or subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    n, dim = a.n, a.dim
    bow = np.random.Generator(np.random.PCG64(2024)).random((n, dim), np.float32)
    view_id, view_off, desc = bow_cases.map_arrays(n)
    rows = []
    with S.Map(view_id, view_off, desc, bow=bow) as dm:
        for k in (20, 100):
            nbr, dist, count = capi.bow_knn(bow, k, profile=True)              # (the first call pays the code object's load)
            ms, wall = [], []
            for _ in range(a.repeats):
                t0 = time.perf_counter()
                nbr, dist, count = capi.bow_knn(bow, k, profile=True)
                wall.append(time.perf_counter() - t0)
                ms.append(capi.bowknn_last_ms())
            for i in range(0, n, max(1, n // 8)):                              # warm-up of the per-view way, and a check
                sel = dm.bow_select(bow[i], k + 1)
                assert sel[sel != i].tolist() == nbr[i].tolist(), f"row {i} differs from bow_select"
            loop = []
            for _ in range(max(1, a.repeats // 2)):
                t0 = time.perf_counter()
                for i in range(n):
                    dm.bow_select(bow[i], k + 1)
                loop.append(time.perf_counter() - t0)
            rows.append({"n": n, "dim": dim, "k": k, "window": 0,
                         "bow_knn_device_ms": {"all": ms, "best": min(ms)},
                         "bow_knn_wall_s": {"all": wall, "best": min(wall)},
                         "bow_select_per_view_wall_s": {"all": loop, "best": min(loop)},
                         "wall_ratio_per_view_over_bow_knn": min(loop) / min(wall),
                         "valu_floor_ms_2_issues_per_element": floor_ms(n, dim, 2),
                         "valu_floor_ms_3_issues_per_element_unfused": floor_ms(n, dim, 3),
                         "device_ms_share_of_2_issue_floor": floor_ms(n, dim, 2) / min(ms),
                         "device_ms_share_of_3_issue_floor": floor_ms(n, dim, 3) / min(ms),
                         "rows_checked_against_bow_select": len(range(0, n, max(1, n // 8)))})
    doc = {"commit": commit, "device": a.device_name, "rows": rows,
           "wave64_valu_instructions_per_second": WAVE_INSTRUCTIONS_PER_SECOND,
           "note": "bow_knn_device_ms is between two events around the passes: the distance and selection kernels of every "
                   "pass and the copies of its results to the host; the shares are that whole figure's, not the distance "
                   "kernel's alone.  bow_select_per_view asks for k + 1 of all views (the view itself is among them)."}
    with open(a.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
