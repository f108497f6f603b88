#!/usr/bin/env python3
"""The matrix-core view-list scan against the popcount form on M-LDB-like descriptors (synthdata.mldb_like_bank: the
statistics of extracted descriptors, where the matrix-core form's untightened threshold flags several times the rows)
and on a uniform bank of the same size: time of the Hamming stage (scan + exact pass over the flagged rows, HIP events)
and rows flagged, per form.  The scan of the whole bank is given as a view list and routed down the shortlist branch
(one slice, lean form) by the two launch-shape knobs, which the library reads when it first scans.
-> one JSON line (profiles/k1mfma_real_bank.json)"""
import json
import os
import sys

os.environ["SFMLOC_K1_SCREEN_BATCH"] = "1"
os.environ["SFMLOC_K1_QSPLIT"] = "1"

import numpy as np  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402


def measure(q, bank, ratio):
    view_off = np.arange(0, len(bank) + 1, len(bank) // 200, dtype=np.uint32)
    view_off[-1] = len(bank)
    sel = np.arange(len(view_off) - 1, dtype=np.uint32)
    out = {}
    for mfma in (0, 1):
        p = S.default_params(profile=1, dist_ratio=ratio, k1_mfma=mfma)
        with S.Map(sel, view_off, bank, params=p) as dm:
            dq = dm.query(q)
            dm.match_putative(dq, sel)
            dm.sync()
            dm.stats_reset()
            for _ in range(10):
                dm.match_putative(dq, sel)
            dm.sync()
            st = dm.stats()
            out["matrix_core" if mfma else "popcount"] = {
                "hamming_stage_ms": round(st.total_ms[0] / st.launches[0], 4),
                "rows_flagged_frac": round(st.hamming_rows_flagged / 10 / len(bank), 5),
                "pairs_finished_frac": round(st.hamming_pairs_finished / st.hamming_pairs, 5),
                "matches": int(dm.putative_read()[0].sum())}
            dq.close()
    assert out["matrix_core"]["matches"] == out["popcount"]["matches"]
    assert out["matrix_core"]["pairs_finished_frac"] == 0 and out["popcount"]["pairs_finished_frac"] > 0
    out["speedup"] = round(out["popcount"]["hamming_stage_ms"] / out["matrix_core"]["hamming_stage_ms"], 3)
    return out


def main():
    q, bank, info = synth.mldb_like_bank(S)
    res = {"rows": int(len(bank)), "nq": int(len(q)), "bank_stats": info}
    for ratio in (0.6, 0.8):
        res[f"mldb_like_ratio_{ratio}"] = measure(q, bank, ratio)
    rng = np.random.Generator(np.random.PCG64(3))
    uq = synth.random_descriptors(rng, len(q))
    ub = synth.random_descriptors(rng, len(bank))
    idx = rng.choice(len(ub), len(ub) // 700, replace=False)   # ~0.14 % true matches, as on the headline's data
    ub[idx] = synth.flip_bits(rng, uq[rng.integers(0, len(uq), len(idx))], 40)
    res["uniform_ratio_0.6"] = measure(uq, ub, 0.6)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
