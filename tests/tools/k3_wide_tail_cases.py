#!/usr/bin/env python3
"""Scenes and drivers of tests/test_gpu_k3_wide_tail.py: the views whose last-arriving workgroup of K3's wide form goes on
alone -- the tail of a view's AC-RANSAC, on four or on eight waves (SFMLOC_K3_WIDE_WAVES), with a new best model's sorted
inlier list copied from the wave that evaluated it or rebuilt by wave 0.  CASES maps a name to (scene, parameters); a
case's queries are the same in the test (which takes them through the oracle) and here.  Run as a program it takes every
case through the device and prints one JSON line: {case: [record per query], "list_counts": {case: [copied, rebuilt]}}
-- the test runs it in a child process per knob value, which the library reads once."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import k3k5_shared_cases as shared  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402


def scene25():
    m = synth.make_map(25, n_views=40, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=140)
    return m, [synth.make_query(m, 400 + k, n_feat=800, n_copies=200, outlier_frac=0.3) for k in range(6)]


def big_view_scene():
    """views of 513 .. 1 024 putative matches: 16 residuals per lane in the register sort"""
    m = synth.make_map(75, n_views=3, desc_per_view=1100, views_per_place=3, landmarks_per_place=1300, obs_per_view=1000,
                       map_flips=8)
    return m, [synth.make_query(m, 750 + k, n_feat=1200, n_copies=1000, outlier_frac=0.1, query_flips=10) for k in range(1, 4)]


def small_view_scene(targets, oracle_localize):
    """edge_scene with views 33 / 34 / 37 trimmed to `targets` putative matches (the oracle says which rows those are)"""
    m, q, rng = shared.edge_scene()
    e0 = oracle_localize(m, q.desc, q.kpt_xy, (q.width, q.height), ransac_round=25)
    shared.trim_views(m, e0["put_count"], e0["put_i"], targets, rng)
    return m, [q]


SMALL_TARGETS = {33: 15, 34: 16, 37: 10}

# name -> (scene, queries taken, device parameters = the oracle's keywords, contexts: 0 = Map.localize, one after the other)
CASES = {
    "default_budget": ("scene25", 4, dict(ransac_round=25), 0),
    "ransac_round_3": ("scene25", 3, dict(ransac_round=3), 0),
    "ransac_round_40": ("scene25", 3, dict(ransac_round=40), 0),
    "ransac_round_200": ("scene25", 4, dict(ransac_round=200), 0),
    "views_513_to_1024": ("big", 3, dict(ransac_round=25, p3p_max_iteration=300), 0),
    "min_putative_16": ("small", 1, dict(ransac_round=25), 0),
    "min_putative_8": ("small", 1, dict(ransac_round=25, min_putative=8), 0),
    "three_contexts": ("scene25", 6, dict(ransac_round=25), 3),
}


def scenes(oracle_localize):
    return {"scene25": scene25(), "big": big_view_scene(), "small": small_view_scene(SMALL_TARGETS, oracle_localize)}


def run_case(scene, n, params, n_ctx):
    m, qs = scene
    S.capi.k3_list_counts(reset=True)
    with shared.device_map(m, **params) as dm:
        dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs[:n]]
        got = shared.run_shared(dm, dqs, n_ctx=n_ctx) if n_ctx else [dm.localize(dq) for dq in dqs]
        for dq in dqs:
            dq.close()
    return [shared.record(r) for r in got], list(S.capi.k3_list_counts())


def main():
    from oracle import pipeline as opipe
    sc = scenes(opipe.localize)
    out, counts = {}, {}
    for name, (scene, n, params, n_ctx) in CASES.items():
        out[name], counts[name] = run_case(sc[scene], n, params, n_ctx)
    out["list_counts"] = counts
    print(json.dumps(out))


if __name__ == "__main__":
    main()
