#!/usr/bin/env python3
"""Scenes and drivers of tests/test_gpu_k3k5_shared_forms.py: queries taken through several contexts with begin / end
interleaved, so that other contexts have work queued when each begins -- the forms K3 and K5 take on a shared GPU.
Run as a program it prints the K5 case's results as one JSON line (the test runs it in a child process with the round
policy forced through the environment, which the library reads once)."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402


def bits(a):
    a = np.ascontiguousarray(a, np.float64)
    u = a.view(np.uint64).copy()
    u[np.isnan(a)] = 0x7FF8000000000000
    return u


def device_map(m, **params):
    p = dict(ransac_round=25)
    p.update(params)
    bow = p.pop("bow", None)
    return S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(**p), view_wh=m.view_wh, kpt_xy=m.kpt_xy,
                 row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic,
                 bow=bow)


def record(res):
    pose, pq, pl = res
    return {"ok": bool(pose.ok), "P": [int(x) for x in bits(np.array(pose.P))], "pq": [int(x) for x in pq],
            "pl": [int(x) for x in pl], "n_put": int(pose.n_putative_views), "n_geo": int(pose.n_geometric_views),
            "n_inl": int(pose.n_inliers) if pose.ok else 0}


LAST = {}   # rows_flagged: what the screened scans of the last run_shared flagged (0: no scan was screened)


def run_shared(dm, dqs, n_ctx=3, begin=None):
    """every query through n_ctx contexts in turn, begin / end interleaved: from the second begin on, other contexts of
    the map have work queued.  begin(ctx, i): how query i starts (default: ctx.begin(dqs[i]))."""
    ctxs = [dm.context() for _ in range(n_ctx)]
    dm.stats_reset()
    got = [None] * len(dqs)
    for i in range(len(dqs)):
        c = ctxs[i % n_ctx]
        if i >= n_ctx:
            got[i - n_ctx] = c.end()
        if begin is None:
            c.begin(dqs[i])
        else:
            begin(c, i)
    for i in range(max(0, len(dqs) - n_ctx), len(dqs)):
        got[i] = ctxs[i % n_ctx].end()
    LAST["rows_flagged"] = int(dm.stats().hamming_rows_flagged)   # (of the map's contexts since the last stats_reset)
    for c in ctxs:
        c.close()
    return got


def edge_scene():
    """The scene of test_concurrent_contexts_equal_sequential (test_gpu_geom.make_scene(25)) and an 800-feature query of
    its place 3 (views 30 .. 39, 400 rows each, so that a view begins and ends inside a 64-row block unless its index is
    a multiple of four), edited so that
      view 33 keeps exactly min_putative - 1 = 15 accepted matches, view 34 exactly min_putative = 16,
      view 37 keeps 10 accepted matches and has 12 more rows that the scan flags and the merge rejects: each is the
        nearest row of TWO query rows at the same distance (2 bits), beyond the scan's head of 64 query rows -- nearer
        than the head's threshold, so flagged; nearest and second-nearest equal, so not accepted;
      the rows of their neighbours that share a 64-row block with view 33, 34 or 37 are clutter (a scan of one of these
        views then flags rows of that view only; between 33 and 34 those are rows of the two themselves).
    A match is taken away by replacing the MAP row's descriptor: that touches no other view."""
    m = synth.make_map(25, n_views=40, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=140)
    q = synth.make_query(m, 400, n_feat=800, n_copies=200, outlier_frac=0.3, place=3)
    rng = np.random.Generator(np.random.PCG64(2533))
    off = m.view_off.astype(np.int64)
    # view 37's twelve flagged-and-rejected rows: clutter rows of the view, query rows without a landmark at the tail
    clutter = off[37] + np.nonzero(m.row_landmark[off[37]:off[38]] < 0)[0][:12]
    free_q = np.nonzero(q.landmark < 0)[0]
    free_q = free_q[free_q >= 400][-24:]
    assert len(clutter) == 12 and len(free_q) == 24
    for k, r in enumerate(clutter):
        a, b = m.desc[r].copy(), m.desc[r].copy()
        a[0] ^= 0x03
        b[1] ^= 0x03
        q.desc[free_q[2 * k]] = a
        q.desc[free_q[2 * k + 1]] = b
    for v in (33, 34, 37):
        for lo, hi in ((off[v] & ~63, off[v]), (off[v + 1], (off[v + 1] + 63) & ~63)):
            m.desc[lo:hi] = synth.random_descriptors(rng, int(hi - lo))
    return m, q, rng


def trim_views(m, put_count, put_i, targets, rng):
    """leave `targets[v]` of view v's accepted matches: the map rows of the others become clutter"""
    off = m.view_off.astype(np.int64)
    for v, keep in targets.items():
        rows = off[v] + put_i[off[v]:off[v] + int(put_count[v])].astype(np.int64)
        assert len(rows) >= keep, (v, len(rows))
        drop = rows[keep:]
        m.desc[drop] = synth.random_descriptors(rng, len(drop))


def k5_scene():
    """test_gpu_geom's scene 74: five small queries (at most 512 correspondences) and one large (more: the small round form's
    fallback to the full form is crossed)"""
    m = synth.make_map(74, n_views=5, desc_per_view=1600, views_per_place=5, landmarks_per_place=1900, obs_per_view=1500,
                       map_flips=8)
    qs = [synth.make_query(m, 7400 + k, n_feat=600, n_copies=260) for k in range(3)]
    qs.append(synth.make_query(m, 7420, n_feat=1700, n_copies=1300, outlier_frac=0.1, query_flips=10))
    qs += [synth.make_query(m, 7404 + k, n_feat=600, n_copies=260) for k in range(2)]
    return m, qs


K5_P3P_ITER = 300


def run_k5_case():
    m, qs = k5_scene()
    with device_map(m, p3p_max_iteration=K5_P3P_ITER) as dm:
        dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs]
        got = run_shared(dm, dqs)
        for dq in dqs:
            dq.close()
    return [record(r) for r in got]


if __name__ == "__main__":
    print(json.dumps(run_k5_case()))
