#!/usr/bin/env python3
"""Guided matching (params.guided_matching, -gm) behind every form of K3: the driver that tests/test_gpu_guided.py shares
with its child processes.  K3 writes the winning F and errorMax -- the residual of the last entry of its sorted inlier
list -- for the guided band; which kernel form serves a view is decided by knobs the library reads once per process
(SFMLOC_K3_WIDE, _WIDE_2048, _BIG, _WIDE_WAVES, _WAVES_ALONE / _SHARED), so each setting takes all the cases in one child.

stages(dm, q, view_sel) takes one query through the staged calls on the map's own context and returns everything they let
one read: the guided lists per surviving view, the 2D-3D set with its point bits, the resection's iterations, inliers and
pose bits.  oracle_stages(m, exp) is the same record from oracle.pipeline.localize(..., guided=True).  Run as a program it
takes the form scenes of tests/guided_cases.py (tile_edges at nq = 513, k4_hash_big, k4_hash_huge, k4_global) through the
device and prints one JSON line {scene: [record per query]}."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
import guided_cases as G  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402


def bits(a):
    """bit patterns, every NaN mapped to one pattern (test_gpu_geom.bits)"""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = 0x7FF8000000000000
    return b


def device_map(m, **params):
    p = dict(ransac_round=25, guided_matching=1)
    p.update(params)
    return S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(**p), view_wh=m.view_wh, kpt_xy=m.kpt_xy,
                 row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic)


def _lists(view_off, count, a, b):
    """the lists of the views with a count, back to back"""
    keep = [np.arange(int(view_off[v]), int(view_off[v]) + int(count[v])) for v in np.nonzero(count)[0]]
    idx = np.concatenate(keep) if keep else np.zeros(0, np.int64)
    return np.asarray(a)[idx].astype(np.uint32), np.asarray(b)[idx].astype(np.uint32)


def stages(dm, m, q, view_sel=None, read_must_raise=False):
    dq = dm.query(q.desc, q.kpt_xy, q.width, q.height)
    out = {}
    dm.match_putative(dq, view_sel)
    out["put_count"], out["put_i"], out["put_j"], out["put_d"] = dm.putative_read()
    dm.geometric_filter(dq)
    gc, gi, gj = dm.geometric_read_pairs()
    out["geo_count"] = gc
    out["geo_i"], out["geo_j"] = _lists(m.view_off, gc, gi, gj)
    if read_must_raise:
        try:
            dm.geometric_read()                 # guided matches are not indices into the putative lists
            out["read_raised"] = False
        except S.SfmlocError:
            out["read_raised"] = True
    dm.match_set(dq)
    qf, lm, p2, p3 = dm.match_set_read()
    out.update(ms_qfeat=qf, ms_landmark=lm, pt2d=bits(p2).ravel(), pt3d=bits(p3).ravel())
    dm.resection(dq)
    pose, pq, pl, ii = dm.pose_read()
    out.update(ok=bool(pose.ok), n_2d3d=int(pose.n_matches_2d3d), iters=int(pose.iterations),
               n_inliers=int(pose.n_inliers) if pose.ok else 0, inlier_idx=ii, pair_qfeat=pq, pair_landmark=pl)
    if pose.ok:
        out.update(P=bits(np.array(pose.P)), R=bits(np.array(pose.R)), center=bits(np.array(pose.center)),
                   K=bits(np.array(pose.K)))
    dq.close()
    return out


def oracle_stages(m, exp):
    gc = exp["geo_count"]
    out = {k: exp[k] for k in ("put_count", "put_i", "put_j", "put_d", "geo_count", "ms_qfeat", "ms_landmark")}
    out["geo_i"], out["geo_j"] = _lists(m.view_off, gc, exp["geo_idx"], exp.get("geo_j", exp["geo_idx"]))
    out.update(pt2d=bits(exp["pt2d"]).ravel(), pt3d=bits(exp["pt3d"]).ravel(), ok=bool(exp["ok"]),
               n_2d3d=len(exp["ms_qfeat"]), iters=int(exp["p3p"]["iters"]) if "p3p" in exp else 0,
               n_inliers=int(exp["n_inliers"]) if exp["ok"] else 0)
    empty = np.zeros(0, np.uint32)
    out.update(inlier_idx=exp["inlier_idx"] if exp["ok"] else empty, pair_qfeat=exp["pair_qfeat"] if exp["ok"] else empty,
               pair_landmark=exp["pair_landmark"] if exp["ok"] else empty)
    if exp["ok"]:
        out.update(P=bits(exp["P"].ravel()), R=bits(exp["R"].ravel()), center=bits(exp["center"].ravel()),
                   K=bits(exp["K"].ravel()))
    return out


FORM_FIELDS = ("geo_count", "geo_i", "geo_j", "ms_qfeat", "ms_landmark", "pt2d", "pt3d", "ok", "n_2d3d", "iters",
               "n_inliers", "inlier_idx", "pair_qfeat", "pair_landmark", "P", "R", "center", "K")


def jsonable(rec):
    """what a child prints of a record: the guided lists, the ms set, the pose bits"""
    return {k: ([int(x) for x in np.asarray(rec[k]).ravel()] if isinstance(rec[k], np.ndarray) else rec[k])
            for k in FORM_FIELDS if k in rec}


def main():
    out = {}
    for name in G.FORM_SCENES:
        s = G.scene(name)
        with device_map(s.m, **s.params) as dm:
            out[name] = [jsonable(stages(dm, s.m, s.queries[k], s.sel(k))) for k in G.form_queries(name)]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
