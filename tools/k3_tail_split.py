#!/usr/bin/env python3
"""Where the wide K3 kernel's time goes for a headline query alone, from the in-kernel time stamps (the instrumented build
of tools/k35_stamps.py, SFMLOC_LIB_PATH pointing at it).  Per surviving view -- a view whose last-arriving workgroup went on
alone -- the time from the kernel's first entry to that workgroup's exit is split into
  (a) prelude + first batch, up to the last arrival having fetched the other workgroups' results (first tag 3),
  (b) the lone workgroup's solves (later tags 3),
  (c) its evaluation rounds (tags 4),
  (d) fetching the sorted inlier list of a new best model (tags 6 -> 7: rebuild_inliers, or the copy that replaces it),
  (e) the rest: flattening, replay, closing a batch, writing the result out.
The kernel lasts as long as its slowest view, so the shares are given for that view of each query and as the mean over all
surviving views.  usage: k3_tail_split.py [n_queries]   (VIEWS=... for a smaller map)"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (synth_bow)
import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402
from sfmlocalization_amd import _lib  # noqa: E402

PARTS = ("a first batch", "b solves", "c eval rounds", "d list fetch", "e rest")


def split_view(tags, tim, t0):
    """one view slot's events -> (parts in us, tail batches, list fetches, end in us) or None (no lone workgroup)"""
    n = int((tags > 0).sum())
    if n <= 2 or tags[n - 1] != 9 or 3 not in tags[:n]:
        return None
    parts = dict.fromkeys(PARTS, 0.0)
    prev, seen3 = t0, False
    for k in range(n):
        t, tag = int(tim[k]), int(tags[k])
        if k < 2:            # tags 1, 2 of whichever workgroup of the view stored last: inside (a) either way
            continue
        d = (t - prev) / 100.0
        if tag == 3 and not seen3:
            parts["a first batch"] += d
            seen3 = True
        elif tag == 3:
            parts["b solves"] += d
        elif tag == 4:
            parts["c eval rounds"] += d
        elif tag == 7:
            parts["d list fetch"] += d
        else:
            parts["e rest"] += d
        prev = t
    return parts, int((tags[:n] == 3).sum()) - 1, int((tags[:n] == 6).sum()), (int(tim[n - 1]) - t0) / 100.0


def main():
    n_q = int(sys.argv[1]) if len(sys.argv) > 1 else 8
    views = int(os.environ.get("VIEWS", "10000"))
    L = _lib.load()
    L.sfmloc_debug_stamps_read.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_ulonglong]
    counts = hasattr(L, "sfmloc_debug_k3_list_counts")
    m = synth.make_map(2, n_views=views, desc_per_view=2000)
    queries = [synth.make_query(m, 1000 + i, n_feat=2000) for i in range(n_q)]
    bow, qbow = bench.synth_bow(m, queries)
    params = S.default_params(device=0, profile=0, ransac_round=25)
    dm = S.Map(m.view_id, m.view_off, m.desc, params=params, view_wh=m.view_wh, kpt_xy=m.kpt_xy,
               row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic,
               bow=bow)
    dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in queries]
    for dq, qb in zip(dqs, qbow):
        dq.set_bow(qb)
    c = dm.context()
    for dq in dqs:  # warm
        c.begin_bow(dq, None, 100)
        c.end()
    if counts:
        S.capi.k3_list_counts(reset=True)
    slowest, every, n_batches, n_fetch = [], [], [], []
    for qi, dq in enumerate(dqs):
        L.sfmloc_debug_stamps_clear()
        c.begin_bow(dq, None, 100)
        c.end()
        f = np.zeros(256 * 64, np.uint64)
        L.sfmloc_debug_stamps_read(2, f.ctypes.data, f.size)
        tags = (f >> np.uint64(48)).astype(np.int64).reshape(256, 64)
        tim = (f & np.uint64(0xFFFFFFFFFFFF)).astype(np.int64).reshape(256, 64)
        t0 = min(int(tim[b, 0]) for b in range(256) if tags[b, 0] == 1)
        rows = [r for r in (split_view(tags[b], tim[b], t0) for b in range(256)) if r]
        if not rows:
            print(f"query {qi}: no surviving view")
            continue
        rows.sort(key=lambda r: -r[3])
        for parts, nb, nf, end in rows:
            print(f"query {qi}: view ends {end:6.1f} us | " + " | ".join(f"{k} {parts[k]:5.1f}" for k in PARTS)
                  + f" | tail batches {nb}, list fetches {nf}")
            every.append([parts[k] for k in PARTS])
            n_batches.append(nb)
            n_fetch.append(nf)
        slowest.append([rows[0][0][k] for k in PARTS])
    for name, arr in (("the slowest view of each query (the kernel's duration)", np.array(slowest)),
                      ("all surviving views", np.array(every))):
        tot = arr.sum(axis=1).mean()
        print(f"== {name}: {len(arr)} views, mean {tot:.1f} us from the kernel's first entry to the view's exit; shares: "
              + ", ".join(f"{k} {arr[:, i].mean():.1f} us = {100 * arr[:, i].mean() / tot:.1f} %" for i, k in enumerate(PARTS)))
    print(f"== per surviving view: {np.mean(n_batches):.2f} tail batches, {np.mean(n_fetch):.2f} list fetches "
          f"(the first batch's included)")
    if counts:
        got = S.capi.k3_list_counts()
        print(f"== list fetches served by copy {got[0]}, by rebuild {got[1]}")


if __name__ == "__main__":
    main()
