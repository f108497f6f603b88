"""The matrix-core form of the view-list scan (k_hamming_screen_mfma, params.k1_mfma = 1) against the CPU oracle and
against the popcount form (k1_mfma = 0) on the same inputs, in one process.

Run by tests/test_gpu_hamming_mfma.py in a child process with SFMLOC_K1_SCREEN_BATCH=1 and SFMLOC_K1_QSPLIT=1: the
library then sends EVERY screened scan of a view list down the branch a shortlist takes while the GPU is shared (one
slice, the lean form) -- the branch the switch acts on -- whatever the list's length; both knobs are read when the
library first scans, hence the child.  Every case checks through the statistics that the intended form ran: the
matrix-core form finishes no pairs (hamming_pairs_finished = 0), the popcount form does.

usage: k1_mfma_cases.py <group> ; groups: sizes, structured, views, gang, whole_path
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import sfmlocalization_amd as S  # noqa: E402
import synthdata as synth  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402
from oracle import oracle_c  # noqa: E402

NAMES = ("view_count", "match_i", "match_j", "match_d")


def scan(q, bank, view_off, view_sel, ratio, mfma):
    """-> (putative_read(), rows flagged, pairs finished, the per-row keys of the rows that carry a pair)"""
    nv = len(view_off) - 1
    p = S.default_params(dist_ratio=ratio, k1_mfma=1 if mfma else 0)
    with S.Map(np.arange(nv, dtype=np.uint32) * 2 + 1, view_off, bank, params=p) as m:
        qq = m.query(q)
        m.stats_reset()
        m.match_putative(qq, view_sel)
        got = m.putative_read()
        s0, _ = m.putative_read_rows()
        st = m.stats()
        # the same query after another one: stale flags or partial results must not leak through
        q2 = m.query(q[::-1].copy())
        m.match_putative(q2, view_sel)
        m.match_putative(qq, view_sel)
        again = m.putative_read()
        for a, b in zip(got, again):
            np.testing.assert_array_equal(a, b, err_msg="same query after another one on the same context")
        q2.close()
        qq.close()
    return got, int(st.hamming_rows_flagged), int(st.hamming_pairs_finished), s0 != S.NOMATCH


def check(q, bank, view_off, view_sel, ratio=0.6, what="", flag_bound=None):
    exp = oracle_c.match_to_query(q, bank, view_off, view_sel, ratio, threads=4)
    got_m, flagged_m, finished_m, have_m = scan(q, bank, view_off, view_sel, ratio, True)
    got_p, flagged_p, finished_p, have_p = scan(q, bank, view_off, view_sel, ratio, False)
    assert finished_m == 0, f"{what}: the matrix-core form did not run (pairs finished {finished_m})"
    assert flagged_m > 0 or got_m[0].sum() == 0, f"{what}: matches but no flagged row: the scan was not screened"
    assert finished_p > 0 or flagged_p == 0, f"{what}: the popcount form did not run"
    for name, a, b, e in zip(NAMES, got_m, got_p, exp):
        np.testing.assert_array_equal(a, e, err_msg=f"{what}: matrix-core form vs oracle: {name}")
        np.testing.assert_array_equal(a, b, err_msg=f"{what}: matrix-core form vs popcount form: {name}")
    # the flagged rows (those that carry an exact pair afterwards) cover every accepted row
    acc = np.zeros(len(bank), bool)
    views = range(len(view_off) - 1) if view_sel is None else view_sel
    for v in views:
        o = int(view_off[v])
        acc[o + got_m[1][o:o + int(got_m[0][v])].astype(np.int64)] = True
    assert have_m[acc].all(), f"{what}: an accepted row was not flagged"
    print(f"{what}: matches {int(got_m[0].sum())}, rows flagged matrix-core {flagged_m} popcount {flagged_p}")
    if flag_bound is not None:
        assert flagged_m <= flag_bound * max(flagged_p, 1), f"{what}: threshold gone loose: {flagged_m} vs {flagged_p}"
    return got_m


def planted(rng, nq, n_rows, kind="uniform"):
    q = synth.random_descriptors(rng, nq)
    bank = synth.random_descriptors(rng, n_rows)
    if kind == "sparse":  # ~1/8 ones: small distances, large thresholds
        q &= synth.random_descriptors(rng, nq) & synth.random_descriptors(rng, nq)
        bank &= synth.random_descriptors(rng, n_rows) & synth.random_descriptors(rng, n_rows)
    n_p = n_rows // 4
    bank[:n_p] = synth.flip_bits(rng, q[rng.integers(0, nq, n_p)], 40)          # near-duplicates of query rows
    bank[n_p:n_p + 50] = q[rng.integers(0, nq, 50)]                              # bank row = a query row: distance 0
    q[100:140] = q[100]                                                          # exact ties between query rows
    q[200:260] = synth.flip_bits(rng, np.repeat(q[200:201], 60, 0), 3)
    bank[n_p + 50:n_p + 60] = q[100]                                             # ... and bank rows that hit the tie
    # the accumulator extremes over all 64 stored bytes: all ones against all zeros (512) and against itself (0)
    q[5] = 0xFF
    q[6] = 0x00
    bank[n_rows - 3] = 0xFF
    bank[n_rows - 2] = 0x00
    return q, bank


def group_sizes():
    view_off = np.array([0, 64, 64, 129, 130, 1000, 2100], np.uint32)  # aligned, empty, 1-row and long views
    all_views = np.arange(len(view_off) - 1, dtype=np.uint32)
    for nq in (768, 769, 1000, 2000, 2047, 2049, 5000):
        for ratio in (0.3, 0.6, 0.95, 1.5):
            rng = np.random.Generator(np.random.PCG64(nq * 7 + int(ratio * 100)))
            q, bank = planted(rng, nq, 2100)
            check(q, bank, view_off, all_views, ratio, f"nq={nq} ratio={ratio}", flag_bound=2)


def group_structured():
    view_off = np.array([0, 1000, 1000, 2500, 6000], np.uint32)
    all_views = np.arange(4, dtype=np.uint32)
    for ratio in (0.3, 0.6, 0.95, 1.5):
        rng = np.random.Generator(np.random.PCG64(int(ratio * 100) + 3))
        q, bank = planted(rng, 1500, 6000, "sparse")
        check(q, bank, view_off, all_views, ratio, f"sparse ratio={ratio}")
    # descriptors with the statistics of real M-LDB output (unrelated rows at 222 +- 42 bits instead of 243 +- 11)
    q, bank, _ = synth.mldb_like_bank(S, n_images=12, target_rows=20000, nq=2000)
    view_off = np.linspace(0, len(bank), 11).astype(np.uint32)
    # (no bound on the flagged rows here: the 2 x bound is the uniform bank's.  This form keeps the head's threshold
    # where the popcount form tightens it with every finished pair, and on these descriptors that is worth a factor
    # of 4-7 in flagged rows -- DESIGN.md K1; both counts are printed)
    for ratio in (0.3, 0.6, 0.95, 1.5):
        check(q, bank, view_off, np.arange(10, dtype=np.uint32), ratio, f"M-LDB-like ratio={ratio}")


def group_views():
    rng = np.random.Generator(np.random.PCG64(77))
    nq = 900
    n_rows = 9000 + 4500 + 70 + 5000
    q, bank = planted(rng, nq, n_rows)
    bank[9000:9600] = synth.flip_bits(rng, q[rng.integers(0, nq, 600)], 40)     # matches in the two middle views too
    bank[13400:13570] = synth.flip_bits(rng, q[rng.integers(0, nq, 170)], 40)
    # 9000 rows = 141 blocks; views start off the 64-row blocks, neighbours share blocks
    view_off = np.array([0, 9000, 13500, 13570, n_rows], np.uint32)
    check(q, bank, view_off, np.arange(4, dtype=np.uint32), 0.6, "long unaligned views", flag_bound=2)
    # (a list must cover more than half of the bank's blocks here, else the scan is split over query parts and takes
    # the exact kernel in either setting; check() asserts through the statistics that it did not)
    check(q, bank, view_off, np.array([0, 1, 2], np.uint32), 0.6, "views sharing bank blocks, from row 0", flag_bound=2)
    check(q, bank, view_off, np.array([1, 2, 3], np.uint32), 0.6, "views sharing bank blocks, off a block", flag_bound=2)
    check(q, bank, view_off, np.array([0, 3], np.uint32), 0.6, "views apart", flag_bound=2)
    # a device-built list is padded with kNoBlock up to its bound: the BoW chain on a map whose views are ragged
    m = synth.make_map(5, n_views=40, desc_per_view=300, views_per_place=8, landmarks_per_place=200, obs_per_view=80,
                       ragged=True)
    qy = synth.make_query(m, 9, n_feat=1200, n_copies=120)
    rngb = np.random.Generator(np.random.PCG64(1))
    bow = np.sqrt(rngb.random((40, 64))).astype(np.float32)
    res = []
    for mfma in (1, 0):
        p = S.default_params(k1_mfma=mfma)
        with S.Map(m.view_id, m.view_off, m.desc, params=p, view_wh=m.view_wh, kpt_xy=m.kpt_xy,
                   row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X,
                   intrinsic=m.intrinsic, bow=bow) as dm:
            dq = dm.query(qy.desc, qy.kpt_xy, qy.width, qy.height)
            pose, pq, pl = dm.localize_bow(dq, bow[3], 12)
            res.append((capi.result_fingerprint(pose, pq, pl), [a.copy() for a in dm.putative_read()]))
            dq.close()
    assert res[0][0] == res[1][0], "shortlist chain (padded block list): fingerprints differ between the forms"
    for a, b in zip(res[0][1], res[1][1]):
        np.testing.assert_array_equal(a, b)
    print("padded device-built block list: equal")


KNN = 120  # of 200 views: a shortlist over more than half of the bank's blocks is scanned in one piece (no query split)


def _campaign(mfma, n_members, n_queries=64):
    """configs[2] in shape at reduced size: BoW shortlist, then the whole path, through the asynchronous entry points;
    n_members = 0: one query at a time, else gang sessions of that many contexts -> fingerprints"""
    m = synth.make_map(21, n_views=200, desc_per_view=500, views_per_place=10, landmarks_per_place=400,
                       obs_per_view=200)
    rng = np.random.Generator(np.random.PCG64(2))
    place_vec = np.sqrt(rng.random((int(m.view_place.max()) + 1, 64)))
    bow = (place_vec[m.view_place] + 0.05 * rng.random((200, 64))).astype(np.float32)  # views of a place lie together
    qs = [synth.make_query(m, 100 + i, n_feat=1000, n_copies=200) for i in range(8)]
    fps = []
    p = S.default_params(k1_mfma=mfma)
    with S.Map(m.view_id, m.view_off, m.desc, params=p, view_wh=m.view_wh, kpt_xy=m.kpt_xy, row_landmark=m.row_landmark,
               landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic, bow=bow) as dm:
        dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs]
        place_bow = [bow[int(np.flatnonzero(m.view_place == q.place)[0])] for q in qs]
        n_ctx = max(n_members, 1)
        ctxs = [dm.context() for _ in range(n_ctx)]
        k = 0
        while k < n_queries:
            batch = list(range(k, min(k + n_ctx, n_queries)))
            if n_members:
                with capi.gang(ctxs[:len(batch)]):
                    for c, i in zip(ctxs, batch):
                        c.begin_bow(dqs[i % 8], place_bow[i % 8], KNN)
            else:
                ctxs[0].begin_bow(dqs[batch[0] % 8], place_bow[batch[0] % 8], KNN)
            for c, i in zip(ctxs, batch):
                pose, pq, pl = c.end()
                fps.append(capi.result_fingerprint(pose, pq, pl))
            k += len(batch)
        # the intended form ran: the matrix-core form finishes no pairs, the popcount form does
        st = dm.stats()
        assert st.hamming_rows_flagged > 0, "no scan flagged a row: the campaign does not exercise the screened scan"
        if mfma:
            assert st.hamming_pairs_finished == 0, "the matrix-core form did not run in this campaign"
        else:
            assert st.hamming_pairs_finished > 0, "the popcount form did not run in this campaign"
        for c in ctxs:
            c.close()
        for d in dqs:
            d.close()
    return fps


def group_gang():
    single = _campaign(1, 0, 32)
    for n in (2, 32):
        assert _campaign(1, n, 32) == single, f"gang of {n}: fingerprints differ from single flight"
    print("gang sessions of 2 and 32 = single flight")


def group_whole_path():
    on, off = _campaign(1, 0, 64), _campaign(0, 0, 64)
    assert on == off, "whole path: fingerprints differ between the forms"
    print(f"whole path, 64 queries: fingerprints equal ({len(set(on))} distinct)")


if __name__ == "__main__":
    {"sizes": group_sizes, "structured": group_structured, "views": group_views, "gang": group_gang,
     "whole_path": group_whole_path}[sys.argv[1]]()
    print("OK")
