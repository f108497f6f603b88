"""GPU: the forms K3 and K5 take while other contexts of the map have work queued (acransac.hip launch_fmatrix_filter,
make_p3p_args): K3's wide form -- one workgroup per iteration of a view's first batch -- with K2 folded in, every
workgroup of a view building the view's putative list for itself unless the view's flagged rows already prove that the
view is not the kernel's; the plain forms for what the wide one does not take; K5's rounds as a shared GPU now sizes
them.  Every form gives the same bits: each query is compared with the oracle and with the same query taken alone
(Map.localize), pose bits, inlier pairs, n_putative_views and n_geometric_views.  No timing here."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sfmlocalization_amd as S
import synthdata as synth
from oracle import oracle_c as oc
from oracle import pipeline as opipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("k3k5_shared_cases", os.path.join(ROOT, "tests", "tools", "k3k5_shared_cases.py"))
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)
bits = cases.bits


def same(a, b, what):
    """two (pose, pair_qfeat, pair_landmark) results, bit for bit"""
    assert bool(a[0].ok) == bool(b[0].ok), what
    assert a[0].n_putative_views == b[0].n_putative_views and a[0].n_geometric_views == b[0].n_geometric_views, what
    np.testing.assert_array_equal(a[1], b[1], err_msg=what)
    np.testing.assert_array_equal(a[2], b[2], err_msg=what)
    np.testing.assert_array_equal(bits(np.array(a[0].P)), bits(np.array(b[0].P)), err_msg=what)


def equals_oracle(got, exp, what):
    pose, pq, pl = got
    assert bool(pose.ok) == exp["ok"], what
    assert pose.n_matches_2d3d == len(exp["ms_qfeat"]), what
    min_put = S.default_params().min_putative
    assert pose.n_putative_views == int((exp["put_count"] >= min_put).sum()), what
    assert pose.n_geometric_views == int((exp["geo_count"] > 0).sum()), what
    if exp["ok"]:
        assert pose.n_inliers == exp["n_inliers"], what
        np.testing.assert_array_equal(pq, exp["pair_qfeat"], err_msg=what)
        np.testing.assert_array_equal(pl, exp["pair_landmark"], err_msg=what)
        np.testing.assert_array_equal(bits(np.array(pose.P)), bits(exp["P"].ravel()), err_msg=what)


def check_shared(m, dm, qs, what, view_sel=None, **okw):
    """qs through three contexts with begin / end interleaved, against the oracle and against each query alone"""
    exps = [opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), view_sel=view_sel, ransac_round=25, **okw) for q in qs]
    dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs]
    alone = [dm.localize(dq, view_sel) for dq in dqs]
    got = cases.run_shared(dm, dqs, begin=lambda c, i: c.begin(dqs[i], view_sel))
    for i, (a, g, e) in enumerate(zip(alone, got, exps)):
        equals_oracle(g, e, f"{what}: query {i}, GPU shared, against the oracle")
        same(a, g, f"{what}: query {i}, GPU shared against the query alone")
    for dq in dqs:
        dq.close()
    return exps


def scene25():
    return synth.make_map(25, n_views=40, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=140)


def test_wide_form_with_k2_folded_in_while_the_gpu_is_shared(oracle_c):
    """The scene of test_concurrent_contexts_equal_sequential through three contexts, nothing forced: the queries of 700
    features (below the screened scan's 768: K2 is a kernel of its own before the wide form) and the same with 800 (the
    screened scan leaves K2 to K3: the folded form), with all views and with a host view list.  The list covers more than
    half of the map's rows -- a shorter one is scanned in query slices, unscreened -- : the query's place and two more."""
    m = scene25()
    with cases.device_map(m) as dm:
        for n_feat in (700, 800):
            qs = [synth.make_query(m, 400 + k, n_feat=n_feat, n_copies=200, outlier_frac=0.3) for k in range(7)]
            exps = check_shared(m, dm, qs, f"{n_feat} features, all views")
            assert sum(e["ok"] for e in exps) >= 5
            assert (cases.LAST["rows_flagged"] > 0) == (n_feat >= 768)       # the screened scan ran: K2 was K3's
            for k in (0, 3):
                p = qs[k].place
                sel = np.nonzero((m.view_place == p) | (m.view_place == (p + 1) % 4) | (m.view_place == (p + 2) % 4))[0]
                sel = sel.astype(np.uint32)
                e = check_shared(m, dm, [qs[k], qs[k + 1], qs[k + 2], qs[k]], f"{n_feat} features, host view list", sel)
                assert 0 < (e[0]["put_count"] >= 16).sum() < len(sel)
                assert (cases.LAST["rows_flagged"] > 0) == (n_feat >= 768)


def test_wide_form_with_k2_folded_in_on_a_device_shortlist(oracle_c):
    """begin_bow with a shortlist that never leaves the device, three contexts: the shortlist holds views of the query's
    place and views of other places, so only some of the listed views reach 16 matches -- the others are the real empty
    views the flagged-row count sends all but a view's first workgroup away from."""
    m = scene25()
    rng = np.random.Generator(np.random.PCG64(77))
    bow = np.sqrt(rng.random((m.n_views, 64))).astype(np.float32)
    knn = 22                                                   # (more than half of the map: one screened scan, see above)
    with cases.device_map(m, bow=bow) as dm:
        qs = [synth.make_query(m, 500 + k, n_feat=800, n_copies=200, outlier_frac=0.3) for k in range(6)]
        # the query's .bow: between a view of its own place and one of another place
        qbs = [(0.5 * bow[np.nonzero(m.view_place == q.place)[0][k % 10]] + 0.5 * bow[(7 * k + 3) % m.n_views]
                + rng.normal(0, 0.02, 64)).astype(np.float32) for k, q in enumerate(qs)]
        sels = [oc.bow_select(bow, qb, knn, None) for qb in qbs]
        exps = [opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), view_sel=s, ransac_round=25) for q, s in zip(qs, sels)]
        some = [int((e["put_count"][s] >= 16).sum()) for e, s in zip(exps, sels)]
        assert all(0 < n < knn for n in some), some          # listed views with and without 16 matches, in every list
        dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs]
        got = cases.run_shared(dm, dqs, begin=lambda c, i: c.begin_bow(dqs[i], qbs[i], knn))
        assert cases.LAST["rows_flagged"] > 0
        for i, (g, e, s) in enumerate(zip(got, exps, sels)):
            equals_oracle(g, e, f"device shortlist: query {i}")
            same(dm.localize(dqs[i], s), g, f"device shortlist: query {i} against the query alone on the same views")
        for dq in dqs:
            dq.close()


def test_edges_of_the_flagged_row_count(oracle_c):
    """The views the early exit must get right (tests/tools/k3k5_shared_cases.py edge_scene): exactly min_putative - 1
    and exactly min_putative accepted matches; at least 16 flagged rows of which fewer than 16 are accepted (the count
    lets the workgroups through, the merge then sends them away); views that begin and end inside a 64-row block shared
    with a neighbour (the edge masks).  The counts are the oracle's and the scan's own and are asserted first."""
    m, q, rng = cases.edge_scene()
    e0 = opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), ransac_round=25)
    min_put = S.default_params().min_putative
    cases.trim_views(m, e0["put_count"], e0["put_i"], {33: min_put - 1, 34: min_put, 37: 10}, rng)
    exp = opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), ransac_round=25)
    assert min_put == 16 and list(exp["put_count"][[33, 34, 37]]) == [15, 16, 10], exp["put_count"][30:40]
    for v in (33, 34, 37):                                    # first and last block shared with the neighbours
        assert m.view_off[v] % 64 != 0 and m.view_off[v + 1] % 64 != 0
    assert all(exp["put_count"][v] > 16 for v in (32, 35, 36, 38))   # ... which have matches of their own
    assert q.desc.shape[0] >= 768                             # the screened scan: flags exist and K2 is left to K3
    with cases.device_map(m) as dm:
        dq = dm.query(q.desc, q.kpt_xy, q.width, q.height)
        # what the scan flags in each of the three views: a list of 23 views of other places (more than half of the map,
        # so that the scan is one screened scan) without and with the view, whose neighbours' rows in the shared blocks are
        # clutter.  View 33: 15 flagged rows, the workgroups leave on the count; view 34: exactly 16, the smallest count
        # that lets them through (a `<=` in the exit would send them away); view 37: through on the count, away on the merge
        others = np.arange(23, dtype=np.uint32)
        assert exp["put_count"][:23].sum() == 0

        def rows_flagged(sel):
            dm.stats_reset()
            dm.match_putative(dq, sel)
            return int(dm.stats().hamming_rows_flagged)
        base = rows_flagged(others)
        flagged = {v: rows_flagged(np.append(others, np.uint32(v))) - base for v in (33, 34, 37)}
        print("rows flagged per view:", flagged, "in the 23 other views:", base)
        assert flagged[33] == min_put - 1 and flagged[34] == min_put and flagged[37] >= 16, flagged
        assert int(dm.putative_read()[0][37]) == 10
        dq.close()
        other = [synth.make_query(m, 410 + k, n_feat=800, n_copies=200, outlier_frac=0.3) for k in range(2)]
        check_shared(m, dm, [other[0], q, other[1], q, q], "edge views, all views")
        assert cases.LAST["rows_flagged"] > 0
        sel = np.concatenate([np.arange(20), [29, 31, 33, 34, 35, 37, 38]]).astype(np.uint32)
        check_shared(m, dm, [q, other[0], q, q], "edge views, host view list", sel)
        assert cases.LAST["rows_flagged"] > 0


def test_plain_forms_take_what_the_wide_form_does_not_while_shared(oracle_c):
    """Shared GPU, nothing forced.  A view list longer than the wide form's 256 result slots takes the plain forms
    (k_fmatrix_fast<4, 512>).  Views above 512 / 1 024 putative matches (the maps of
    test_k3_register_form_for_513_to_1024_matches_per_view and test_k3_wide_form_for_1025_to_2048_matches_per_view, three
    views each, so the wide form serves them): the first query finds them in k_fmatrix_filter, the following ones in the
    wide 1 024-match instance with K2 folded in, or -- Map::k3_huge_credit -- in the 2 048-match instance behind a K2
    launch of its own.  The result is the oracle's and the lone query's in every case."""
    m = synth.make_map(26, n_views=260, desc_per_view=100, views_per_place=10, landmarks_per_place=200, obs_per_view=80)
    with cases.device_map(m) as dm:
        qs = [synth.make_query(m, 600 + k, n_feat=800, n_copies=150, outlier_frac=0.3) for k in range(4)]
        exps = check_shared(m, dm, qs, "260 views")
        assert all((e["put_count"] >= 16).sum() > 0 for e in exps)
    for seed, dpv, lm, obs, nf, nc, lo, hi, it in ((75, 1100, 1300, 1000, 1200, 1000, 512, 1024, 300),
                                                   (77, 2100, 2500, 2000, 2300, 2000, 1024, 2048, 200)):
        m = synth.make_map(seed, n_views=3, desc_per_view=dpv, views_per_place=3, landmarks_per_place=lm, obs_per_view=obs,
                           map_flips=8)
        with cases.device_map(m, p3p_max_iteration=it) as dm:
            qs = [synth.make_query(m, seed * 10 + k, n_feat=nf, n_copies=nc, outlier_frac=0.1, query_flips=10) for k in range(4)]
            exps = check_shared(m, dm, qs, f"views of {lo + 1} .. {hi} matches", p3p_max_iteration=it)
            assert all(lo < int(e["put_count"].max()) <= hi for e in exps), [int(e["put_count"].max()) for e in exps]


def test_k5_shared_round_policy_gives_the_bits_of_the_one_it_replaces(oracle_c):
    """Six queries, three in flight, one of them with more than 512 correspondences (the small round form's fallback is
    crossed): K5's rounds as a shared GPU sizes them by default, and -- in child processes, the policy is read when the
    library first runs -- the policy this replaces (max(64, 3 t) hypotheses per round, the coming round's hypotheses
    prepared by the replaying workgroup) and full batches with the hypotheses prepared ahead.  The oracle's bits each time."""
    m, qs = cases.k5_scene()
    exps = [opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), ransac_round=25, p3p_max_iteration=cases.K5_P3P_ITER)
            for q in qs]
    sizes = [len(e["ms_qfeat"]) for e in exps]
    assert max(sizes) > 512 and sorted(sizes)[-2] <= 512 and all(e["ok"] for e in exps), sizes
    want = [{"ok": True, "P": [int(x) for x in bits(e["P"].ravel())], "pq": [int(x) for x in e["pair_qfeat"]],
             "pl": [int(x) for x in e["pair_landmark"]], "n_put": int((e["put_count"] >= 16).sum()),
             "n_geo": int((e["geo_count"] > 0).sum()), "n_inl": int(e["n_inliers"])} for e in exps]
    assert cases.run_k5_case() == want, "the default policy"
    for extra in ({"SFMLOC_P3P_PREP_AHEAD": "1"},      # the parent's rule exactly: adaptive and prepared ahead while shared
                  {"SFMLOC_P3P_ADAPTIVE": "1", "SFMLOC_P3P_PREP_AHEAD": "2"},
                  {"SFMLOC_P3P_ADAPTIVE": "0", "SFMLOC_P3P_PREP_AHEAD": "2"},
                  {"SFMLOC_P3P_ADAPTIVE": "0", "SFMLOC_P3P_PREP_AHEAD": "0"}):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "k3k5_shared_cases.py")],
                           env=dict(os.environ, **extra), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (extra, r.stdout[-2000:] + r.stderr[-2000:])
        assert json.loads(r.stdout.strip().splitlines()[-1]) == want, extra
