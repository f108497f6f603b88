"""GPU: guided matching (params.guided_matching, -gm) wherever a query's geometric stage changes with it -- behind every
form of K3 (which writes the F and errorMax the band is cut with), at k_guided_rows' tile and block edges, at the edges of
its selection rule, through K4's three look-ups of "the last putative match with this query feature", in the sharded
export, in a gang session and in the pair path.  Scenes: tests/guided_cases.py (tests/test_guided_cases_cpu.py asserts on
the oracle's side that each reaches its path).  Every comparison is with oracle.pipeline (guided=True), bit for bit."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import guided_cases as G
import sfmlocalization_amd as S
import synthdata as synth
from oracle import pipeline as opipe
from sfmlocalization_amd import capi

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "guided_forms_cases.py")
_spec = importlib.util.spec_from_file_location("guided_forms_cases", TOOL)
forms = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(forms)
bits = forms.bits

STAGE_FIELDS = ("put_count", "put_i", "put_j", "put_d",                      # putative_read
                "geo_count", "geo_i", "geo_j",                                  # geometric_read_pairs
                "ms_qfeat", "ms_landmark", "pt2d", "pt3d",                      # match_set_read
                "ok", "n_2d3d", "iters", "n_inliers", "inlier_idx", "pair_qfeat", "pair_landmark", "P", "R", "center", "K")


def same_stages(got, want, what=""):
    for f in STAGE_FIELDS:
        assert (f in got) == (f in want), (what, f)
        if f in want:
            np.testing.assert_array_equal(got[f], want[f], err_msg=f"{what}: {f}")


def compare_guided(m, q, dm, view_sel=None, exp=None, **okw):
    """One query through the staged calls with guided matching on, every stage against the oracle: putative_read;
    geometric_read_pairs' counts and both lists per surviving view; geometric_read raises; match_set_read's features,
    landmarks and point bits; the resection's iterations, inlier indices, pairs and the bits of P, R, centre and K."""
    if exp is None:
        exp = opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), view_sel=view_sel, guided=True, **okw)
    got = forms.stages(dm, m, q, view_sel, read_must_raise=True)
    assert got["read_raised"]
    same_stages(got, forms.oracle_stages(m, exp), f"nq {len(q.desc)}")
    return exp, got


def compare_scene(name, oracle_c):
    s = G.scene(name)
    exps = G.expected(name, opipe.localize)
    out = []
    with forms.device_map(s.m, **s.params) as dm:
        for k, q in enumerate(s.queries):
            out.append(compare_guided(s.m, q, dm, s.sel(k), exp=exps[k]))
    return s, out


def compare_view_candidates(dm, m, q, v, cap=4096, **okw):
    """K4 for ONE view, seen through the shard export: every candidate of the view that wins its query feature inside the
    view, with its order key -- the descriptor distance of the LAST putative match with that query feature, the view
    id and the position in the guided list -- against oracle.pipeline.shard_candidates(guided=True)."""
    import torch
    from sfmlocalization_amd import dist as D
    part = torch.zeros(D.part_bytes(cap), dtype=torch.uint8, device="cuda")
    dq = dm.query(q.desc, q.kpt_xy, q.width, q.height)
    c = dm.context()
    c.shard_begin(dq, np.array([v], np.uint32))
    c.shard_export(part.data_ptr(), cap)
    c.sync()
    c.close()
    dq.close()
    want = D.reduce_candidates(opipe.shard_candidates(m, q.desc, q.kpt_xy, (q.width, q.height), v, v + 1, guided=True, **okw))
    got = np.sort(D.unpack_part(part.cpu().numpy(), cap), order="order")
    want = np.sort(want, order="order")
    assert len(got) == len(want) > 0, (v, len(got), len(want))
    for f in ("order", "qfeat", "landmark_id", "X"):
        np.testing.assert_array_equal(got[f], want[f], err_msg=f"view {v}: {f}")
    return got


def test_tile_edges(oracle_c):
    """kGTile = 512 query positions per LDS tile: nq below one tile (40, 511), exactly one (512), one more (513), exactly
    two (1 024), one more (1 025)."""
    s, out = compare_scene("tile_edges", oracle_c)
    assert all(exp["geo_count"].sum() > 0 for exp, _ in out)
    assert sum(exp["ok"] for exp, _ in out) >= 5


def test_ragged_views(oracle_c):
    """views of 350 .. 700 rows: blockIdx.y up to 2 in k_guided_rows, views that end inside a 64-lane step of
    k_guided_compact, a view without rows"""
    s, out = compare_scene("ragged", oracle_c)
    assert all(exp["ok"] for exp, _ in out)


def test_shortlist(oracle_c):
    """the view_sel form of k_guided_rows / k_guided_compact / K4: match_putative with a strict subset of the views"""
    s, out = compare_scene("shortlist", oracle_c)
    for k, (exp, got) in enumerate(out):
        outside = np.setdiff1d(np.arange(s.m.n_views), s.sel(k))
        assert got["geo_count"][outside].sum() == 0 and got["geo_count"].sum() > 0


def test_context_reuse(oracle_c):
    """d_guided_row and d_geo_j are a context's own and never cleared: 1 025 features on the whole map, 40 features on a
    shortlist of the same place, the first again -- on the map's one context.  The three are the oracle's, and the third is
    the first, byte for byte."""
    s, out = compare_scene("reuse", oracle_c)
    first, third = out[0][1], out[2][1]
    assert sorted(first) == sorted(third)
    for f in first:
        assert np.asarray(first[f]).tobytes() == np.asarray(third[f]).tobytes(), f
    assert 0 < out[1][1]["geo_count"].sum() < first["geo_count"].sum()


def test_selection_rule_edges(oracle_c):
    """best == second (rejected, a best of 0 included), best == 0 < second (accepted), one candidate in the band, none:
    counted on this scene by test_guided_cases_cpu.py::test_ties.  A candidate that ties the best must still become the
    second best (dropping that is caught here); whether it also REPLACES the best (`d <= bd` for `d < bd`) changes no
    row's result and cannot be seen: test_guided_cases_cpu.py::test_a_tie_at_the_best_distance_never_decides_a_row."""
    s, out = compare_scene("ties", oracle_c)
    assert out[0][0]["geo_count"].sum() > 100


def test_k4_backward_walk_in_lds(oracle_c):
    """put_count in [16, 127]; guided matches without a featDist entry (kNoDist) and query features twice in a view's
    putative list; a view's own candidates with their order keys"""
    s, out = compare_scene("k4_walk", oracle_c)
    with forms.device_map(s.m, **s.params) as dm:
        for q, (exp, _) in zip(s.queries, out):
            v = max(G.surviving(exp), key=lambda w: G.no_dist_matches(s.m, exp, w))
            compare_view_candidates(dm, s.m, q, v, **s.params)


@pytest.mark.parametrize("name", ["k4_hash_big", "k4_hash_huge"])
def test_k4_hash_table_and_k3_register_forms(oracle_c, name):
    """put_count in [513, 1 024] (k4_hash_big) and [1 025, 2 048] (k4_hash_huge), three queries in a row on one map: the
    first meets K3's block-wide LDS form, the following ones -- the map's credit -- the register forms
    k_fmatrix_fast<W, 1024> and <4, 2048, wide>; each writes the F and errorMax of the band.  K4 looks "the last putative
    match with this query feature" up in its hash table; query features occur twice in a view's list."""
    s, out = compare_scene(name, oracle_c)
    assert all(exp["ok"] for exp, _ in out)
    with forms.device_map(s.m, **s.params) as dm:
        exp = out[0][0]
        v = max(G.surviving(exp), key=lambda w: len(G.twice_in_putative(s.m, exp, w)))
        compare_view_candidates(dm, s.m, s.queries[0], v, **s.params)


def test_k4_walk_in_global_memory_and_k3_global_store_form(oracle_c):
    """a view of more than kFMaxM = 2 048 putative matches: K3's global-store form writes the band's model, K4 walks the
    putative list in global memory (staged == false) -- from its LAST entry, which here is the only one with its query
    feature and is asked for by a guided match"""
    s, out = compare_scene("k4_global", oracle_c)
    exp = out[0][0]
    assert exp["put_count"].max() > 2048 and exp["ok"]
    with forms.device_map(s.m, **s.params) as dm:
        for v in G.surviving(exp):
            if exp["put_count"][v] > 2048:
                compare_view_candidates(dm, s.m, s.queries[0], v, **s.params)


def test_radial_intrinsic(oracle_c):
    s, out = compare_scene("radial", oracle_c)
    assert out[0][0]["ok"] and len(s.m.intrinsic) == 6


K3_SETTINGS = {
    "default": {},
    "wide forced": {"SFMLOC_K3_WIDE": "2", "SFMLOC_K3_WIDE_2048": "2"},
    "wide off": {"SFMLOC_K3_WIDE": "0", "SFMLOC_K3_WIDE_2048": "0"},
    "big forced": {"SFMLOC_K3_BIG": "2"},
    "big off": {"SFMLOC_K3_BIG": "0"},
    "wide tail on eight waves": {"SFMLOC_K3_WIDE_WAVES": "8"},
    "four waves per view": {"SFMLOC_K3_WAVES_ALONE": "4", "SFMLOC_K3_WAVES_SHARED": "4"},
}
K3_KNOBS = sorted({k for v in K3_SETTINGS.values() for k in v})


def test_every_k3_form_writes_the_same_band(oracle_c):
    """errorMax is read from the last entry of K3's sorted inlier list, which comes from a wave's segment, from
    take_inliers or from a rebuild, depending on the form: with a list in any other order the inlier SET is the same and
    only the guided band moves.  The form scenes (tile_edges at nq = 513, k4_hash_big, k4_hash_huge, k4_global) under
    every setting of the form knobs, each in a child process (the library reads them once), at most three at a time:
    guided lists, 2D-3D set and pose bits equal the oracle's record, and hence each other's."""
    want = {}
    for name in G.FORM_SCENES:
        s, exps = G.scene(name), G.expected(name, opipe.localize)
        want[name] = [json.loads(json.dumps(forms.jsonable(forms.oracle_stages(s.m, exps[k])))) for k in G.form_queries(name)]
    names = list(K3_SETTINGS)
    got = {}
    for b in range(0, len(names), 3):
        children = {}
        for n in names[b:b + 3]:
            env = {k: v for k, v in os.environ.items() if k not in K3_KNOBS}
            env.update(K3_SETTINGS[n])
            children[n] = subprocess.Popen([sys.executable, TOOL], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
        for n, p in children.items():
            try:
                o, e = p.communicate(timeout=300)
            except subprocess.TimeoutExpired:
                for c in children.values():
                    c.kill()
                raise
            assert p.returncode == 0, (n, o[-2000:] + e[-2000:])
            got[n] = json.loads(o.strip().splitlines()[-1])
    for n in names:
        assert sorted(got[n]) == sorted(want)
        for name in want:
            assert len(got[n][name]) == len(want[name])
            for k, (g, w) in enumerate(zip(got[n][name], want[name])):
                for f in forms.FORM_FIELDS:
                    assert g.get(f) == w.get(f), f"{n}: {name}, query {k}: {f}"


def test_sharded_export_and_merge(oracle_c):
    """Two shards of the ragged map on one GPU, guided matching on in all three maps: a shard's exported part is the
    oracle's (guided candidates carry the guided list's positions in their order keys and drop the matches without a
    featDist entry), the merged pose is the unsharded one."""
    import torch
    from sfmlocalization_amd import dist as D
    s = G.scene("ragged")
    m = s.m
    cap = 4096
    full = forms.device_map(m, **s.params)
    ranges = D.shard_views(m.view_off, 2)
    shards = []
    for v0, v1 in ranges:
        r0, r1 = int(m.view_off[v0]), int(m.view_off[v1])
        shards.append(S.Map(m.view_id[v0:v1], m.view_off[v0:v1 + 1] - m.view_off[v0], m.desc[r0:r1],
                            params=S.default_params(guided_matching=1, **s.params), view_wh=m.view_wh[v0:v1],
                            kpt_xy=m.kpt_xy[r0:r1], row_landmark=m.row_landmark[r0:r1], landmark_id=m.landmark_id,
                            landmark_X=m.landmark_X, intrinsic=m.intrinsic))
    pb = D.part_bytes(cap)
    n_cand = 0
    for k, q in enumerate(s.queries):
        exp = G.expected("ragged", opipe.localize)[k]
        fq = full.query(q.desc, q.kpt_xy, q.width, q.height)
        ref = full.localize(fq)
        parts = torch.zeros((2, pb), dtype=torch.uint8, device="cuda")
        qs = []
        for sh, sm in enumerate(shards):
            sq = sm.query(q.desc, q.kpt_xy, q.width, q.height)
            qs.append(sq)
            c = sm.context()
            c.shard_begin(sq)
            c.shard_export(parts.data_ptr() + sh * pb, cap)
            c.sync()
            c.close()
            v0, v1 = ranges[sh]
            exp_c = D.reduce_candidates(opipe.shard_candidates(m, q.desc, q.kpt_xy, (q.width, q.height), v0, v1, guided=True,
                                                               **s.params))
            got_c = D.unpack_part(parts[sh].cpu().numpy(), cap)
            assert len(np.unique(got_c["qfeat"])) == len(got_c)
            got_c, exp_c = np.sort(got_c, order="order"), np.sort(exp_c, order="order")   # arrival order is free
            assert len(got_c) == len(exp_c)
            for f in ("order", "qfeat", "landmark_id", "X"):
                np.testing.assert_array_equal(got_c[f], exp_c[f], err_msg=f)
            n_cand += len(got_c)
        c = shards[1].context()
        c.merge_begin(qs[1], parts.data_ptr(), 2, cap)
        pose, pq, pl = c.end()
        c.close()
        assert exp["ok"] and bool(pose.ok) and bool(ref[0].ok) and pose.n_inliers == ref[0].n_inliers == exp["n_inliers"]
        for a in ((pq, pl, pose), (ref[1], ref[2], ref[0])):
            np.testing.assert_array_equal(a[0], exp["pair_qfeat"])
            np.testing.assert_array_equal(a[1], exp["pair_landmark"])
            np.testing.assert_array_equal(bits(np.array(a[2].P)), bits(exp["P"].ravel()))
            np.testing.assert_array_equal(bits(np.array(a[2].center)), bits(exp["center"]))
        for sq in qs:
            sq.close()
        fq.close()
    assert n_cand > 200
    for sm in shards:
        sm.close()
    full.close()


def test_gang_session(oracle_c):
    """four tile_edges queries (nq = 40, 512, 513, 1 025) in one gang session -- one launch per kernel for the four, a
    member's guided rows and lists its own: the same queries one at a time, and the oracle's"""
    s, exps = G.scene("tile_edges"), G.expected("tile_edges", opipe.localize)
    pick = [G.TILE_NQ.index(n) for n in (40, 512, 513, 1025)]
    with forms.device_map(s.m, **s.params) as dm:
        dqs = [dm.query(s.queries[k].desc, s.queries[k].kpt_xy, s.queries[k].width, s.queries[k].height) for k in pick]
        ref = [dm.localize(dq) for dq in dqs]
        lead = dm.context()
        ctxs = [lead] + [dm.context(share=lead) for _ in range(3)]
        with capi.gang(ctxs):
            for c, dq in zip(ctxs, dqs):
                c.begin(dq)
        got = [c.end() for c in ctxs]
        launches, ganged = capi.gang_counters(lead)
        assert ganged >= 4                                     # the chain, guided kernels included, went out as gang launches
        for k, g, r in zip(pick, got, ref):
            e = exps[k]
            for pose, pq, pl in (g, r):
                assert bool(pose.ok) == e["ok"] and pose.n_matches_2d3d == len(e["ms_qfeat"])
                assert pose.n_geometric_views == int((e["geo_count"] > 0).sum())
                if e["ok"]:
                    assert pose.n_inliers == e["n_inliers"]
                    np.testing.assert_array_equal(pq, e["pair_qfeat"])
                    np.testing.assert_array_equal(pl, e["pair_landmark"])
                    np.testing.assert_array_equal(bits(np.array(pose.P)), bits(e["P"].ravel()))
                    np.testing.assert_array_equal(bits(np.array(pose.center)), bits(e["center"]))
            assert capi.result_fingerprint(*g) == capi.result_fingerprint(*r)
        for c in ctxs[1:] + [lead]:
            c.close()
        for dq in dqs:
            dq.close()


def test_pair_path(oracle_c):
    """sfmloc_geometric_pairs with guided matching on two images of 2 100 features: more than one y-block of
    k_guided_rows on the first image's side, more than kGTile on the second's; against oracle.pipeline.geometric_match
    (guided=True)"""
    m = G.pair_images(G.SEEDS["pair_images"])
    off = m.view_off.astype(np.int64)
    kp = synth.round6(m.kpt_xy)
    descs = [m.desc[off[v]:off[v + 1]] for v in range(2)]
    p = S.default_params(ransac_round=25, geom_precision=4.0, guided_matching=1)
    with S.Map(m.view_id, m.view_off, m.desc, params=p, view_wh=m.view_wh, kpt_xy=kp) as dm:
        put = dm.match_pairs([(0, 1)])
        got = dm.geometric_pairs(put)
    assert list(put) == [(0, 1)] and len(put[(0, 1)][0]) > 512
    exp = opipe.geometric_match([kp[off[v]:off[v + 1]] for v in range(2)], m.view_wh, m.view_id, put, ransac_round=25,
                                guided=True, descs=descs)
    plain = opipe.geometric_match([kp[off[v]:off[v + 1]] for v in range(2)], m.view_wh, m.view_id, put, ransac_round=25)
    assert list(got) == list(exp) == [(0, 1)]
    np.testing.assert_array_equal(got[(0, 1)][0], exp[(0, 1)][0])
    np.testing.assert_array_equal(got[(0, 1)][1], exp[(0, 1)][1])
    assert (np.diff(got[(0, 1)][0].astype(np.int64)) > 0).all() and len(got[(0, 1)][0]) > 512
    assert got[(0, 1)][0].max() >= 512 and got[(0, 1)][1].max() >= 1024          # rows of a later block, positions of a later tile
    assert not np.array_equal(np.sort(plain[(0, 1)][0]), got[(0, 1)][0])          # guided matching changed the list
