"""The scenes of the guided-matching tests (tests/guided_cases.py) are what they are for -- asserted on the oracle's side,
without a GPU.  A scene that misses its property gets another seed in guided_cases.SEEDS; the property stays.

For every scene and every view that passes the F-matrix filter the C oracle's guided list is held against the NumPy twin
(oracle/twins_np.py guided_match) on ALL rows.  One pair per view cannot be kept away from the band's threshold by any
seed: errorMax is the residual of AC-RANSAC's last inlier, so that inlier's own (row, query feature) pair has an epipolar
error EQUAL to the threshold, and which side of the strict `<` it falls on is the rounding of the route taken (normalised
frame against pixels; measured 1e-16 .. 2e-13 relative, where every other pair stays 4e-7 or more away).  The test
therefore asserts
  - that pair is the threshold's own (within 1e-9 of it) and NO other pair lies within 1e-9 relative of the threshold;
  - the C oracle's list equals the twin's with that one pair inside the band, or the twin's with it outside (the twin run
    at errorMax (1 +- 1e-11), which moves no other pair across), on every row -- none is left out.
The device and the C oracle take the same route, so between those two the pair is compared bit for bit like any other."""
import numpy as np
import pytest

import guided_cases as G
from oracle import pipeline as opipe
from oracle import twins_np as T

MARGIN = 1e-9
OWN_SCENES = ("tile_edges", "ragged", "ties", "k4_walk", "k4_hash_big", "k4_hash_huge", "k4_global")
DERIVED = {"radial": "tile_edges", "shortlist": "ragged", "reuse": "tile_edges"}     # same map: same F per view


@pytest.fixture(scope="module")
def exp(oracle_c):
    return lambda name: G.expected(name, opipe.localize)


def views(name, exp):
    s = G.scene(name)
    for k, (q, e) in enumerate(zip(s.queries, exp(name))):
        for v in G.surviving(e):
            yield s, k, q, e, v


def test_every_scene_is_listed():
    assert sorted(G.SCENES) == sorted(OWN_SCENES + tuple(DERIVED))


@pytest.mark.parametrize("name", OWN_SCENES)
def test_c_oracle_equals_numpy_twin_on_every_surviving_view(exp, name):
    n_views = n_flipped = 0
    for s, k, q, e, v in views(name, exp):
        b = G.band_stats(s.m, q, e, v)
        what = f"{name}, query {k}, view {v}"
        assert b["margin_defining"] < MARGIN, (what, b["margin_defining"])
        assert b["margin_others"] >= MARGIN, (what, b["margin_others"])
        off, end = int(s.m.view_off[v]), int(s.m.view_off[v + 1])
        st = e["f_stats"][v]
        args = (tuple(int(t) for t in s.m.view_wh[v]), (q.width, q.height), s.m.kpt_xy[off:end], s.m.desc[off:end],
                opipe.round6(q.kpt_xy), q.desc)
        ci, cj = G.guided_lists(s.m, e, v)
        twin = [T.guided_match(st["F"], st["errmax"] * f, *args) for f in (1.0 + 1e-11, 1.0 - 1e-11)]   # pair in / out
        same = [np.array_equal(ci, ti) and np.array_equal(cj, tj) for ti, tj in twin]
        assert any(same), what
        # the two twin runs differ in nothing but the row of the threshold's own pair
        rows = set(map(int, twin[0][0])) ^ set(map(int, twin[1][0]))
        both = np.intersect1d(twin[0][0], twin[1][0])
        ja = dict(zip(map(int, twin[0][0]), map(int, twin[0][1])))
        jb = dict(zip(map(int, twin[1][0]), map(int, twin[1][1])))
        rows |= {int(i) for i in both if ja[int(i)] != jb[int(i)]}
        assert rows <= {b["defining_pair"][0]}, (what, rows, b["defining_pair"])
        n_views += 1
        n_flipped += int(not all(same))
    print(f"{name}: {n_views} surviving views, all rows compared; the threshold's own pair decides a row in {n_flipped}")
    assert n_views >= 1


@pytest.mark.parametrize("name", sorted(DERIVED))
def test_derived_scenes_have_their_parents_models(exp, name):
    """radial / shortlist / reuse run on a parent scene's map: a view's F and errorMax do not depend on the intrinsic or
    on which other views are searched, so the comparison above covers their guided lists."""
    s, p = G.scene(name), G.scene(DERIVED[name])
    pq = {id_: k for k, id_ in enumerate(q.desc.tobytes() for q in p.queries)}
    n = 0
    for k, (q, e) in enumerate(zip(s.queries, exp(name))):
        if q.desc.tobytes() not in pq:
            continue                                    # (reuse's 40-feature query is its own: checked below)
        pe = exp(DERIVED[name])[pq[q.desc.tobytes()]]
        for v in G.surviving(e):
            assert np.array_equal(e["f_stats"][v]["F"], pe["f_stats"][v]["F"]) and e["f_stats"][v]["errmax"] == pe["f_stats"][v]["errmax"]
            a, c = G.guided_lists(s.m, e, v), G.guided_lists(p.m, pe, v)
            assert np.array_equal(a[0], c[0]) and np.array_equal(a[1], c[1])
            n += 1
    assert n >= 1


def test_tile_edges(exp):
    s, es = G.scene("tile_edges"), exp("tile_edges")
    assert tuple(len(q.desc) for q in s.queries) == G.TILE_NQ == (40, 511, 512, 513, 1024, 1025)
    assert all(int(o) == 400 * v for v, o in enumerate(s.m.view_off)) and s.m.n_views == 40
    for q, e in zip(s.queries, es):
        sv = G.surviving(e)
        assert len(sv) >= 1, len(q.desc)
        assert all(e["put_count"][v] >= 16 for v in sv)                 # (nq = 40 included: min_putative is met)
        assert sum(int(e["geo_count"][v]) for v in sv) >= 1
        if len(q.desc) > 40:        # the last position -- alone in its LDS tile at nq = 513 and 1 025 -- is one guided matches name
            assert sum(int((G.guided_lists(s.m, e, v)[1] == len(q.desc) - 1).sum()) for v in sv) >= 1, len(q.desc)


def test_ragged(exp):
    s, es = G.scene("ragged"), exp("ragged")
    sizes = np.diff(s.m.view_off.astype(np.int64))
    assert sizes.min() == 0 and sizes.max() <= 700 and sizes[sizes > 0].min() >= 350
    sv = sorted({v for e in es for v in G.surviving(e)})
    assert any(sizes[v] % 64 != 0 for v in sv) and any(sizes[v] % 256 != 0 for v in sv) and any(sizes[v] > 512 for v in sv)
    # (for the sharded export: both of K4's special cases occur in either half of the map)
    assert all(sum(G.no_dist_matches(s.m, e, v) for v in G.surviving(e)) >= 1 for e in es)
    assert all(sum(len(G.twice_in_putative(s.m, e, v)) for v in G.surviving(e)) >= 1 for e in es)


def test_shortlist(exp):
    s, es, whole = G.scene("shortlist"), exp("shortlist"), exp("ragged")
    for k, (e, w) in enumerate(zip(es, whole)):
        sel = s.sel(k)
        assert (np.diff(sel.astype(np.int64)) > 0).all() and len(sel) < s.m.n_views
        assert any(s.m.view_off[v + 1] == s.m.view_off[v] for v in sel)       # (the view without rows is on the list)
        sv, wv = G.surviving(e), G.surviving(w)
        assert sv and set(sv) <= set(int(v) for v in sel)
        assert any(int(v) not in sv for v in sel)                       # views of the list that fail
        assert any(v not in set(int(x) for x in sel) for v in wv)       # a view outside it would have survived
        assert sv == [v for v in wv if v in set(int(x) for x in sel)]


def test_reuse(exp):
    s, es = G.scene("reuse"), exp("reuse")
    assert [len(q.desc) for q in s.queries] == [1025, 40, 1025] and s.queries[0] is s.queries[2]
    assert s.sels[0] is None and s.sels[2] is None and len(s.sels[1]) < s.m.n_views
    first, second = set(G.surviving(es[0])), set(G.surviving(es[1]))
    sel = set(int(v) for v in s.sels[1])
    assert second and second <= first & sel          # views the first query left lists in get shorter ones ...
    assert all(es[1]["geo_count"][v] < es[0]["geo_count"][v] for v in second)
    assert (first & sel) - second                    # ... or none at all, and only geo_count says so
    assert first - sel                               # ... and views the second query does not visit keep theirs


def test_ties(exp):
    s, e = G.scene("ties"), exp("ties")[0]
    tie = zero = one = none = 0
    for v in G.surviving(e):
        b = G.band_stats(s.m, s.queries[0], e, v)
        two = b["n_band"] >= 2
        tie += int((two & (b["best"] == b["second"])).sum())
        zero += int((two & (b["best"] == 0) & (b["second"] > 0)).sum())
        one += int((b["n_band"] == 1).sum())
        none += int((b["n_band"] == 0).sum())
        # what the rule makes of them, on the oracle's list (but for the row of the threshold's own pair, whose band
        # the two routes may count differently: module docstring)
        gi, _ = G.guided_lists(s.m, e, v)
        got = np.zeros(len(b["best"]), bool)
        got[gi.astype(np.int64)] = True
        rest = np.ones(len(got), bool)
        rest[b["defining_pair"][0]] = False
        assert not got[rest & two & (b["best"] == b["second"])].any() and not got[rest & ~two].any()
        assert got[rest & two & (b["best"] == 0) & (b["second"] > 0)].all()
    print(f"ties: best == second {tie}, best == 0 < second {zero}, one candidate {one}, none {none}")
    assert tie >= 20 and zero >= 20 and one >= 1 and none >= 1


def test_k4_walk(exp):
    s, es = G.scene("k4_walk"), exp("k4_walk")
    for e in es:
        sv = G.surviving(e)
        assert sv and all(16 <= e["put_count"][v] <= 127 for v in sv)
        n_nodist = sum(G.no_dist_matches(s.m, e, v) for v in sv)
        n_landmark_rows = sum(int((s.m.row_landmark[int(s.m.view_off[v]) + G.guided_lists(s.m, e, v)[0].astype(np.int64)] >= 0).sum())
                              for v in sv)
        assert n_nodist >= 1 and len(e["ms_qfeat"]) < n_landmark_rows
        assert sum(len(G.twice_in_putative(s.m, e, v)) for v in sv) >= 1


@pytest.mark.parametrize("name,lo,hi", [("k4_hash_big", 513, 1024), ("k4_hash_huge", 1025, 2048)])
def test_k4_hash(exp, name, lo, hi):
    s, es = G.scene(name), exp(name)
    assert len(es) >= 3                                     # several queries in a row: the credit changes K3's form
    for e in es:
        sv = G.surviving(e)
        assert sv and all(lo <= e["put_count"][v] <= hi for v in sv) and e["ok"]
        assert sum(len(G.twice_in_putative(s.m, e, v)) for v in sv) >= 1
        assert sum(G.no_dist_matches(s.m, e, v) for v in sv) >= 1


def test_k4_global(exp):
    s, e = G.scene("k4_global"), exp("k4_global")[0]
    v = int(np.argmax(e["put_count"]))
    assert e["put_count"][v] > 2048 and v in G.surviving(e) and e["geo_count"][v] > 0
    assert np.diff(s.m.view_off.astype(np.int64)).tolist() == [2600] * 3 and len(s.queries[0].desc) == 2700
    # the walk in global memory starts at the LAST putative match: in some view that takes it, the last one is the only
    # one with its query feature, and a guided match at a row with a landmark asks for it
    found = 0
    for w in G.surviving(e):
        off, c = int(s.m.view_off[w]), int(e["put_count"][w])
        if c <= 2048:
            continue
        last_j = int(e["put_j"][off + c - 1])
        gi, gj = G.guided_lists(s.m, e, w)
        found += int((e["put_j"][off:off + c] == last_j).sum() == 1 and
                     any(s.m.row_landmark[off + int(i)] >= 0 for i in gi[gj == last_j]))
    assert found >= 1
    assert G.no_dist_matches(s.m, e, v) >= 1 and len(G.twice_in_putative(s.m, e, v)) >= 1


def test_guided_shard_candidates_against_a_brute_force_restatement(exp):
    """oracle.pipeline.shard_candidates(guided=True): (geo_idx, geo_j) are the match itself, and a match whose query
    feature no putative match of the view has is skipped.  Restated here from the oracle's lists with plain loops."""
    from sfmlocalization_amd import dist as D
    s, es = G.scene("ragged"), exp("ragged")
    m = s.m
    total = skipped = 0
    for (v0, v1) in D.shard_views(m.view_off, 2):
        for q, e in zip(s.queries, es):
            want = []
            n_skipped = 0
            for v in range(v0, v1):
                off = int(m.view_off[v])
                last = {}
                for p in range(int(e["put_count"][v])):
                    last[int(e["put_j"][off + p])] = int(e["put_d"][off + p])          # the later entry replaces
                gi, gj = G.guided_lists(m, e, v)
                for p, (i, j) in enumerate(zip(gi, gj)):
                    lm = int(m.row_landmark[off + int(i)])
                    if lm < 0:
                        continue
                    if int(j) not in last:
                        n_skipped += 1
                        continue
                    key = (last[int(j)] << 48) | ((int(m.view_id[v]) & 0xFFFFFF) << 24) | p
                    want.append((key, int(j), int(m.landmark_id[lm]), tuple(m.landmark_X[lm])))
            want = np.array(want, dtype=D.CANDIDATE_DTYPE)
            got = opipe.shard_candidates(m, q.desc, q.kpt_xy, (q.width, q.height), v0, v1, guided=True, **s.params)
            assert len(got) == len(want)
            total += len(want)
            skipped += n_skipped
            for f in ("order", "qfeat", "landmark_id", "X"):
                np.testing.assert_array_equal(got[f], want[f], err_msg=f)
            # the unguided function is untouched: it still reads geo_idx as positions in the putative list
            plain = opipe.shard_candidates(m, q.desc, q.kpt_xy, (q.width, q.height), v0, v1, **s.params)
            pe = opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), view_sel=np.arange(v0, v1, dtype=np.uint32), **s.params)
            n_plain = sum(int((m.row_landmark[int(m.view_off[v]) + pe["put_i"][int(m.view_off[v]) + pe["geo_idx"][int(m.view_off[v]):int(m.view_off[v]) + int(pe["geo_count"][v])].astype(np.int64)].astype(np.int64)] >= 0).sum())
                          for v in range(v0, v1))
            assert len(plain) == n_plain
    assert total > 100 and skipped >= 2         # (a query's place lies in one half of the map: its other half is empty)


def test_a_tie_at_the_best_distance_never_decides_a_row():
    """k_guided_rows scans a row's candidates with `d < bd` / `d < sbd`.  Whether a candidate that TIES the best replaces
    it (`d <= bd`) cannot change a row's result: after a tie best == second, and a row is kept only if
    best^2 < 0.36 second^2 -- never with best == second, 0 included -- while a later, strictly better candidate replaces
    the index either way.  So the scan's `<` against `<=` at the best is not something a comparison with the oracle can
    see (the ties scene checks what it CAN: that such rows are rejected, and that a tie still counts as the second best).
    Shown here exhaustively for every sequence of up to six distances out of {0, 1, 2, 3, 5, 9}."""
    import itertools

    def scan(ds, tie_replaces):
        bd = sbd = G.NO_DIST
        idx = -1
        for j, d in enumerate(ds):
            if d < bd or (tie_replaces and d == bd):
                idx, sbd, bd = j, bd, d
            elif d < sbd:
                sbd = d
        ok = sbd != G.NO_DIST and bd * bd < 0.36 * (sbd * sbd)
        return idx if ok else None

    n = 0
    for k in range(7):
        for ds in itertools.product((0, 1, 2, 3, 5, 9), repeat=k):
            assert scan(ds, False) == scan(ds, True), ds
            n += 1
    assert n > 50000
