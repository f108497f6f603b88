"""CPU: the scenes of tests/k3_cases.py are what their contents claim -- conditions on the INPUTS, checked against the C
oracle alone (oracle_c.fmatrix_filter, the call oracle.pipeline.geometric_match makes per pair), so that no change of a
kernel can make a case stop testing what it is for.  test_gpu_k3_forms.py runs the same scenes through every launch
form of K3."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k3_cases as KC  # noqa: E402


def normalised(x, wh):
    """NormalizePoints(x, w, h) in the oracle's operation order"""
    s = 1.0 / np.sqrt(float(wh[0] * wh[1]))
    x = np.asarray(x, np.float64)
    return np.stack([s * x[:, 0] + (-0.5 * float(wh[0]) * s), s * x[:, 1] + (-0.5 * float(wh[1]) * s)], 1)


def err_fmatrix(F, a, b):
    """err_fmatrix (geom_device.h) = kernel_error's EpipolarDistanceError: the squared distance of b to the line F a, on
    normalised points, in the same operation order; NaN -> +inf"""
    M = np.asarray(F, np.float64).reshape(9)
    x, y, u, v = a[:, 0], a[:, 1], b[:, 0], b[:, 1]
    with np.errstate(all="ignore"):
        l0 = (M[0] * x + M[1] * y) + M[2]
        l1 = (M[3] * x + M[4] * y) + M[5]
        l2 = (M[6] * x + M[7] * y) + M[8]
        num = (l0 * u + l1 * v) + l2
        e = (num * num) / (l0 * l0 + l1 * l1)
    e[np.isnan(e)] = np.inf
    return e


def filter_pair(oracle_c, sc, k, budget=None):
    """the oracle's record of pair k of a scene, and the pair's normalised points in list order"""
    N = len(sc.sizes)
    mi, mj = sc.matches[(k, N)]
    kp = KC.view_kpts(sc)
    x1, x2 = kp[k].astype(np.float64)[mi.astype(np.int64)], kp[N].astype(np.float64)[mj.astype(np.int64)]
    r = oracle_c.fmatrix_filter(x1, KC.WH1, x2, KC.WH2, KC.GEOM_PRECISION, sc.budget if budget is None else budget, KC.SEED,
                                stream=int(sc.view_id[k]))
    return r, normalised(x1, KC.WH1), normalised(x2, KC.WH2)


def test_the_scenes():
    """every scene has one pair per size with exactly that many matches, first images of exactly that many rows (three
    times as many in `shuffled`), one second image that is the concatenation of the pairs' slices, two non-square image
    sizes, ascending view ids from 0 to the ABI's largest"""
    assert KC.SIZES == (7, 8, 17, 18, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048,
                        2049, 4097)
    assert KC.BUDGETS["clean"] == (25, 2, 3, 36, 4096) and all(b == (25,) for c, b in KC.BUDGETS.items() if c != "clean")
    assert KC.WH1 != KC.WH2 and KC.WH1[0] != KC.WH1[1] and KC.WH2[0] != KC.WH2[1]
    for content, budget in KC.all_scenes():
        sc = KC.scene(content, budget)
        N = len(sc.sizes)
        assert sc.sizes == (KC.SIZES if budget < 4096 else tuple(s for s in KC.SIZES if s <= 512))
        assert sc.view_id[0] == 0 and sc.view_id[N - 1] == (1 << 24) - 2 and sc.view_id[N] == (1 << 24) - 1
        assert np.all(np.diff(sc.view_id.astype(np.int64)) > 0)
        rows = np.diff(sc.view_off.astype(np.int64))
        assert rows[N] == sum(sc.sizes) < 65536 and len(sc.kpt) == sc.view_off[-1] == len(sc.desc)
        assert np.isfinite(sc.kpt).all() and sc.kpt.dtype == np.float32
        lo = 0
        for k, m in enumerate(sc.sizes):
            mi, mj = sc.matches[(k, N)]
            assert len(mi) == len(mj) == m and rows[k] == (3 * m if content == "shuffled" else m)
            assert mi.max() < rows[k] and len(np.unique(mi)) == m
            assert sorted(mj.tolist()) == list(range(lo, lo + m))         # its own slice, every row once
            if content == "shuffled" and m > 8:
                assert not np.array_equal(mi, np.arange(m)) and not np.array_equal(mj, np.arange(lo, lo + m))
            lo += m


def test_tie_groups_lie_where_the_content_says():
    """`ties`: groups of 2 .. 8 distinct rows with bit-equal keypoints in both images, one across list positions 63|64,
    255|256, 511|512 and 1 023|1 024 wherever the list holds them, one at the very end"""
    sc = KC.scene("ties", 25)
    N = len(sc.sizes)
    kp = KC.view_kpts(sc)
    sizes_seen = set()
    for k, m in enumerate(sc.sizes):
        groups = KC.pair("ties", m, 25, int(sc.view_id[k])).groups
        assert groups == KC.tie_groups(m)
        mi, mj = (a.astype(np.int64) for a in sc.matches[(k, N)])
        for b in KC.BOUNDARIES:
            assert (m > b) == any(b - 1 in g and b in g for g in groups), (m, b)
        if m >= 8:
            assert any(g[-1] == m - 1 for g in groups), m
        for g in groups:
            g = list(g)
            sizes_seen.add(len(g))
            assert 2 <= len(g) <= 8 and len(set(mi[g])) == len(g) and len(set(mj[g])) == len(g)
            assert len({kp[k][mi[p]].tobytes() for p in g}) == 1 and len({kp[N][mj[p]].tobytes() for p in g}) == 1
    assert sizes_seen >= {2, 3, 4, 5, 8}


@pytest.mark.parametrize("budget", KC.BUDGETS["clean"])
def test_clean_keeps_every_match(oracle_c, budget):
    """n == m from 18 matches on, nothing at 17 and below (the "> 2.5 * 7 inliers" rule; 7 does not run)"""
    sc = KC.scene("clean", budget)
    for k, m in enumerate(sc.sizes):
        r, _, _ = filter_pair(oracle_c, sc, k)
        assert r["n"] == (m if m >= 18 else 0), (m, budget, r["n"])
    exp = KC.expectations(oracle_c, "clean", budget)
    assert sorted(exp) == [(k, len(sc.sizes)) for k, m in enumerate(sc.sizes) if m >= 18]


def test_shuffled_keeps_every_match(oracle_c):
    sc = KC.scene("shuffled", 25)
    for k, m in enumerate(sc.sizes):
        assert filter_pair(oracle_c, sc, k)[0]["n"] == (m if m >= 18 else 0), m


def test_outliers100_drops_every_pair(oracle_c):
    sc = KC.scene("outliers100", 25)
    for k, m in enumerate(sc.sizes):
        r, _, _ = filter_pair(oracle_c, sc, k)
        assert r["n"] == 0, m
        assert r["iters"] == (25 if m > 7 else 0), (m, r["iters"])      # the whole budget, reserve included
    assert KC.expectations(oracle_c, "outliers100", 25) == {}


def test_outliers30_survives(oracle_c):
    """from 63 matches on the pair survives with most of its 70 % inliers (AC-RANSAC may cut the worst few of a model that
    seven of them gave) and no more than the list"""
    sc = KC.scene("outliers30", 25)
    got = []
    for k, m in enumerate(sc.sizes):
        n = filter_pair(oracle_c, sc, k)[0]["n"]
        got.append((m, n))
        if m >= 63:
            assert 0.6 * m <= n <= m, (m, n)
    print("outliers30 (m, inliers):", got)


def test_outliers85_survives_late_with_its_inliers(oracle_c):
    """from 128 matches on the pair survives with 10 % .. 20 % of the list, and not before iteration LATE_ITER: the
    oracle run on a budget that ends in front of that iteration finds nothing"""
    sc = KC.scene("outliers85", 25)
    got = []
    for k, m in enumerate(sc.sizes):
        r, _, _ = filter_pair(oracle_c, sc, k)
        got.append((m, r["n"]))
        if m >= 128:
            assert 0.10 * m <= r["n"] <= 0.20 * m, (m, r["n"])
            assert filter_pair(oracle_c, sc, k, budget=KC.LATE_ITER)[0]["n"] == 0, m
    print("outliers85 (m, inliers):", got)


def test_ties_stand_together_in_the_oracle_order(oracle_c):
    """Inside the oracle's inlier list every planted group is present whole, with equal residual bits under the oracle's
    F, on consecutive places, ascending list index.  Printed: which groups lie across a named boundary of the SORTED
    order as well (across the list's they all do: test_tie_groups_lie_where_the_content_says)."""
    sc = KC.scene("ties", 25)
    whole, across_sorted = 0, set()
    for k, m in enumerate(sc.sizes):
        r, a, b = filter_pair(oracle_c, sc, k)
        groups = KC.pair("ties", m, 25, int(sc.view_id[k])).groups
        if m < 18:
            assert r["n"] == 0
            continue
        assert r["n"] >= 18, m
        bits = err_fmatrix(r["F"], a, b).view(np.uint64)
        pos = np.full(m, -1)
        pos[r["inliers"]] = np.arange(r["n"])
        for g in groups:
            g = list(g)
            assert (pos[g] >= 0).all(), (m, g)
            assert len(set(bits[g].tolist())) == 1, (m, g)
            assert np.array_equal(pos[g], pos[g[0]] + np.arange(len(g))), (m, g, pos[g])
            whole += 1
            for bd in KC.BOUNDARIES:
                if pos[g[0]] < bd <= pos[g[-1]]:
                    across_sorted.add(bd)
        # the residuals of the list ascend in the oracle's order, ties by index
        e = bits[r["inliers"]]
        assert np.all((e[1:] > e[:-1]) | ((e[1:] == e[:-1]) & (np.diff(r["inliers"]) > 0))), m
    print(f"ties: {whole} groups whole and consecutive; across boundaries of the sorted order: {sorted(across_sorted)}")
    assert whole == sum(len(KC.tie_groups(m)) for m in sc.sizes if m >= 18) >= 50


@pytest.mark.parametrize("content", ["degenerate_line", "degenerate_point"])
def test_degenerate_is_deterministic_and_dropped(oracle_c, content):
    """orc_fmatrix_filter orders residuals with <, > and the index (cmp_err_idx) after kernel_error has turned NaN into
    +inf, and bestNFA stops at the first residual above the threshold: no outcome rests on an unordered comparison.
    Two calls agree bit for bit, and no pair survives."""
    sc = KC.scene(content, 25)
    for k, m in enumerate(sc.sizes):
        r1, a, b = filter_pair(oracle_c, sc, k)
        r2, _, _ = filter_pair(oracle_c, sc, k)
        assert r1["n"] == r2["n"] and np.array_equal(r1["inliers"], r2["inliers"]) and r1["iters"] == r2["iters"]
        assert r1["F"].tobytes() == r2["F"].tobytes() and np.float64(r1["nfa"]).tobytes() == np.float64(r2["nfa"]).tobytes()
        assert r1["n"] == 0, (content, m, r1["n"], r1["nfa"])
    assert KC.expectations(oracle_c, content, 25) == {}


def test_collinear_is_deterministic_and_kept(oracle_c):
    """(k3_cases.collinear says why) two calls agree bit for bit; from 18 matches on the pair survives"""
    sc = KC.scene("collinear", 25)
    got = []
    for k, m in enumerate(sc.sizes):
        r1, _, _ = filter_pair(oracle_c, sc, k)
        r2, _, _ = filter_pair(oracle_c, sc, k)
        assert r1["n"] == r2["n"] and np.array_equal(r1["inliers"], r2["inliers"]) and r1["F"].tobytes() == r2["F"].tobytes()
        got.append((m, r1["n"]))
        assert (r1["n"] > 17) == (m >= 18), (m, r1["n"])
    print("collinear (m, inliers):", got)
