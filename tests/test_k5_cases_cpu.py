"""CPU: the cases of tests/k5_cases.py are what their contents claim -- conditions on the INPUTS, checked against the C
oracle alone (adjust_scene.p3p_raw through k5_cases.expectations), so that no change of a kernel can make a case stop
testing what it is for.  test_gpu_k5_forms.py runs the same cases through every launch form of K5."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import k5_cases as KC  # noqa: E402

TIE_FLOOR, NEAR_TIE_FLOOR = 20, 10   # per content, over all its sizes
BUDGET = 4096                        # p3p_max_iteration of the tool
RESERVE = BUDGET // 10


@pytest.fixture(scope="module")
def exp(oracle_c):
    return KC.expectations(oracle_c)


def residuals(case, P):
    """the oracle's residuals (kernel_error, normalised frame, same operation order) of a case under K [R|t] = P.  The
    normalised model is recovered from P, so the values are the oracle's up to that rounding -- exact copies of a
    correspondence get equal bits whatever the model."""
    f, ppx, ppy = KC.INTRINSIC
    pix, X = KC.case_arrays(case)
    inv_f = 1.0 / f
    a = pix * inv_f + np.array([-ppx * inv_f, -ppy * inv_f])
    M = np.stack([(P[0] - ppx * P[2]) * inv_f, (P[1] - ppy * P[2]) * inv_f, P[2]])
    p = ((M[:, 0] * X[:, 0:1] + M[:, 1] * X[:, 1:2]) + M[:, 2] * X[:, 2:3]) + M[:, 3]
    dx, dy = p[:, 0] / p[:, 2] - a[:, 0], p[:, 1] / p[:, 2] - a[:, 1]
    e = dx * dx + dy * dy
    e[np.isnan(e)] = np.inf
    return e


def test_the_case_list():
    """23 clean sizes, 12 each of ties / near_ties / exact / late, 3 none, 11 degenerate: 85 cases, every one with the n
    it names, distinct ascending id_views, copies planted where the contents say."""
    assert len(KC.CASES) == 23 + 4 * 12 + 3 + 11 and len(KC.BY_NAME) == len(KC.CASES)
    assert [c.n for c in KC.CASES] == sorted(c.n for c in KC.CASES)
    assert [c.id_view for c in KC.CASES] == list(range(KC.ID_VIEW0, KC.ID_VIEW0 + len(KC.CASES)))
    assert {c.n for c in KC.CASES if c.content == "clean"} == set(KC.SIZES) and KC.SIZES[0] == 11
    for content in ("ties", "near_ties", "exact", "late"):
        assert sorted(c.n for c in KC.CASES if c.content == content) == [64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049,
                                                                         4096, 4097]
    assert sorted(c.n for c in KC.CASES if c.content == "none") == [12, 257, 1025]
    assert max(c.n for c in KC.CASES if c.content == "degenerate") == 257
    for c in KC.CASES:
        pix, X = KC.case_arrays(c)
        assert c.name == f"{c.content}_{c.n}" and pix.shape == (c.n, 2) and X.shape == (c.n, 3)
        assert np.isfinite(pix).all() and np.isfinite(X).all()
        if c.content in ("ties", "near_ties"):
            pairs = KC.planted_pairs(c.n, c.seed)
            flat = [i for p in pairs for i in p]
            assert len(set(flat)) == len(flat) and len(pairs) >= c.n // 4      # disjoint, about n / 3
            assert {hi - lo for lo, hi in pairs} == {d for d in KC.PAIR_DISTANCES if d < c.n}
            for j, (lo, hi) in enumerate(pairs):
                assert np.array_equal(X[lo], X[hi]) and pix[lo, 1] == pix[hi, 1]
                if c.content == "ties":
                    assert pix[lo, 0] == pix[hi, 0]
                else:
                    assert pix[hi, 0] == np.nextafter(pix[lo, 0], np.inf if j % 2 == 0 else -np.inf)
        if c.content == "degenerate":
            m = KC.degenerate_copies(c.n)
            assert m == (40 if c.n >= 80 else c.n // 2)
            assert len(np.unique(np.concatenate([pix[:m], X[:m]], 1), axis=0)) == 3
    a = KC.assemble(KC.CASES)
    assert a["obs_off"][-1] == sum(c.n for c in KC.CASES) and np.all(np.diff(a["landmark_id"].astype(np.int64)) > 0)
    assert np.bincount(a["obs_view"]).tolist() == [c.n for c in KC.CASES]
    order, ids = KC.descending(KC.CASES)
    assert [c.n for c in order] == sorted((c.n for c in KC.CASES), reverse=True) and ids[0] > KC.CASES[-1].id_view


def test_every_case_has_its_n_and_its_outcome(exp):
    """clean, ties, near_ties, exact and late succeed; none ends without inliers after the whole budget; exact keeps
    every correspondence; late needs more than 64 iterations before AC-RANSAC cuts the budget to the reserve.
    Observed: late runs 483 .. 913 iterations (budget cut at iteration 74 .. 504); degenerate (nothing required of it)
    fails without inliers at 11 and 12 and succeeds from 63 on, at 129, 255 and 257 on a model of 16 copies."""
    late_iters = []
    for c in KC.CASES:
        e = exp[c.name]
        assert e["ran"] and e["n_obs"] == c.n, c.name
        assert 1 <= e["iters"] <= BUDGET, c.name
        if c.content in ("clean", "ties", "near_ties", "exact", "late"):
            assert e["ok"] and e["n"] >= 8, c.name
        if c.content == "none":
            assert e["n"] == 0 and not e["ok"] and e["iters"] == BUDGET and not np.any(e["P"]), c.name
        if c.content == "exact":
            assert e["n"] == c.n, c.name
        if c.content == "late":
            late_iters.append(e["iters"])
            assert e["iters"] > 64 + RESERVE, (c.name, e["iters"])
    print("late: iterations", late_iters)
    print("degenerate:", [(c.n, bool(exp[c.name]["ok"]), exp[c.name]["n"]) for c in KC.CASES if c.content == "degenerate"])


def test_ties_are_adjacent_in_the_oracle_order(exp):
    """Planted copies that are both inliers of the oracle's model have bit-equal residuals and stand next to each other
    in the oracle's inlier order, lower list index first (std::sort on (residual, index) pairs).  Floor: 20 such pairs
    over the content's sizes; every case has at least one.  Observed: 3 919 pairs over the twelve sizes (17 at n = 64, 15 at
    65), all adjacent and in index order: 1 092 / 1 062 / 1 008 / 757 at distances 1 / 64 / 256 / 1 024."""
    total, by_dist = 0, {}
    for c in KC.CASES:
        if c.content != "ties":
            continue
        e = exp[c.name]
        pos = np.full(c.n, -1)
        pos[e["inliers"]] = np.arange(e["n"])
        res = residuals(c, e["P"]).view(np.uint64)
        got = 0
        for lo, hi in KC.planted_pairs(c.n, c.seed):
            if pos[lo] < 0 or pos[hi] < 0:
                continue
            assert res[lo] == res[hi], (c.name, lo, hi)
            assert pos[hi] == pos[lo] + 1, (c.name, lo, hi, pos[lo], pos[hi])
            got += 1
            by_dist[hi - lo] = by_dist.get(hi - lo, 0) + 1
        print(f"{c.name}: {got} tied inlier pairs, all adjacent, lower index first")
        assert got >= 1, c.name
        total += got
    print(f"ties: {total} pairs (floor {TIE_FLOOR}), by distance {sorted(by_dist.items())}")
    assert total >= TIE_FLOOR and set(by_dist) == set(KC.PAIR_DISTANCES)


def test_near_ties_reach_the_packed_sort_fallback(exp):
    """Planted one-ulp copies whose residual keys (the f64 bits) agree above bit 10 and differ below it, the larger key at
    the lower list index: what wave_sort_fast orders wrongly by index and must hand to its fallback (distances 1 and 64)
    and what the rank merge sees as keys a few ulps apart (256, 1 024).  Floor: 10 such pairs over the content's sizes.
    Observed: 962 of 5 330 planted pairs (253 / 246 / 274 / 189 at distances 1 / 64 / 256 / 1 024); every size has some, 2 of
    21 at n = 64."""
    total, planted, by_dist = 0, 0, {}
    for c in KC.CASES:
        if c.content != "near_ties":
            continue
        key = residuals(c, exp[c.name]["P"]).view(np.uint64)
        got = 0
        pairs = KC.planted_pairs(c.n, c.seed)
        for lo, hi in pairs:
            if (key[lo] >> np.uint64(10)) == (key[hi] >> np.uint64(10)) and key[lo] > key[hi]:
                got += 1
                by_dist[hi - lo] = by_dist.get(hi - lo, 0) + 1
        print(f"{c.name}: {got} of {len(pairs)} planted pairs descend below bit 10")
        total += got
        planted += len(pairs)
    print(f"near_ties: {total} of {planted} pairs (floor {NEAR_TIE_FLOOR}), by distance {sorted(by_dist.items())}")
    assert total >= NEAR_TIE_FLOOR
    assert by_dist.get(1, 0) + by_dist.get(64, 0) >= 1 and by_dist.get(256, 0) + by_dist.get(1024, 0) >= 1
