"""CPU: the inputs of tests/test_gpu_bow_edges.py (tests/bow_cases.py) reach what they are for -- distinct-prefix counts,
tie runs across the compaction's chunk and wave boundaries, the tie count at every k, subnormal and infinite distances,
the merge cases' owner counts -- and the C oracle agrees with the references R1 / R2 bit for bit, with R3 within its
band."""
import numpy as np
import pytest

import bow_cases as BC
from sfmlocalization_amd import dist as D


def oracle_dists(oc, case):
    return np.array([oc.bow_dist(row, case.query) for row in case.bow], np.float32)


def check_oracle(oc, case):
    for k, cand in case.picks:
        got = oc.bow_select(case.bow, case.query, k, cand)
        if case.ref == "R3":
            case.check_r3(got, k, cand)
            assert case.r3_band(k, cand)[2] <= 4, (case.name, k)
        else:
            np.testing.assert_array_equal(got, case.expected(k, cand), err_msg=f"{case.name} k {k}")


def distinct_prefixes(case, top_bits):
    return len(np.unique(BC.bits_of(case.dist) >> (32 - top_bits)))


@pytest.mark.parametrize("case", BC.pattern_cases(), ids=repr)
def test_pattern_cases(oracle_c, case):
    check_oracle(oracle_c, case)
    bits = BC.bits_of(case.dist)
    pattern, n = case.name.split("-")[0], case.n
    np.testing.assert_array_equal(BC.bits_of(oracle_dists(oracle_c, case)), bits)
    if pattern == "uniform" and n >= 16383:        # pass 1 nearly decides: what the other patterns are there to change
        assert 30 <= distinct_prefixes(case, 11) <= 150
    if pattern == "top11":
        assert distinct_prefixes(case, 11) == 1 and distinct_prefixes(case, 22) > 1000
    if pattern == "top22":
        assert distinct_prefixes(case, 22) <= 2 and len(np.unique(bits)) > 400      # (pass 3 still has work)
    if pattern == "all_equal":
        assert len(np.unique(bits)) == 1
        np.testing.assert_array_equal(case.expected(1024), np.arange(1024))
    if pattern == "edge_values":
        g = case.meta["n_inf"]
        assert (bits == BC.INF_BITS).sum() == g == BC.INF_GROUP and not np.isnan(case.dist).any()
        assert (bits == 0).sum() >= 4                                   # distance 0, and squares below the smallest subnormal
        assert ((bits > 0) & (bits < BC.MIN_NORMAL_BITS)).sum() >= 4    # subnormal distances
        k = case.meta["k_in_inf"]
        assert (k, None) in case.picks and n - g < k < n
        sel = case.expected(k)
        assert (bits[sel] == BC.INF_BITS).sum() == g // 2 and (bits[np.setdiff1d(np.arange(n), sel)] == BC.INF_BITS).all()
    assert any(c is not None and len(c) == m for _, c in case.picks for m in (16384, 16385, 3)) == (n == 40000)


@pytest.mark.parametrize("n", BC.SIZES)
def test_tie_runs_cases(oracle_c, n):
    chunk, L = BC.chunk_of(n), min(BC.RUN, n)
    runs = dict((name, (a, ln)) for name, a, ln in BC.run_starts(n))
    assert "end" in runs and runs["end"] == (n - L, L)
    if n >= 1023:                                   # all three runs, where the kernel's boundaries are
        a, _ = runs["chunk"]
        assert any(b % chunk == 0 and b // chunk % 64 != 0 for b in range(a + 1, a + L))
        a, _ = runs["wave"]
        assert a < 64 * chunk < a + L
    if n == 65:
        assert runs["end"][0] < 64 < n              # (the one run of a short list straddles the wave boundary)
    cases = BC.tie_runs_cases(n)
    assert [c.picks[0][0] for c in cases[::3]] == BC.ks_for(n)
    seen = set()
    for case in cases:
        check_oracle(oracle_c, case)
        if n <= 1025 or case is cases[0]:
            np.testing.assert_array_equal(BC.bits_of(oracle_dists(oracle_c, case)), BC.bits_of(case.dist))
        k = case.picks[0][0]
        bits = BC.bits_of(case.dist)
        name, a, ln = case.meta["cut"]
        T = np.sort(bits)[k - 1]
        assert (bits[a:a + ln] == T).all() and (bits == T).sum() == ln            # the k-th distance is the run's
        taken, less = case.meta["taken"], int((bits < T).sum())
        assert less == k - taken and 1 <= taken <= ln
        sel = case.expected(k)
        np.testing.assert_array_equal(sel[np.isin(sel, np.arange(a, a + ln))], np.arange(a, a + taken))
        for _, b, lb in case.meta["runs"]:
            assert len(np.unique(bits[b:b + lb])) == 1 and (bits == bits[b]).sum() == lb
        seen.add((name, "first" if taken == 1 else "last" if taken == ln else "middle"))
    if n >= 1023:                                   # every run is cut, and a run at its first, a middle and its last element
        assert {s[0] for s in seen} == {"chunk", "wave", "end"} and {s[1] for s in seen} == {"first", "middle", "last"}
        for k in (1023, 1024, 1025):
            if k + L <= n:
                assert sorted(c.meta["taken"] for c in BC.tie_runs_cases(n) if c.picks[0][0] == k) == [1, L // 2, L]


@pytest.mark.parametrize("case", BC.dim_cases(), ids=repr)
def test_dim_cases(oracle_c, case):
    check_oracle(oracle_c, case)
    d = oracle_dists(oracle_c, case)
    if case.ref == "R1":
        assert case.dist.max() < 2 ** 24 and len(np.unique(case.dist)) < case.n // 4        # exact, and full of ties
        np.testing.assert_array_equal(BC.bits_of(d), BC.bits_of(case.dist_f32))
    else:
        g = ((case.dim + 63) // 64 + 8) * 2.0 ** -24
        assert (np.abs(d.astype(np.float64) - case.dist) <= g * case.dist).all()


def test_key_cases(oracle_c):
    case = BC.five_view_case()
    ids = BC.map_ids(case.n)
    np.testing.assert_array_equal(BC.bits_of(oracle_dists(oracle_c, case)), BC.bits_of(case.dist_f32))
    keys = BC.expected_keys(case, ids, 1024)
    assert (keys[5:] == BC.PAD).all() and (keys[:4] < keys[1:5]).all()
    np.testing.assert_array_equal(keys[:5], np.sort(D.bow_key(case.dist_f32, ids)))
    assert BC.PAD == D.BOW_KEY_PAD
    big = BC.r1_case(24)
    ids = BC.map_ids(big.n)
    assert ids[-1] == 2 ** 24 - 1 and (np.diff(ids.astype(np.int64)) == 3).all()
    for knn in (1, 100, 1024):
        np.testing.assert_array_equal(BC.expected_keys(big, ids, knn), np.sort(D.bow_key(big.dist_f32, ids))[:knn])


def test_merge_cases():
    cases = {c.name: c for c in BC.merge_cases()}
    assert sorted(cases) == ["cap", "cap_none", "cross_tie_hi", "cross_tie_lo", "mostly_pad", "short_shard", "strided"]
    for c in cases.values():
        exp = c.expected()
        assert len(exp) == min(c.k, c.n_views)
        np.testing.assert_array_equal(exp[exp != c.n_views], D.select_from_keys(c.gathered(), c.k, c.local_id))
        assert (np.diff(c.local_id.astype(np.int64)) > 0).all() and c.local_id.max() < 2 ** 24
        real = c.gathered()[c.gathered() != BC.PAD]
        assert len(np.unique(real)) == len(real)                      # (the kernel ranks by counting: distinct keys)
    c = cases["cap"]
    assert c.keys.shape == (8, 1024) and c.k == 1024 and c.n_owned() == 1024 and (c.keys != BC.PAD).all()
    assert (cases["cap_none"].keys == c.keys).all() and cases["cap_none"].n_owned() == 0
    assert (cases["cap_none"].expected() == cases["cap_none"].n_views).all() and len(cases["cap_none"].expected()) == 1024
    c = cases["short_shard"]
    assert c.n_views == 5 and c.k == 1024 and c.expected().tolist() == [0, 3, 4, 5, 5]
    lo, hi = cases["cross_tie_lo"], cases["cross_tie_hi"]
    assert (lo.keys == hi.keys).all()
    w = np.sort(lo.gathered().ravel())
    assert w[99] >> np.uint64(32) == w[100] >> np.uint64(32) and w[98] >> np.uint64(32) < w[99] >> np.uint64(32)
    assert int(w[99]) & 0xFFFFFFFF == lo.local_id[123] and int(w[100]) & 0xFFFFFFFF == hi.local_id[45]
    assert 123 in lo.expected() and 45 not in hi.expected() and lo.n_owned() == 50 and hi.n_owned() == 50
    c = cases["mostly_pad"]
    assert (c.keys != BC.PAD).sum() == 3 and c.expected().tolist() == [1, 6, 7, 7, 7, 7, 7]
    c = cases["strided"]
    assert c.part_stride == 3 * c.k and 0 < c.n_owned() < c.k
    decoys = c.keys[:, c.k:]
    assert (decoys < c.gathered().min()).all() and np.isin(decoys & np.uint64(0xFFFFFFFF), c.local_id).all()


def test_both_forms_of_the_selection_are_asked_for():
    """k_bow_topk keeps up to 16 384 distances in registers and re-reads global memory above: every family of cases has
    candidate counts on both sides, and the two next to the threshold"""
    def counts(cases):
        return {case.n if cand is None else len(cand) for case in cases for _, cand in case.picks}
    for fam in (BC.pattern_cases(), [c for n in BC.SIZES for c in BC.tie_runs_cases(n)], BC.dim_cases()):
        got = counts(fam)
        assert min(got) <= 65 and max(got) >= 20000 and any(n > BC.REG_LIMIT for n in got)
    for fam in (BC.pattern_cases(), [c for n in BC.SIZES for c in BC.tie_runs_cases(n)]):
        assert {BC.REG_LIMIT, BC.REG_LIMIT + 1, 40000} <= counts(fam)
    for p in BC.PATTERNS:
        assert {BC.REG_LIMIT, BC.REG_LIMIT + 1, 40000} <= counts([BC.pattern_case(p, n) for n in BC.PATTERN_SIZES])
