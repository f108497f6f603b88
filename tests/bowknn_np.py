"""References for sfmloc_bow_knn (include/sfmloc.h "All-views BoW k-NN"; csrc/bowknn.hip).  No GPU here.

  expected      row i from the C oracle: the selection oracle_c.bow_select(bow, bow[i], k, cand(i)) -- K8's own reference --
                and the distance orc_bow_dist(bow[j], bow[i]) of every kept j; count from the definition of cand(i).
  expected_int  independent of the oracle and of any summation order: for matrices of small integers (values 0..15,
                dim <= 1000: every sum is below 2^24) float32 is exact however the sum is ordered, so the distances are
                int64 NumPy and the ranking a stable sort by distance over ascending indices, i.e. by (d, index).
Both return (nbr uint32 [rows, k], dist float32 [rows, k], count uint32 [n]); unused slots hold 0xFFFFFFFF and +inf.
"""
import ctypes as C

import numpy as np

PAD = 0xFFFFFFFF


def candidates(i, n, window):
    """cand(i) = { j : |j - i| > window }, ascending"""
    j = np.arange(n, dtype=np.int64)
    return j[np.abs(j - i) > window].astype(np.uint32)


def counts(n, k, window):
    """count[i] = min(k, |cand(i)|), from the definition"""
    return np.array([min(k, len(candidates(i, n, window))) for i in range(n)], np.uint32)


def counts_closed_form(n, k, window):
    """the same without building the lists (the large sizes): n minus the part of [i - window, i + window] inside [0, n)"""
    i = np.arange(n, dtype=np.int64)
    band = np.minimum(i + window, n - 1) - np.maximum(i - window, 0) + 1
    return np.minimum(k, n - band).astype(np.uint32)


def expected(oracle_c, bow, k, window, rows=None):
    """rows: the rows to build (default all); count is always that of every row"""
    bow = np.ascontiguousarray(bow, np.float32)
    n, dim = bow.shape
    rows = list(range(n)) if rows is None else [int(r) for r in rows]
    nbr = np.full((len(rows), k), PAD, np.uint32)
    dist = np.full((len(rows), k), np.inf, np.float32)
    f, base = oracle_c.lib().orc_bow_dist, bow.ctypes.data
    for r, i in enumerate(rows):
        cand = candidates(i, n, window)
        if len(cand) == 0:
            continue
        sel = oracle_c.bow_select(bow, bow[i], k, cand)
        nbr[r, :len(sel)] = sel
        dist[r, :len(sel)] = [f(C.c_void_p(base + 4 * dim * int(j)), C.c_void_p(base + 4 * dim * i), C.c_int(dim)) for j in sel]
    return nbr, dist, (counts(n, k, window) if n <= 2048 else counts_closed_form(n, k, window))


def expected_int(bow, k, window):
    b = np.asarray(bow)
    assert (b == np.round(b)).all() and b.min() >= 0 and b.max() <= 15 and b.shape[1] <= 1000
    b = b.astype(np.int64)
    n = len(b)
    nbr = np.full((n, k), PAD, np.uint32)
    dist = np.full((n, k), np.inf, np.float32)
    for i in range(n):
        d = ((b - b[i]) ** 2).sum(1)
        assert d.max() < 2 ** 24
        cand = candidates(i, n, window).astype(np.int64)
        kept = np.sort(cand[np.argsort(d[cand], kind="stable")[:k]])
        nbr[i, :len(kept)] = kept
        dist[i, :len(kept)] = d[kept].astype(np.float32)
    return nbr, dist, counts(n, k, window)


def same(got, exp, rows=None, tag=""):
    """bit equality of (nbr, dist, count); rows: the rows `exp` holds"""
    from bow_cases import bits_of
    nbr, dist, count = got
    sl = slice(None) if rows is None else np.asarray(rows, np.int64)
    np.testing.assert_array_equal(count, exp[2], err_msg=f"{tag} count")
    np.testing.assert_array_equal(nbr[sl], exp[0], err_msg=f"{tag} nbr")
    np.testing.assert_array_equal(bits_of(dist[sl]), bits_of(exp[1]), err_msg=f"{tag} dist")
