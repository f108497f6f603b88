"""sfmloc_reduce_points (csrc/reduce.hip) against its sequential twin (globalcoord_np.reduce_points): owner, order,
dist and the counts, every comparison on bits.  The scenes are the smallest at which the grid, the cap of the
neighbour list, the order of a keeper's list or the passes of the resolution can go wrong; the twin's answer for each
is computed once."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import globalcoord_np as GN  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

pytestmark = pytest.mark.gpu
T = 0.01
H = T * (1 + 2.0 ** -10)                    # the grid's cell
A3 = np.array([[0.0, -3.0, 0.0, 12.5], [3.0, 0.0, 0.0, -40.0], [0.0, 0.0, 3.0, 7.25]])   # scale 3 and a translation


def straddle():
    """a far corner that fixes the grid's origin at negative coordinates, then for each of the 26 directions a pair
    0.5 T |dir| apart on either side of a cell corner (mid-cell on the axes the direction does not move along)"""
    lo = np.array([-7.3, -2.1, -0.4])
    pts = [lo]
    for k, dirn in enumerate(d for d in itertools.product((-1, 0, 1), repeat=3) if any(d)):
        dirn = np.array(dirn, float)
        corner = lo + H * np.array([10 + 10 * k, 20, 30 + k])
        mid = corner + 0.5 * H * (dirn == 0)
        pts += [mid - 0.25 * T * dirn, mid + 0.25 * T * dirn]
    return np.array(pts)


def planted(n=5003, clusters=200, seed=3):
    rng = np.random.Generator(np.random.PCG64(seed))
    X = rng.uniform(-1.0, 1.0, (n, 3))
    at = rng.permutation(n)
    k = 0
    for c in range(clusters):
        m = 2 + c % 5
        X[at[k + 1:k + m]] = X[at[k]] + rng.uniform(-0.45 * T, 0.45 * T, (m - 1, 3))
        k += m
    return X


def line(n=301):
    X = np.zeros((n, 3))
    X[:, 1] = 0.6 * T * np.arange(n) - 0.9
    return X


def scenes():
    rng = np.random.Generator(np.random.PCG64(1))
    tri = np.array([[0, 0, 0], [0.7 * T, 0, 0], [1.4 * T, 0, 0.0]])
    mix = planted(n=257, clusters=30, seed=5)
    dup = rng.uniform(-0.1, 0.1, (40, 3))
    dup[20:] = dup[:20][rng.permutation(20)]
    dup[33] = dup[2]
    out = {
        "pair_in": (np.array([[0.1, 0.2, 0.3], [0.1, 0.2 + 0.5 * T, 0.3]]), None, T, 1000),
        "pair_out": (np.array([[0.1, 0.2, 0.3], [0.1, 0.2 + 1.5 * T, 0.3]]), None, T, 1000),
        "triple": (tri, None, T, 1000),
        "mix": (mix, None, T, 1000),
        "mix_shuffled": (mix[np.random.Generator(np.random.PCG64(2)).permutation(len(mix))], None, T, 1000),
        "straddle": (straddle(), None, T, 1000),
        "duplicates": (dup, None, T, 1000),
        # one keeper, three absorbed at 0.8 T, 0.2 T, 0.5 T: the list goes 2, 3, 1
        "order": (np.array([[0, 0, 0], [0.8 * T, 0, 0], [0, 0.2 * T, 0], [0, 0, -0.5 * T], [5.0, 5, 5]]), None, T, 1000),
        # six points within thres of one another, knn = 3: every list is cut to the point and its two nearest
        "knn3": (np.array([[0, 0, 0], [0.3, 0, 0], [0.1, 0.05, 0], [0.45, 0.1, 0], [0.2, 0.2, 0.15], [0.05, 0.3, 0.2]]) * T,
                 None, T, 3),
        "knn1": (tri, None, T, 1),
        "scaled": (np.cumsum(np.full((40, 3), 0.25 * T / np.sqrt(3)), 0), A3, T, 1000),
        "scaled_mix": (mix, A3, 3 * T, 1000),
        "line": (line(), None, T, 1000),
        "planted": (planted(), None, T, 1000),
        "mix_knn2": (mix, None, T, 2),
    }
    return out


SCENES = scenes()


@pytest.fixture(scope="module")
def refs():
    return {k: GN.reduce_points(*v) for k, v in SCENES.items()}


def same(dev, ref):
    for k in ("n_keep", "n_absorbed", "n_pairs", "rounds"):
        assert dev[k] == ref[k], k
    np.testing.assert_array_equal(dev["owner"], ref["owner"])
    np.testing.assert_array_equal(dev["order"], ref["order"])
    np.testing.assert_array_equal(dev["dist"].view(np.uint64), ref["dist"].view(np.uint64))


@pytest.mark.parametrize("name", list(SCENES))
def test_matches_twin(refs, name):
    X, A, thres, knn = SCENES[name]
    order = np.zeros(len(X), np.uint32)
    dev = S.reduce_points(X, A, thres, knn, out=(np.empty(len(X), np.uint32), order, np.empty(len(X))))
    same(dev, refs[name])
    assert (order[dev["n_absorbed"]:] == GN.NONE).all()


def test_what_the_scenes_are_for(refs):
    assert refs["pair_in"]["owner"].tolist() == [0, 0] and refs["pair_out"]["owner"].tolist() == [0, 1]
    assert refs["triple"]["owner"].tolist() == [0, 0, 2]                      # not transitive
    assert refs["straddle"]["n_absorbed"] == 26 and refs["straddle"]["owner"][2::2].tolist() == list(range(1, 53, 2))
    assert refs["duplicates"]["n_absorbed"] == 20 and (refs["duplicates"]["dist"] == 0).all()
    assert refs["order"]["order"].tolist() == [2, 3, 1]
    uncut = GN.reduce_points(SCENES["knn3"][0], None, T, 1000)
    assert uncut["n_keep"] == 1 and refs["knn3"]["n_keep"] > 1 and refs["knn3"]["n_pairs"] < uncut["n_pairs"]
    assert refs["knn1"]["n_absorbed"] == 0
    assert refs["scaled"]["n_keep"] == 20 and GN.reduce_points(SCENES["scaled"][0], None, T, 1000)["n_keep"] < 15   # world units
    assert refs["line"]["rounds"] >= 2 and refs["line"]["owner"].tolist() == [i - i % 2 for i in range(301)]
    assert refs["planted"]["n_absorbed"] >= 200 and refs["planted"]["n_keep"] > 4000
    assert refs["mix_knn2"]["n_pairs"] < refs["mix"]["n_pairs"]


@pytest.mark.parametrize("n", [0, 1])
def test_fewer_than_two(n):
    X = np.full((n, 3), 0.25)
    dev = S.reduce_points(X, None, T, 1000)
    same(dev, GN.reduce_points(X, None, T, 1000))
    assert dev["rounds"] == 0 and dev["n_keep"] == n


@pytest.mark.parametrize("name", ["line", "planted"])
def test_passes_per_launch_do_not_matter(refs, name):
    X, A, thres, knn = SCENES[name]
    for per in (1, 3, 0, 1000):
        same(S.reduce_points(X, A, thres, knn, params=S.merge_default_params(rounds_per_launch=per)), refs[name])


def raw(X, n, A, thres, knn, outs):
    res = S.ReduceResult(7, 7, 7, 7, 7)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))  # noqa: E731
    rc = S._L().sfmloc_reduce_points(p(X, C.c_double), n, p(A, C.c_double), thres, knn, None, p(outs[0], C.c_uint32),
                                     p(outs[1], C.c_uint32), p(outs[2], C.c_double), C.byref(res))
    return rc, res


def untouched(outs, res):
    return (outs[0] == 0xABABABAB).all() and (outs[1] == 0xCDCDCDCD).all() and (outs[2] == -1.5).all() and \
        (res.n_keep, res.n_absorbed, res.n_pairs, res.rounds, res.reserved) == (7, 7, 7, 7, 7)


def fresh(n):
    return np.full(n, 0xABABABAB, np.uint32), np.full(n, 0xCDCDCDCD, np.uint32), np.full(n, -1.5)


def test_refusals_leave_the_outputs_alone():
    X = np.ascontiguousarray(SCENES["mix"][0][:16])
    bad_x, bad_a = X.copy(), A3.copy()
    bad_x[5, 1] = np.nan
    bad_a[2, 3] = np.inf
    cases = [(X, None, 0.0), (X, None, -T), (X, None, np.nan), (X, None, np.inf), (bad_x, None, T),
             (X, np.ascontiguousarray(bad_a), T)]
    for x, a, thres in cases:
        outs = fresh(16)
        rc, res = raw(x, 16, a, thres, 1000, outs)
        assert rc == S.EINVAL and untouched(outs, res)
    # n > 2^24: refused before the arrays are looked at
    rc, res = raw(None, (1 << 24) + 1, None, T, 1000, (None, None, None))
    assert rc == S.ECAP and res.n_keep == 7
    # more than 2^21 cells on an axis
    far = np.array([[0.0, 0, 0], [0, 3e6 * T, 0]])
    outs = fresh(2)
    rc, res = raw(far, 2, None, T, 1000, outs)
    assert rc == S.ECAP and untouched(outs, res)
    near = np.array([[0.0, 0, 0], [0, 2e6 * T, 0]])
    assert S.reduce_points(near, None, T, 1000)["n_keep"] == 2
    # a world coordinate that overflows ends at the same check
    outs = fresh(2)
    rc, res = raw(np.array([[1e200, 0, 0], [-1e200, 0, 0.0]]), 2, np.ascontiguousarray(A3 * 1e150), T, 1000, outs)
    assert rc == S.ECAP and untouched(outs, res)
    # more than 2^28 close pairs: 23 200 copies of one point, each listing all the later ones
    n = 23200
    assert n * (n - 1) // 2 > 1 << 28
    outs = fresh(n)
    rc, res = raw(np.zeros((n, 3)), n, None, T, n, outs)
    assert rc == S.ECAP and untouched(outs, res)
    assert "2^28" in S._L().sfmloc_last_error().decode()
