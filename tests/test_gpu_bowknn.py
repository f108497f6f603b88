"""GPU: sfmloc_bow_knn (csrc/bowknn.hip) against the C oracle row by row (tests/bowknn_np.py: K8's own selection and
distance for every row) and against an order-free int64 reference, bit for bit in all three outputs; then the two tools
that turn it into a pair file, against each other and against knn_pairs of the reference.

The distance kernel's tile is 16 query rows x 16 bank rows (a wave: 4 x 16), staged 256 elements at a time; the selection
keeps a row in registers up to 16 384 views.  The sizes run one under, on and over each of those edges."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bow_cases as BC
import bowknn_np as KN
import sfmlocalization_amd as S
from sfmlocalization_amd import bowpairs, capi, extfeat, fileio

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sfmlocalization_amd", "bin", "ComputeBoWPairs")


def uniform(seed, n, dim):
    return np.random.Generator(np.random.PCG64(seed)).random((n, dim), np.float32)


def integers(seed, n, dim):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 16, (n, dim)).astype(np.float32)


@pytest.mark.parametrize("n", [2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1023, 1025])
def test_sizes(oracle_c, n):
    """every row against the oracle; k = 5 above n - 1 at n = 2, 3 checks the padding of every row"""
    bow = uniform(n, n, 24)
    for k in sorted({1, 5, n - 1}):
        KN.same(capi.bow_knn(bow, k), KN.expected(oracle_c, bow, k, 0), tag=f"n {n} k {k}")


@pytest.mark.parametrize("dim", [1, 63, 64, 65, 127, 500, 1000])
def test_dims(oracle_c, dim):
    """less than one wave of elements, a ragged last round, several staged chunks; uniform vectors against the oracle,
    integer ones against the oracle and against int64 arithmetic"""
    n, k = 130, 7
    bow = uniform(1000 + dim, n, dim)
    KN.same(capi.bow_knn(bow, k), KN.expected(oracle_c, bow, k, 0), tag=f"dim {dim} uniform")
    ints = integers(2000 + dim, n, dim)
    got = capi.bow_knn(ints, k)
    KN.same(got, KN.expected_int(ints, k, 0), tag=f"dim {dim} int64")
    KN.same(got, KN.expected(oracle_c, ints, k, 0), tag=f"dim {dim} integers, oracle")


def test_window_smallest_case_with_row_dependent_counts(oracle_c):
    bow = uniform(5, 12, 24)
    nbr, dist, count = got = capi.bow_knn(bow, 5, window=4)
    assert count.tolist() == [5, 5, 5, 4, 3, 3, 3, 3, 4, 5, 5, 5]          # row 0: 7 candidates; row 6: {0, 1, 11}
    assert nbr[6].tolist() == [0, 1, 11, KN.PAD, KN.PAD] and np.isposinf(dist[6, 3:]).all() and np.isfinite(dist[6, :3]).all()
    assert nbr[0].min() >= 5
    KN.same(got, KN.expected(oracle_c, bow, 5, 4))


@pytest.mark.parametrize("window", [0, 1, 5, 198, 199, 200])
def test_window_clipped_bands(oracle_c, window):
    """rows 0 and n - 1 with the band clipped by the ends; 198 leaves one candidate to the two end rows alone; 199 and 200
    leave none to anybody"""
    n, k = 200, 9
    bow = uniform(77, n, 24)
    nbr, dist, count = got = capi.bow_knn(bow, k, window=window)
    KN.same(got, KN.expected(oracle_c, bow, k, window), tag=f"window {window}")
    if window == 198:
        assert count.tolist() == [1] + [0] * 198 + [1] and nbr[0, 0] == 199 and nbr[199, 0] == 0
    if window >= 199:
        assert (count == 0).all() and (nbr == KN.PAD).all() and np.isposinf(dist).all()


def test_ties_all_rows_identical(oracle_c):
    n, k, w = 100, 6, 2
    bow = np.tile(uniform(9, 1, 24), (n, 1))
    nbr, dist, count = got = capi.bow_knn(bow, k, window=w)
    assert (dist == 0).all() and (count == k).all()
    for i in range(n):
        assert nbr[i].tolist() == [j for j in range(n) if abs(j - i) > w][:k]
    KN.same(got, KN.expected(oracle_c, bow, k, w))


@pytest.mark.parametrize("window", [0, 3])
def test_ties_duplicate_groups(oracle_c, window):
    """40 copies of one vector across index 63 / 64 and 40 of another at the end; k cuts inside a group"""
    n = 150
    bow = uniform(10, n, 24)
    bow[44:84] = bow[44]
    bow[110:150] = bow[110]
    for k in (10, 39, 45):
        got = capi.bow_knn(bow, k, window=window)
        KN.same(got, KN.expected(oracle_c, bow, k, window), tag=f"k {k}")
        assert (got[1][50] == 0).sum() == min(k, 39 - 2 * window)      # row 50's copies outside its window


def test_ties_duplicate_inside_and_outside_the_window(oracle_c):
    n, k, w = 50, 4, 3
    bow = uniform(11, n, 24)
    bow[23] = bow[24] = bow[17] = bow[16] = bow[20]          # |j - 20| = 3 (inside), 4 (outside), on both sides
    nbr, dist, count = got = capi.bow_knn(bow, k, window=w)
    assert 24 in nbr[20] and 16 in nbr[20] and 23 not in nbr[20] and 17 not in nbr[20]
    assert dist[20][nbr[20] == 24] == 0 and dist[20][nbr[20] == 16] == 0
    KN.same(got, KN.expected(oracle_c, bow, k, w))


def test_distances_that_overflow_to_inf(oracle_c):
    """entries of 1e19: finite inputs, distances of +inf.  They order after every finite distance and before an excluded
    entry, and count does not change"""
    n, k, w = 40, 35, 2
    rng = np.random.Generator(np.random.PCG64(12))
    bow = rng.random((n, 8), np.float32)
    bow[10:20] = (rng.choice([-1.0, 1.0], (10, 8)) * 1e19).astype(np.float32)
    nbr, dist, count = got = capi.bow_knn(bow, k, window=w)
    np.testing.assert_array_equal(count, KN.counts(n, k, w))
    assert np.isposinf(dist[0, :count[0]]).sum() >= 5 and np.isfinite(dist[0, :count[0]]).sum() >= 25
    assert ((np.arange(k)[None, :] < count[:, None]) == (nbr != KN.PAD)).all()
    KN.same(got, KN.expected(oracle_c, bow, k, w))


def test_rows_per_launch_changes_no_bit(oracle_c):
    n, k, w = 257, 9, 2
    bow = uniform(13, n, 24)
    ref = capi.bow_knn(bow, k, window=w)
    KN.same(ref, KN.expected(oracle_c, bow, k, w))
    for per in (1, 7, 64, 256, 257, 1000):
        KN.same(capi.bow_knn(bow, k, window=w, rows_per_launch=per), ref, tag=f"rows_per_launch {per}")


@pytest.mark.parametrize("n", [16385, 20000])
def test_above_the_register_form_of_the_selection(oracle_c, n):
    """the whole call runs; count of every row; the oracle on a fixed list of rows"""
    k, w = 20, 3
    bow = uniform(n, n, 8)
    rng = np.random.Generator(np.random.PCG64([14, n]))
    rows = sorted({0, 1, 63, 64, 4095, 4096, 16383, 16384, n - 2, n - 1} | set(rng.choice(n, 22, replace=False).tolist()))
    KN.same(capi.bow_knn(bow, k, window=w), KN.expected(oracle_c, bow, k, w, rows=rows), rows=rows, tag=f"n {n}")


def test_rows_agree_with_k8_on_the_same_matrix():
    """row i at window 0 = Map.bow_select(bow[i], k, all views but i): two paths into one semantics"""
    n, k = 300, 12
    bow = uniform(15, n, 500)
    nbr, dist, count = capi.bow_knn(bow, k)
    view_id, view_off, desc = BC.map_arrays(n)
    with S.Map(view_id, view_off, desc, bow=bow) as dm:
        for i in range(n):
            cand = np.delete(np.arange(n, dtype=np.uint32), i)
            np.testing.assert_array_equal(nbr[i], dm.bow_select(bow[i], k, cand), err_msg=f"row {i}")
            d = dm.bow_distances(bow[i])
            np.testing.assert_array_equal(BC.bits_of(dist[i]), BC.bits_of(d[nbr[i]]), err_msg=f"row {i}")
    assert (count == k).all()


def test_profile_reports_device_time():
    bow = uniform(16, 300, 64)
    capi.bow_knn(bow, 5, profile=True)
    assert capi.bowknn_last_ms() > 0.0
    capi.bow_knn(bow, 5)
    assert capi.bowknn_last_ms() == 0.0


def test_pair_files_of_both_tools(oracle_c, tmp_path):
    """a walk of 20 places there and back: view i and view 39 - i are near-copies, neighbouring frames similar"""
    V, dim, k, v = 40, 500, 3, 2
    rng = np.random.Generator(np.random.PCG64(17))
    place = np.cumsum(rng.normal(0, 0.05, (V // 2, dim)), 0) + rng.random(dim)
    vec = np.concatenate([place, place[::-1] + rng.normal(0, 1e-3, (V // 2, dim))])
    ids = [5 + 3 * i for i in range(V)]
    names = [f"img{i:04d}.jpg" for i in range(V)]
    fileio.write_sfm_data(tmp_path / "sfm_data.json", fileio.make_sfm_data(ids, names, 640, 480, 500.0, 320.0, 240.0,
                                                                          root_path=str(tmp_path)))
    for name, x in zip(names, vec):
        fileio.write_mat_bin(tmp_path / (name[:-4] + ".bow"), x.reshape(-1, 1))
    bow = vec.astype(np.float32)
    exp_nbr, _, exp_count = KN.expected(oracle_c, bow, k, v)
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for flags in ([], ["--mutual"]):
        tag = "m" if flags else "p"
        for cmd, out in (([sys.executable, "-m", "sfmlocalization_amd.bowpairs"], f"py.{tag}.txt"), ([EXE], f"cc.{tag}.txt")):
            r = subprocess.run(cmd + ["-m", str(tmp_path), "-k", str(k), "-v", str(v), "-o", out] + flags,
                               capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)
            assert r.returncode == 0, (r.stdout, r.stderr)
            assert "pairs of 40 views" in r.stdout
        py, cc = (tmp_path / f"py.{tag}.txt").read_bytes(), (tmp_path / f"cc.{tag}.txt").read_bytes()
        assert py == cc and len(py) > 0
        pairs = extfeat.read_pair_file(tmp_path / f"py.{tag}.txt")
        assert pairs == bowpairs.knn_pairs(ids, exp_nbr, exp_count, video_frame=v, mutual=bool(flags))
        assert all(a in ids and b in ids and a < b for a, b in pairs)
        video = set(extfeat.generate_video_match_pairs(ids, v))
        closing = {(ids[i], ids[V - 1 - i]) for i in range(V // 2)}
        assert closing - video <= set(pairs) and len(closing - video) == 19 and video <= set(pairs)
    # the default output name, and -w: the window on its own
    r = subprocess.run([EXE, "-m", str(tmp_path), "-k", str(k), "-w", "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "window 0" in r.stdout
    assert extfeat.read_pair_file(tmp_path / "pairs.bow.txt") == bowpairs.knn_pairs(ids, *KN.expected(oracle_c, bow, k, 0)[::2])
