"""CPU: the host side of the all-views BoW k-NN -- the entry points of sfmloc_bow_knn as the header declares them, every
refusal it makes before anything is allocated or launched (they come back without a GPU, outputs untouched), the calls
that launch nothing, bowpairs.knn_pairs on hand-written lists, and the refusals of the two command-line tools."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from sfmlocalization_amd import _abi, bowpairs, capi, extfeat, fileio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "sfmlocalization_amd", "bin", "ComputeBoWPairs")
PAD = 0xFFFFFFFF


def test_symbols_and_defaults():
    names = {"sfmloc_bowknn_default_options", "sfmloc_bow_knn", "sfmloc_bowknn_last_ms"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        assert getattr(L, n).argtypes == _abi.PROTOTYPES[n][1]
    assert [f for f, _ in capi.BowknnOptions._fields_] == ["k", "window", "rows_per_launch", "profile"]
    o = capi.bowknn_default_options()
    assert (o.k, o.window, o.rows_per_launch, o.profile) == (20, 0, 0, 0)
    assert L.sfmloc_abi_version() == 2
    assert capi.bowknn_last_ms() == 0.0


def raw_call(bow, n, dim, nbr, dist, count, opt=None, **fields):
    """sfmloc_bow_knn as C sees it (None = a NULL array) -> (code, error text)"""
    o = capi.bowknn_default_options(**fields) if opt is None else opt
    p = capi._ptr
    rc = capi._L().sfmloc_bow_knn(0, p(bow, C.c_float), n, dim, C.byref(o) if o is not False else None,
                                  p(nbr, C.c_uint32), p(dist, C.c_float), p(count, C.c_uint32))
    return rc, capi._L().sfmloc_last_error().decode()


def filled(n, k):
    return np.full((n, k), 0xABCD1234, np.uint32), np.full((n, k), -7.5, np.float32), np.full(n, 0x5A5A5A5A, np.uint32)


def test_refusals_come_back_without_a_gpu_and_write_nothing():
    bow = np.arange(5 * 4, dtype=np.float32).reshape(5, 4)
    nan, inf = bow.copy(), bow.copy()
    nan[3, 2], inf[1, 0] = np.nan, -np.inf
    big = np.zeros(((1 << 22) + 1, 1), np.float32)
    nbr, dist, count = filled(5, 3)
    for kw, code, text in (
            (dict(k=0), capi.EINVAL, "sfmloc_bow_knn: k = 0"),
            (dict(dim=0), capi.EINVAL, "sfmloc_bow_knn: dim = 0"),
            (dict(bow=None), capi.EINVAL, "sfmloc_bow_knn: null array"),
            (dict(nbr=None), capi.EINVAL, "sfmloc_bow_knn: null array"),
            (dict(dist=None), capi.EINVAL, "sfmloc_bow_knn: null array"),
            (dict(count=None), capi.EINVAL, "sfmloc_bow_knn: null array"),
            (dict(bow=nan), capi.EINVAL, "sfmloc_bow_knn: row 3 has a non-finite value"),
            (dict(bow=inf), capi.EINVAL, "sfmloc_bow_knn: row 1 has a non-finite value"),
            (dict(bow=big, n=(1 << 22) + 1, dim=1), capi.ECAP, "sfmloc_bow_knn: 4194305 views (at most 2^22)"),
            (dict(k=0xFFFFFFFF), capi.ECAP, "sfmloc_bow_knn: 5 views x k = 4294967295: more than 2^32 entries"),
            (dict(bow=big, n=1 << 22, dim=1, k=1025), capi.ECAP, "sfmloc_bow_knn: 4194304 views x k = 1025")):
        a = dict(bow=bow, n=5, dim=4, nbr=nbr, dist=dist, count=count, k=3)
        a.update(kw)
        rc, err = raw_call(a["bow"], a["n"], a["dim"], a["nbr"], a["dist"], a["count"], k=a["k"])
        assert rc == code and err.startswith(text), (kw.keys(), rc, err)
        for got, ref in zip((nbr, dist, count), filled(5, 3)):
            np.testing.assert_array_equal(got, ref)
    with pytest.raises(capi.SfmlocError) as e:
        capi.bow_knn(nan, 3)
    assert e.value.code == capi.EINVAL and e.value.message == "sfmloc_bow_knn: row 3 has a non-finite value"


@pytest.mark.parametrize("n,window", [(0, 0), (1, 0), (5, 4), (5, 7), (2, 1), (3, 0xFFFFFFFF)])
def test_nothing_to_launch(n, window):
    """n = 0, n = 1, window >= n - 1: SFMLOC_OK on a machine without a GPU, every count 0, every slot padding"""
    nbr, dist, count = capi.bow_knn(np.ones((n, 6), np.float32), 4, window=window, profile=True)
    assert nbr.shape == (n, 4) and dist.shape == (n, 4) and count.shape == (n,)
    assert (count == 0).all() and (nbr == PAD).all() and np.isposinf(dist).all()
    assert capi.bowknn_last_ms() == 0.0
    if n == 1:                                                   # a NULL options pointer is the defaults: k = 20
        out = filled(1, 20)
        assert raw_call(np.ones((1, 6), np.float32), 1, 6, *out, opt=False)[0] == capi.OK
        assert (out[2] == 0).all() and (out[0] == PAD).all() and np.isposinf(out[1]).all()


# ---- knn_pairs -------------------------------------------------------------------------------------------------------
IDS = [3, 10, 11, 40, 41, 97]                                    # not contiguous


def lists(rows, k):
    nbr = np.full((len(rows), k), PAD, np.uint32)
    for i, r in enumerate(rows):
        nbr[i, :len(r)] = r
    return nbr, np.array([len(r) for r in rows], np.uint32)


ROWS = [[1, 4], [0], [5], [2, 5], [0, 1], []]                    # 0<->1 and 0<->4 both ways; 1<-4, 2->5, 3->2, 3->5 one way


def test_knn_pairs_asymmetric_lists():
    nbr, count = lists(ROWS, 3)
    assert bowpairs.knn_pairs(IDS, nbr, count) == [(3, 10), (3, 41), (10, 41), (11, 40), (11, 97), (40, 97)]
    assert bowpairs.knn_pairs(IDS, nbr, count, mutual=True) == [(3, 10), (3, 41)]      # each found from both sides, once


def test_knn_pairs_reads_count_not_the_padding():
    nbr, count = lists(ROWS, 3)
    nbr[5, :] = [0, 1, 2]                                        # beyond count[5] = 0: not read
    count[3] = 1                                                 # row 3 keeps only its first entry
    assert bowpairs.knn_pairs(IDS, nbr, count) == [(3, 10), (3, 41), (10, 41), (11, 40), (11, 97)]


def test_knn_pairs_video_pairs_are_united_in_and_survive_mutual():
    nbr, count = lists(ROWS, 3)
    video = extfeat.generate_video_match_pairs(IDS, 2)
    assert (3, 11) in video and (41, 97) in video and len(video) == 9
    plain = bowpairs.knn_pairs(IDS, nbr, count, video_frame=2)
    assert plain == sorted(set(video) | {(3, 10), (3, 41), (10, 41), (11, 40), (11, 97), (40, 97)})
    mutual = bowpairs.knn_pairs(IDS, nbr, count, video_frame=2, mutual=True)
    assert mutual == sorted(set(video) | {(3, 41)}) and set(video) <= set(mutual)
    for got in (plain, mutual):
        assert all(a < b for a, b in got) and all(x < y for x, y in zip(got, got[1:]))    # strictly ascending


def test_pair_file_round_trip(tmp_path):
    nbr, count = lists(ROWS, 3)
    pairs = bowpairs.knn_pairs(IDS, nbr, count, video_frame=1)
    bowpairs.write_pair_file(tmp_path / "pairs.bow.txt", pairs)
    assert (tmp_path / "pairs.bow.txt").read_text().splitlines()[0] == "3 10"
    assert extfeat.read_pair_file(tmp_path / "pairs.bow.txt") == pairs


# ---- the tools' refusals ---------------------------------------------------------------------------------------------
def match_dir(path, dims):
    """a match directory of len(dims) views; view v has a .bow of dims[v] values (None: no file)"""
    path.mkdir()
    names = [f"frame{v:03d}.jpg" for v in range(len(dims))]
    fileio.write_sfm_data(path / "sfm_data.json", fileio.make_sfm_data([7 + 2 * v for v in range(len(dims))], names, 640, 480,
                                                                      500.0, 320.0, 240.0, root_path=str(path)))
    for v, (name, d) in enumerate(zip(names, dims)):
        if d is not None:                                        # (every other one as float32: both depths are read)
            fileio.write_mat_bin(path / (name[:-4] + ".bow"), np.linspace(0.0, 1.0, d).reshape(-1, 1).astype(np.float32 if v % 2 else np.float64))
    return path


def run_tool(which, args):
    cmd = [sys.executable, "-m", "sfmlocalization_amd.bowpairs"] if which == "py" else [EXE]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    return subprocess.run(cmd + [str(a) for a in args], capture_output=True, text=True, timeout=120, cwd=ROOT, env=env)


@pytest.mark.parametrize("which", ["py", "cc"])
def test_cli_refusals(tmp_path, which):
    missing = match_dir(tmp_path / "missing", [8, None, 8])
    mixed = match_dir(tmp_path / "mixed", [8, 8, 9])
    one = match_dir(tmp_path / "one", [8])
    short = match_dir(tmp_path / "short", [8, 8, 8, 8])
    (short / "frame003.bow").write_bytes((short / "frame003.bow").read_bytes()[:-5])       # the body ends early
    for d, names in ((missing, ["frame001.bow"]), (mixed, ["frame002.bow", "frame000.bow"]), (one, ["sfm_data.json"]),
                     (short, ["frame003.bow"])):
        r = run_tool(which, ["-m", d, "-k", 2])
        assert r.returncode == 1, (r.stdout, r.stderr)
        for name in names:
            assert str(d / name) in r.stderr, r.stderr
        assert not (d / "pairs.bow.txt").exists()
    for bad in (["-k", 2], ["-m", missing, "-k", 0], ["-m", missing, "-k"], ["-m", missing, "--nonsense", 1]):
        r = run_tool(which, bad)
        assert r.returncode == 1 and "Usage: ComputeBoWPairs" in r.stderr
