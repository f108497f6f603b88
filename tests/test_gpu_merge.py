"""mergeSfM.mergeModel's device half (sfmloc_merge_*, csrc/merge.hip) against its NumPy restatement (merge_np): every
comparison is on bits.  The RANSAC's winning round, its count, the ascending inlier list and the final M for both
models at n = 5 (the smallest past the gate), 48 (the planted scene) and 5 000 (more than one LDS tile whatever the tile,
no multiple of 64); rounds that are no multiple of a wave; ties; a match with a missing (inf) point; the caps; the
independence of the launch geometry; the median, the transform, and mergeModel end to end into adjust.run."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import merge_np as MN  # noqa: E402
import merge_scene as MS  # noqa: E402
from sfmlocalization_amd import adjust, merge  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = int(S.merge_default_params().seed)
CASES = {"n5": (dict(seed=3, n=5, n_in=4), 500), "n48": (dict(seed=7), 4800),
         "n5000": (dict(seed=9, n=5000, n_in=3000), 4096), "r130": (dict(seed=5), 130)}
RATIO = {MN.SIMILARITY: 1.75, MN.AFFINE: 1.75}


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same(dev, ref):
    assert (dev["round"], dev["count"]) == (ref["round"], ref["count"])
    np.testing.assert_array_equal(dev["inliers"], ref["inliers"])
    assert (dev["M"] is None) == (ref["M"] is None)
    if ref["M"] is not None:
        np.testing.assert_array_equal(bits(dev["M"]), bits(ref["M"]))


@pytest.fixture(scope="module")
def refs():
    """the twin's answer for every (case, model), computed once"""
    out = {}
    for name, (kw, rounds) in CASES.items():
        A, B, _, inl = MS.planted(**kw)
        for model in (MN.SIMILARITY, MN.AFFINE):
            out[name, model] = (A, B, inl, MN.ransac(A, B, MS.THRES, rounds, RATIO[model], model, SEED, want_counts=True))
    return out


@pytest.mark.parametrize("model", [MN.SIMILARITY, MN.AFFINE])
@pytest.mark.parametrize("name", list(CASES))
def test_ransac_matches_twin(refs, name, model):
    A, B, inl, ref = refs[name, model]
    dev = S.merge_ransac(A, B, MS.THRES, CASES[name][1], RATIO[model], model)
    same(dev, ref)
    assert ref["count"] >= 4 and dev["M"] is not None
    if name in ("n48", "n5000"):
        np.testing.assert_array_equal(dev["inliers"], inl)      # the planted set


@pytest.mark.parametrize("model", [MN.SIMILARITY, MN.AFFINE])
def test_tie_goes_to_the_lower_round(refs, model):
    A, B, _, ref = refs["n48", model]
    top = np.nonzero(ref["counts"] == ref["counts"].max())[0]
    assert len(top) >= 2, "the scene must have two rounds with the winning count"
    dev = S.merge_ransac(A, B, MS.THRES, CASES["n48"][1], RATIO[model], model)
    assert dev["round"] == top[0] and dev["count"] == ref["counts"].max()


@pytest.mark.parametrize("model", [MN.SIMILARITY, MN.AFFINE])
def test_missing_point_is_never_an_inlier(model):
    A, B, _, inl = MS.planted(seed=7)
    A, B = A.copy(), B.copy()
    A[inl[0]] = np.inf                      # get3DPointloc: an id model A does not have
    B[inl[5]] = np.inf
    ref = MN.ransac(A, B, MS.THRES, 2000, RATIO[model], model, SEED, want_counts=True)
    samples = MN.sample4(len(A), SEED, 0, np.arange(2000))
    hit = np.isin(samples, [inl[0], inl[5]]).any(1)
    assert hit.any() and not ref["counts"][hit].any()           # a sample that contains it counts nothing
    dev = S.merge_ransac(A, B, MS.THRES, 2000, RATIO[model], model)
    same(dev, ref)
    np.testing.assert_array_equal(dev["inliers"], np.delete(inl, [0, 5]))


def test_small_and_caps():
    A, B, _, _ = MS.planted(seed=1, n=3, n_in=3)
    dev = S.merge_ransac(A, B, MS.THRES, 300, 1.75)
    assert dev["M"] is None and dev["count"] == 0 and len(dev["inliers"]) == 0
    res = S.MergeResult()
    L = S._L()
    for n, rounds in (((1 << 24) + 1, 100), (48, 1 << 32)):     # refused before anything is touched: null pointers
        rc = L.sfmloc_merge_ransac(None, None, n, 0.5, rounds, 1.75, 0, 0, None, C.byref(res), None, 0)
        assert rc == S.ECAP
    out = C.c_double(1.0)
    assert L.sfmloc_merge_median_nn(None, (1 << 24) + 1, None, C.byref(out)) == S.ECAP
    with pytest.raises(S.SfmlocError) as e:
        S.merge_ransac(A, B, MS.THRES, 300, 1.75, model=2)
    assert e.value.code == S.EINVAL


@pytest.mark.parametrize("model", [MN.SIMILARITY, MN.AFFINE])
def test_launch_geometry_does_not_matter(refs, model):
    A, B, _, ref = refs["n5000", model]
    got = []
    for per in (256, 0, 256, 0):
        dev = S.merge_ransac(A, B, MS.THRES, CASES["n5000"][1], RATIO[model], model,
                             params=S.merge_default_params(rounds_per_launch=per))
        got.append((dev["round"], dev["count"], dev["inliers"].tobytes(), dev["M"].tobytes()))
    assert got[0] == got[1] == got[2] == got[3]
    assert got[0][3] == ref["M"].tobytes()


def test_stream_selects_the_samples(refs):
    A, B, _, _ = refs["r130", MN.SIMILARITY]
    dev = S.merge_ransac(A, B, MS.THRES, 130, 1.75, stream=9)
    same(dev, MN.ransac(A, B, MS.THRES, 130, 1.75, MN.SIMILARITY, SEED, stream=9))


def test_inliers_of_a_given_model(refs):
    A, B, _, ref = refs["n5000", MN.AFFINE]
    for thres in (MS.THRES, 1e-3, 50.0):
        exp = np.nonzero(MN.inlier_mask(A, B, ref["M"].reshape(12), thres))[0]
        np.testing.assert_array_equal(S.merge_inliers(A, B, ref["M"], thres), exp)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 1025, 1026, 4099])
def test_median_nn(n):
    rng = np.random.Generator(np.random.PCG64(100 + n))
    X = rng.uniform(-50, 50, (n, 3))
    assert bits(S.merge_median_nn(X)) == bits(MN.median_nn(X))
    if n >= 4:                              # duplicated points: their distance is 0
        X[n // 2:] = X[:n - n // 2]
        got = S.merge_median_nn(X)
        assert bits(got) == bits(MN.median_nn(X))
        assert got == 0.0


def test_median_nn_refuses_non_finite():
    X = np.zeros((5, 3))
    for bad in (np.inf, np.nan):
        X[3, 1] = bad
        with pytest.raises(S.SfmlocError) as e:
            S.merge_median_nn(X)
        assert e.value.code == S.EINVAL


def test_transform():
    rng = np.random.Generator(np.random.PCG64(5))
    M = MS.planted(seed=2)[2]
    R = np.stack([MS.rotation(rng) for _ in range(7)])
    X = rng.uniform(-100, 100, (1001, 3))
    Rd, Xd = S.merge_transform(M, R, X)
    Rn, Xn = MN.transform(M, R, X)
    np.testing.assert_array_equal(bits(Rd), bits(Rn))
    np.testing.assert_array_equal(bits(Xd), bits(Xn))
    Rd, Xd = S.merge_transform(M, None, X[:1])
    assert Rd.shape == (0, 3, 3) and bits(Xd).tolist() == bits(Xn[:1]).tolist()


@pytest.mark.parametrize("model", ["similarity", "affine"])
def test_merge_model_end_to_end(tmp_path, model):
    scene = MS.make_docs()
    pa, pb, loc = MS.write_docs(scene, str(tmp_path))
    out_dev, out_np = str(tmp_path / "merged_dev.json"), str(tmp_path / "merged_np.json")
    ratio = 1.75
    got = merge.mergeModel(pa, pb, loc, out_dev, MS.THRES, MS.THRES, model=model, svdRatio=ratio, inputImgDir="/merged")
    exp = merge.mergeModel(pa, pb, loc, out_np, MS.THRES, MS.THRES, model=model, svdRatio=ratio, inputImgDir="/merged",
                           ops=MN.Ops(SEED))
    assert got[:2] == exp[:2] == (50, 31)
    np.testing.assert_array_equal(bits(got[2]), bits(exp[2]))
    with open(out_dev, "rb") as a, open(out_np, "rb") as b:
        assert a.read() == b.read()
    for fn in (merge.findMedianThres, merge.findMedianStructurePointsThres):
        assert bits(fn(scene["docA"], 2.5)) == bits(fn(scene["docA"], 2.5, ops=MN.Ops(SEED)))
    # the chain the merge loop runs next: OpenMVG_BA on the merged file
    assert adjust.run(out_dev, str(tmp_path / "adjusted.json"), log=lambda s: None) == 0
