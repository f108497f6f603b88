"""CPU: the map merge (sfmlocalization_amd.merge) with its device calls served by the NumPy restatement (merge_np) --
against independent arithmetic (LAPACK closed forms, scipy's cKDTree) on planted scenes, and against what the
reference's own functions return on the documents of merge_scene (tests/golden/merge_ref/expected.json, minted by
tests/golden/make_merge_fixtures.py)."""
import copy
import json
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
from sfmlocalization_amd import capi, hulo, merge  # noqa: E402

SEED = int(capi.merge_default_params().seed)
# the largest |M - LAPACK| measured over the five planted scenes below (10 Jacobi sweeps); max |A| there is about 60,
# so 1e-9 max|A| = 6e-8 is far above: the sweeps are enough
DEV_SIMILARITY, DEV_AFFINE = 7.2e-15, 1.1e-14


@pytest.fixture(scope="module")
def ops():
    return MN.Ops(SEED)


@pytest.fixture(scope="module")
def ref():
    with open(os.path.join(HERE, "golden", "merge_ref", "expected.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def scene():
    return MS.make_docs()


def lapack_similarity(A, B):
    a0, b0 = A - A.mean(0), B - B.mean(0)
    U, _, Vt = np.linalg.svd(a0.T @ b0)
    R = U @ np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))]) @ Vt
    s = np.sqrt((a0 ** 2).sum() / (b0 ** 2).sum())
    return np.hstack([s * R, (A.mean(0) - s * R @ B.mean(0))[:, None]])


def lapack_affine(A, B):
    return np.linalg.lstsq(np.hstack([B, np.ones((len(B), 1))]), A, rcond=None)[0].T


@pytest.mark.parametrize("model", [MN.SIMILARITY, MN.AFFINE])
@pytest.mark.parametrize("seed", range(5))
def test_planted_scene(model, seed):
    """n = 48, 30 inliers, n x 100 rounds: the inlier set is the planted one (the reference's affine loop and a LAPACK
    similarity loop return exactly it on this scene), and the final M is the LAPACK closed form on that set to 100 x
    the deviation measured here: similarity 7.2e-15, affine 1.1e-14."""
    A, B, _, inl = MS.planted(seed)
    r = MN.ransac(A, B, MS.THRES, len(A) * 100, 1.75, model, SEED)
    np.testing.assert_array_equal(r["inliers"], inl)
    assert r["count"] == 30
    exp = lapack_similarity(A[inl], B[inl]) if model == MN.SIMILARITY else lapack_affine(A[inl], B[inl])
    dev = np.abs(r["M"] - exp).max()
    print(f"model {model} seed {seed}: |M - LAPACK| = {dev:.3g}, max|A| = {np.abs(A).max():.3g}")
    assert dev <= 100 * (DEV_SIMILARITY if model == MN.SIMILARITY else DEV_AFFINE)


def test_four_point_fits_are_the_closed_forms():
    A, B, _, _ = MS.planted(3, n=200, n_in=200, thres=0.0)
    M, ok, s = MN.round_models(A, B, SEED, 0, np.arange(64), MN.SIMILARITY, 1.75)
    Ma, oka, _ = MN.round_models(A, B, SEED, 0, np.arange(64), MN.AFFINE, 1.75)
    assert ok.all() and oka.all()
    assert (np.diff(s, axis=1) > 0).all() and s.min() >= 0 and s.max() < 200
    for k in range(64):
        assert np.abs(M[k].reshape(3, 4) - lapack_similarity(A[s[k]], B[s[k]])).max() <= 100 * DEV_SIMILARITY
        # (four points: the affine system is square, its conditioning sets the agreement)
        assert np.abs(Ma[k].reshape(3, 4) - lapack_affine(A[s[k]], B[s[k]])).max() <= 1e-9


def test_degenerate_samples_count_nothing():
    A, B, _, _ = MS.planted(1)
    B = B.copy()
    B[:, 2] = 0.0                            # coplanar: the 4-point affine system is singular (a zero pivot)
    _, ok, _ = MN.round_models(A, B, SEED, 0, np.arange(32), MN.AFFINE, 1e300)
    assert not ok.any()
    B[:] = B[0]                              # one point: no scale
    _, ok, _ = MN.round_models(A, B, SEED, 0, np.arange(32), MN.SIMILARITY, 1.75)
    assert not ok.any()


def test_ratio_test_sees_the_singular_values():
    rng = np.random.Generator(np.random.PCG64(1))
    for _ in range(20):
        L = MS.rotation(rng) @ np.diag(rng.uniform(0.5, 3.0, 3)) @ MS.rotation(rng)
        s = np.linalg.svd(L, compute_uv=False)
        M = [np.float64(x) for x in np.hstack([L, np.zeros((3, 1))]).ravel()]
        assert bool(MN.ratio_ok(M, s[0] / s[-1] * (1 + 1e-9)))
        assert not bool(MN.ratio_ok(M, s[0] / s[-1] * (1 - 1e-9)))


def kdtree_median(X):
    from scipy.spatial import cKDTree
    d, _ = cKDTree(X).query(X, 2)
    return float(np.median(d[:, 1]))


@pytest.mark.parametrize("n", [2, 3, 4, 257, 1000])
def test_median_against_kdtree(n):
    """relative 1e-12: a three-term sum and one square root differ by a few ulp between evaluations"""
    rng = np.random.Generator(np.random.PCG64(n))
    X = rng.uniform(-40, 40, (n, 3))
    assert MN.median_nn(X) == pytest.approx(kdtree_median(X), rel=1e-12)
    X[n // 2:] = X[:n - n // 2]
    assert MN.median_nn(X) == pytest.approx(kdtree_median(X), rel=1e-12, abs=0.0)


def test_threshold_functions(scene, ops):
    for doc in (scene["docA"], scene["docB"]):
        C = np.array([e["value"]["center"] for e in doc["extrinsics"]])
        X = np.array([s["value"]["X"] for s in doc["structure"]])
        assert merge.findMedianThres(doc, 2.5, ops=ops) == pytest.approx(2.5 * kdtree_median(C), rel=1e-12)
        assert merge.findMedianStructurePointsThres(doc, 2.5, ops=ops) == pytest.approx(2.5 * kdtree_median(X), rel=1e-12)
    one = dict(scene["docA"], extrinsics=scene["docA"]["extrinsics"][:1], structure=[])
    assert merge.findMedianThres(one, 2.5, ops=ops) == 0 and merge.findMedianStructurePointsThres(one, 2.5, ops=ops) == 0


# ---- against the reference's own functions -----------------------------------------------------------------------------

def matches_of(scene, tmp):
    pa, pb, loc = MS.write_docs(scene, str(tmp))
    names, pairs = hulo.read_match(loc)
    view_id = merge.imgname_to_view_id(names, scene["docB"])
    return view_id, merge.consistent_3d_match(view_id, pairs, scene["docB"])


def test_consistency_filter(scene, ref, tmp_path):
    view_id, match = matches_of(scene, tmp_path)
    assert view_id == ref["viewID"] and -1 in view_id                     # zz.jpg is not an image of model B
    assert set(map(tuple, match.tolist())) == set(map(tuple, ref["getConsistent3DMatch"]))
    assert (np.diff(match[:, 0]) > 0).all()                               # ascending B landmark id
    got = dict(match.tolist())
    assert got[300] == 200                                                # seen twice with the same A: kept
    assert 302 not in got                                                 # two different A: dropped
    assert 304 not in got and 306 not in got                              # two B on one A: both dropped
    assert 308 not in got and got[310] == 204                             # duplicate (view, feat): the later entry owns it
    assert len(match) == 50                                               # (feature 9999 has no landmark: no row)
    np.testing.assert_array_equal(match, scene["match"])


def close(a, b, path=""):
    """documents equal key by key, floats to relative 1e-12 (the reference's np.dot may fuse)"""
    if isinstance(b, dict):
        assert isinstance(a, dict) and sorted(a) == sorted(b), path
        for k in b:
            close(a[k], b[k], f"{path}/{k}")
    elif isinstance(b, list):
        assert isinstance(a, list) and len(a) == len(b), path
        for i, (x, y) in enumerate(zip(a, b)):
            close(x, y, f"{path}[{i}]")
    elif isinstance(b, float):
        assert isinstance(a, float) and a == pytest.approx(b, rel=1e-12, abs=0.0), path
    else:
        assert type(a) is type(b) and a == b, path


def test_inliers_merge_and_transform(scene, ref, ops):
    A, B, M = scene["A"], scene["B"], scene["M"]
    inl = ops.merge_inliers(A, B, M, MS.THRES)
    assert inl.tolist() == ref["getInliersByAffineTransform"]
    docA, docB = copy.deepcopy(scene["docA"]), copy.deepcopy(scene["docB"])
    match = scene["match"]
    merge.merge_sfm_data(docA, docB, M, {int(match[x, 0]): int(match[x, 1]) for x in inl}, ops=ops)
    close(json.loads(json.dumps(docA)), ref["merge_sfm_data"])
    moved = copy.deepcopy(scene["docB"])
    merge.transform_sfm_data(moved, M, ops=ops)
    close(json.loads(json.dumps(moved["extrinsics"])), ref["transform_sfm_data"]["extrinsics"])
    close([s["value"]["X"] for s in moved["structure"]], ref["transform_sfm_data"]["X"])


def test_reference_thresholds(scene, ref, ops):
    for name, doc in (("A", scene["docA"]), ("B", scene["docB"])):
        assert merge.findMedianThres(doc, 2.5, ops=ops) == pytest.approx(ref["findMedianThres"][name], rel=1e-12)
        assert merge.findMedianStructurePointsThres(doc, 2.5, ops=ops) == \
            pytest.approx(ref["findMedianStructurePointsThres"][name], rel=1e-12)


def test_reference_affine_ransac(scene, ref):
    """the reference's ransacAffineTransform (five seeds of `random`, n x 100 rounds): the same inlier set, and its
    lstsq M within the LAPACK bound of the normal-equation fit"""
    A, B = scene["A"], scene["B"]
    r = MN.ransac(A, B, MS.THRES, len(A) * 100, 1.75, MN.AFFINE, SEED)
    for run in ref["ransacAffineTransform"]:
        assert r["inliers"].tolist() == run["inliers"]
        assert np.abs(r["M"] - np.array(run["M"])).max() <= 100 * DEV_AFFINE


def test_model_merge_check_local(scene, ref, ops, tmp_path):
    pa, pb, loc = MS.write_docs(scene, str(tmp_path))
    out = str(tmp_path / "merged.json")
    n, k, M = merge.mergeModel(pa, pb, loc, out, MS.THRES, MS.THRES, ops=ops)
    assert (n, k) == (50, 31) and M.shape == (3, 4)
    # (the fixture's document was merged with the planted M, this one with the fitted M: centres differ by 1e-3)
    assert list(merge.modelMergeCheckLocal(out, loc, 1.0)) == ref["modelMergeCheckLocal"]


# ---- the gates of mergeModel (mergeSfM.py:560-591) -----------------------------------------------------------------------

def run(scene, tmp, ops, **kw):
    pa, pb, loc = MS.write_docs(scene, str(tmp))
    out = os.path.join(str(tmp), "out.json")
    kw.setdefault("ransacThres", MS.THRES)
    kw.setdefault("mergePointThres", MS.THRES)
    n, k, M = merge.mergeModel(pa, pb, loc, out, ops=ops, **kw)
    return n, k, M, os.path.exists(out)


def test_gate_four_matches(ops, tmp_path):
    n, k, M, written = run(MS.make_docs(n=2, n_in=2), tmp_path, ops)
    assert (n, k, M.size, written) == (4, 4, 0, False)


def test_gate_min_limit(scene, ops, tmp_path):
    n, k, M, written = run(scene, tmp_path, ops, minLimit=50)
    assert (n, k, M.size, written) == (50, 50, 0, False)


def test_gate_fewer_than_four_inliers(scene, ops, tmp_path):
    n, k, M, written = run(scene, tmp_path, ops, ransacThres=1e-9)     # no similarity fits 4 noisy points that well
    assert (n, k, M.size, written) == (50, 50, 0, False)


def test_gate_inliers_at_min_limit(scene, ops, tmp_path):
    n, k, M, written = run(scene, tmp_path, ops, minLimit=31)
    assert (n, k, M.shape, written) == (50, 31, (3, 4), False)
    n, k, M, written = run(scene, tmp_path, ops, minLimit=30, inputImgDir="/elsewhere")
    assert (n, k, M.shape, written) == (50, 31, (3, 4), True)
    with open(os.path.join(str(tmp_path), "out.json")) as fh:
        doc = json.load(fh)
    assert doc["root_path"] == "/elsewhere" and len(doc["views"]) == 9 and doc["views"][4]["key"] == 4


def test_gate_ratio(ops, tmp_path):
    """an anisotropic planted map (singular values 2.6, 1.3, 1.3: ratio 2), affine.  At svdRatio 1.75 every round near it
    fails the ratio test inside the RANSAC: what wins is a chance model with a handful of inliers (6 here), stopped by
    minLimit.  At 2.5 the merge goes through.  With svdRatio a hair under the final fit's own ratio, rounds whose
    4-point ratio is below it still win with the planted support, and the second gate (:590) stops the merge on the
    ratio of the refitted M."""
    scene = MS.make_docs(stretch=(1.0, 1.0, 2.0))
    n, k, M, written = run(scene, tmp_path, ops, model="affine", minLimit=10)
    assert (n, M.shape, written) == (50, (3, 4), False) and k <= 10
    n, k, M, written = run(scene, tmp_path, ops, model="affine", svdRatio=2.5)
    assert (n, k, written) == (50, 31, True)
    s = np.linalg.svd(M[:, :3], compute_uv=False)
    assert s[0] / s[-1] == pytest.approx(2.0, abs=1e-3)
    os.remove(os.path.join(str(tmp_path), "out.json"))
    cut = s[0] / s[-1] * (1 - 1e-12)
    n, k, M2, written = run(scene, tmp_path, ops, model="affine", svdRatio=cut)
    assert (n, k, written) == (50, 31, False)
    np.testing.assert_array_equal(M2, M)
