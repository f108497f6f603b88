"""GPU: the vocabulary trainer (sfmloc_bowtrain_*, sfmlocalization_amd.trainbow) against the NumPy restatement of its
stated arithmetic (tests/trainbow_np.py, include/sfmloc.h): exact PCA moments, bit-exact k-means on integer rows, the
assignment on float rows, determinism, the drawn dense rows, and the whole TrainBoW program on a small map."""
import os

import numpy as np
import pytest

import sfmlocalization_amd as S
import synthdata as synth
import trainbow_np as tnp
from sfmlocalization_amd import capi, engine, fileio, trainbow

pytestmark = pytest.mark.gpu


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _trainer(x, cap=None):
    tr = capi.BowTrainer(x.shape[1], cap or max(1, x.shape[0]))
    tr.add_rows(x)
    return tr


@pytest.mark.parametrize("case", ["full", "rank_deficient"])
def test_pca_moments_exact_and_eigen(case):
    rng = np.random.Generator(np.random.PCG64(3))
    x = rng.integers(0, 256, (5000, 61)).astype(np.float32)
    x[:, 7] = 42.0                                      # a constant column
    if case == "rank_deficient":
        x[:, 30:] = x[:, :31]                           # duplicated columns: rank 30
    with _trainer(x) as tr:
        mean, cov, evec, evals = tr.pca64()
        m32, v32, e32 = tr.pca()
    want_mean, want_cov = tnp.pca_moments(x)
    np.testing.assert_array_equal(bits(mean), bits(want_mean))
    np.testing.assert_array_equal(bits(cov), bits(want_cov))
    w, V = np.linalg.eigh(want_cov)
    w, V = w[::-1], V[:, ::-1]
    lmax = w[0]
    assert np.all(np.diff(evals) <= 0), "eigenvalues descending"
    np.testing.assert_allclose(evals, w, rtol=0, atol=1e-9 * lmax)
    # the sign rule: the largest-magnitude component of every eigenvector is positive
    for r in range(61):
        assert evec[r, np.argmax(np.abs(evec[r]))] > 0
    np.testing.assert_allclose(evec @ evec.T, np.eye(61), atol=1e-9)
    ref = tnp.sign_rule(V.T)
    for r in range(61):
        gap = min(abs(w[r] - w[r - 1]) if r else np.inf, abs(w[r] - w[r + 1]) if r < 60 else np.inf)
        if gap > 1e-6 * lmax:                           # (a repeated eigenvalue's vectors are only a basis of its space)
            np.testing.assert_allclose(evec[r], ref[r], rtol=0, atol=max(1e-9, 1e-13 * lmax / gap))
    np.testing.assert_allclose(cov @ evec.T, evec.T * evals[None, :], atol=1e-9 * lmax)
    np.testing.assert_array_equal(m32.ravel(), mean.astype(np.float32))
    np.testing.assert_array_equal(v32, evec.astype(np.float32))
    np.testing.assert_array_equal(e32.ravel(), evals.astype(np.float32))


@pytest.mark.parametrize("data", ["small_ints", "float"])
def test_one_lloyd_step_bit_exact(data):
    rng = np.random.Generator(np.random.PCG64(8))
    if data == "small_ints":
        x = rng.integers(0, 4, (3000, 8)).astype(np.float32)     # exact ties everywhere
    else:
        x = (rng.normal(size=(3000, 32)) * 3).astype(np.float32)
        x[1000:1100] = x[0]                                       # planted duplicates: tied distances
    st = {}
    with _trainer(x) as tr:
        c, lab, comp = tr.kmeans(25, attempts=1, max_iter=2, stats=st)
    wc, wl, wcomp, wmind = tnp.kmeans(x, 25, attempts=1, max_iter=2, want_min_dist=True)
    assert st["iterations"] == 1
    np.testing.assert_array_equal(bits(st["min_dist"]), bits(wmind))
    np.testing.assert_array_equal(lab, wl)
    np.testing.assert_array_equal(bits(c), bits(wc))
    assert comp == wcomp


@pytest.mark.parametrize("shape", [(2500, 61, 100), (50, 8, 100), (3000, 32, 20), (1200, 16, 12)])
def test_kmeans_bit_exact_on_integer_rows(shape):
    n, d, K = shape
    rng = np.random.Generator(np.random.PCG64(n + d))
    x = rng.integers(0, 256, (n, d)).astype(np.float32)
    if n == 3000:
        x[500:900] = x[7]                                          # duplicate rows
    trace = []
    if n == 1200:                                                  # 6 distinct rows, 12 clusters: the empty rule fires
        x = np.repeat(rng.integers(0, 256, (6, d)), 200, 0).astype(np.float32)[rng.permutation(1200)]
    with _trainer(x) as tr:
        c, lab, comp = tr.kmeans(K)
        c2, lab2, comp2 = tr.kmeans(K)
    wc, wl, wcomp = tnp.kmeans(x, K, trace=trace)
    assert c.shape == (min(K, n), d)
    np.testing.assert_array_equal(bits(c), bits(wc))
    np.testing.assert_array_equal(lab, wl)
    assert comp == wcomp
    np.testing.assert_array_equal(bits(c2), bits(c))
    np.testing.assert_array_equal(lab2, lab)
    if n == 1200:
        assert trace, "the empty-cluster rule was not exercised"
        assert sorted(set(lab.tolist())) == list(range(K))


def test_projected_kmeans_deterministic_and_close_to_restatement():
    rng = np.random.Generator(np.random.PCG64(21))
    x = rng.integers(0, 256, (4000, 61)).astype(np.float32)
    with _trainer(x) as tr:
        mean, evec, evals = tr.pca()
        tr.project(mean, evec, evals, 32)
        assert tr.size() == (4000, 32)
        y = tr.read()
        c1, l1, k1 = tr.kmeans(100)
        c2, l2, k2 = tr.kmeans(100)
    # the projection is bow.hip's arithmetic: sequential f32, then the division
    want = np.zeros((4000, 32), np.float32)
    for dd in range(32):
        acc = np.zeros(4000, np.float32)
        for i in range(61):
            acc = acc + (x[:, i] - mean[0, i]) * evec[dd, i]
        want[:, dd] = acc / evals[dd, 0]
    np.testing.assert_array_equal(bits(y), bits(want))
    np.testing.assert_array_equal(bits(c1), bits(c2))
    np.testing.assert_array_equal(l1, l2)
    assert k1 == k2
    wc, wl, wk = tnp.kmeans(y, 100)
    np.testing.assert_allclose(c1, wc, rtol=1e-5, atol=1e-5 * np.abs(wc).max())


def test_planted_blobs_recovered_as_a_partition():
    rng = np.random.Generator(np.random.PCG64(4))
    cen = rng.normal(size=(100, 32)).astype(np.float32) * 100
    blob = np.repeat(np.arange(100), 30)
    x = (cen[blob] + rng.normal(size=(3000, 32)).astype(np.float32) * 0.5).astype(np.float32)
    with _trainer(x) as tr:
        _, lab, _ = tr.kmeans(100)
    pairs = set(zip(blob.tolist(), lab.tolist()))
    assert len(pairs) == 100 and len({b for b, _ in pairs}) == 100 and len({l for _, l in pairs}) == 100


def test_add_image_rows_equal_the_oracle_at_the_restated_draws(oracle_c):
    imgs = []
    for k, (h, w) in enumerate([(240, 320), (300, 300), (240, 320)]):
        g = synth.texture_image(400 + k, h, w, n_blobs=500, n_rects=80)
        imgs.append(np.stack([g, np.roll(g, 2, 1), g // 2 + 40], 2))
    grid = engine.dense_grid_keypoints(300)
    rng = tnp.CvRng()
    want = []
    with capi.BowTrainer(61, 1000) as tr:
        for k, img in enumerate(imgs + [imgs[2]]):                # the last one: the same image again (cached)
            state0 = rng.state
            picks = [tnp.draw_index(len(grid), rng.uniform01()) for _ in range(60)]
            od, _ = oracle_c.akaze_compute(oracle_c.dense_gray(img, 300), grid)
            want.append(od[picks, :61].astype(np.float32))
            assert tr.add_image(img, 60, state0) == rng.state
        # an image without descriptors: zero rows, no draws
        assert tr.add_image(None, 40, 777) == 777
        got = tr.read()
    assert got.shape == (280, 61)
    np.testing.assert_array_equal(got[:240], np.concatenate(want))
    assert not got[240:].any()


F, W, H, PPM = 800.0, 640, 480, 100.0
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin")


@pytest.fixture(scope="module")
def plane_map(tmp_path_factory):
    """A textured plane seen from 16 known poses; the map (features, landmarks, sfm_data.json) is extracted from the
    rendered views by the AKAZE kernels and written in the reference's layout, images and all, into <root>/matches;
    three held-out query frames from new poses."""
    from PIL import Image
    root = tmp_path_factory.mktemp("trainmap")
    mdir = root / "matches"
    rng = np.random.Generator(np.random.PCG64(3))
    tex = synth.texture_image(7, 1600, 1600, n_blobs=3000, n_rects=900)
    centres = [(x, y) for x in (4.5, 6.8, 9.2, 11.5) for y in (4.5, 6.8, 9.2, 11.5)]
    ak = S.Akaze(W, H)
    views, view_off, desc_all, kp_all, X_all = [], [0], [], [], []
    for cxy in centres:
        R, C = synth.plane_camera(rng, cxy, 10.0, tilt=0.15)
        img = synth.render_plane_view(tex, PPM, R, C, F, W, H)
        kp, desc = ak.detect_and_compute(img)
        views.append((R, C, img))
        desc_all.append(desc)
        kp_all.append(synth.round6(kp[:, :2]))
        X_all.append(synth.backproject_to_plane(kp[:, :2].astype(np.float64), R, C, F, W, H))
        view_off.append(view_off[-1] + len(desc))
    ak.close()
    n, nv = view_off[-1], len(centres)
    m = synth.SynthMap(view_id=np.arange(nv, dtype=np.uint32), view_off=np.array(view_off, np.uint32),
                       view_wh=np.tile(np.array([[W, H]], np.uint32), (nv, 1)), desc=np.concatenate(desc_all),
                       kpt_xy=np.concatenate(kp_all), row_landmark=np.arange(n, dtype=np.int32),
                       landmark_id=np.arange(n, dtype=np.uint32) + 1000, landmark_X=np.concatenate(X_all),
                       landmark_desc=np.zeros((0, 64), np.uint8), landmark_place=np.zeros(n, np.int64),
                       view_place=np.zeros(nv, np.int64), view_R=np.stack([v[0] for v in views]),
                       view_C=np.stack([v[1] for v in views]), place_center=np.zeros((1, 3)),
                       intrinsic=(F, W / 2.0, H / 2.0), width=W, height=H)
    names = synth.write_map_to_disk(m, str(mdir), str(mdir))
    for name, (_, _, img) in zip(names, views):                  # the images sfm_data.json names (root_path = mdir)
        Image.fromarray(np.stack([img, img, img], 2)).save(mdir / f"{name}.jpg", quality=95)
    qdir = root / "q"
    qdir.mkdir()
    truth = {}
    for k in range(3):
        R, C = synth.plane_camera(rng, (5.5 + 2.0 * k, 10.5 - 2.0 * k), 9.5 + 0.5 * k, tilt=0.12)
        Image.fromarray(synth.render_plane_view(tex, PPM, R, C, F, W, H)).save(qdir / f"query{k}.png")
        truth[f"query{k}"] = (R, C)
    return root, names, truth


@pytest.mark.parametrize("with_pca", [True, False])
def test_trainbow_programs_end_to_end(plane_map, oracle_c, with_pca, tmp_path):
    import json
    import subprocess
    root, names, truth = plane_map
    mdir = root / "matches"
    bow, pca = str(tmp_path / "BOWfile.yml"), str(tmp_path / "PCAfile.yml")
    popt = [f"-p={pca}"] if with_pca else []
    # the Python program, then the C++ one: the same bytes in every file
    assert trainbow.main([str(root), bow] + popt) == 0
    files = [bow] + ([pca] if with_pca else []) + [str(mdir / f"{n}.bow") for n in names]
    first = {f: open(f, "rb").read() for f in files}
    for f in files:
        os.remove(f)
    r = subprocess.run([os.path.join(BIN, "TrainBoW"), str(root), bow] + popt, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for f in files:
        assert open(f, "rb").read() == first[f], f
    b = fileio.read_cv_yaml(bow)
    assert b["K"] == 100 and b["ResizedImageSize"] == 300 and b["NormBofFeatureType"] == "L1"
    assert b["Centers"].shape == (100, 32 if with_pca else 61)
    p = fileio.read_cv_yaml(pca) if with_pca else None
    if with_pca:
        assert p["DimPCA"] == 32 and p["EigenVectorsPCA"].shape == (61, 61) and p["EigenValuesPCA"].shape == (61, 1)
        assert p["MeanPCA"].shape == (1, 61)
    model = S.BofModel.from_files(bow, pca if with_pca else None)
    assert model.dim == 500
    model.close()
    # each .bow is the reference chain of its view under the trained model
    grid = engine.dense_grid_keypoints(300)
    kw = dict(pca_mean=p["MeanPCA"], pca_eigvec=p["EigenVectorsPCA"], pca_eigval=p["EigenValuesPCA"],
              n_pca=32) if with_pca else {}
    for n in (names[0], names[9]):
        vec = fileio.read_mat_bin(mdir / f"{n}.bow")
        assert vec.shape == (500, 1) and vec.dtype == np.float64
        img = capi.image_read(str(mdir / f"{n}.jpg"), color=True)
        od, _ = oracle_c.akaze_compute(oracle_c.dense_gray(img, 300), grid)
        want = oracle_c.bof(od[:, :61].astype(np.float32), grid[:, :2].copy(), b["Centers"], 300, 2, 2, **kw)
        np.testing.assert_array_equal(bits(vec.ravel()), bits(want))
    # the localiser with the trained vocabulary: a BoW shortlist of 4 of the 16 views, held-out frames on their poses
    out = tmp_path / "out"
    r = subprocess.run([os.path.join(BIN, "OpenMVGLocalization_AKAZE"), str(root / "q"), str(mdir), str(mdir), str(out),
                        "-r=25", "-k=4", f"-a={bow}"] + popt, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    n_ok = 0
    for name, (R, C) in truth.items():
        d = json.load(open(out / (name + ".json")))
        if "t" in d and np.abs(np.array(d["t"]) - C).max() < 0.2 and np.abs(np.array(d["R"]) - R).max() < 0.03:
            n_ok += 1
    assert n_ok >= 2, n_ok
