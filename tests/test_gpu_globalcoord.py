"""python -m sfmlocalization_amd.globalcoord end to end on the device against the same command driven by the NumPy twin
(globalcoord_np.Ops): the files are compared as bytes.  Then the chain the step exists for: the Amat.yml it writes,
handed to LocalizeEngine, gives the world pose its own loc_global.json holds."""
import json
import os
import shutil
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import globalcoord_np as GN  # noqa: E402
import globalcoord_scene as GS  # noqa: E402
import synthdata as synth  # noqa: E402
from sfmlocalization_amd import capi, engine, fileio, globalcoord, hulo  # noqa: E402

pytestmark = pytest.mark.gpu
SEED = int(capi.merge_default_params().seed)
GOLD = os.path.join(HERE, "golden", "ref_consumers")
QUIET = dict(log=lambda s: None)


def read(path):
    with open(path, "rb") as fh:
        return fh.read()


@pytest.mark.parametrize("model", ["similarity", "affine"])
def test_ref_points_route_equals_the_twin(tmp_path, model):
    doc, A = GS.reduce_scenes()["clusters"][:2]
    refs = GS.ref_points(doc, A)                                # 6 reference landmarks, 1 an outlier
    out = {}
    for who, ops in (("dev", None), ("np", GN.Ops(SEED))):
        proj, matches, sfm = GS.write_project(str(tmp_path / who), doc, refs)
        assert globalcoord.main([proj, matches, sfm, "--ref-points", "--reduce-points", "--model=" + model], ops=ops) == 0
        out[who] = {n: read(os.path.join(d, n)) for d, n in ((proj + "/Ref", "Amat.txt"), (proj + "/Ref", "Amat.yml"),
                                                             (sfm, "sfm_data_global.json"), (sfm, "sfm_data.json"),
                                                             (sfm, "sfm_data_b4rp.json"))}
    assert out["dev"] == out["np"]
    assert len(json.loads(out["dev"]["sfm_data.json"])["structure"]) == 41 < len(doc["structure"])


def recorded_frames(folder):
    """the recorded result files of the localiser in one folder -> how many have a pose"""
    n = 0
    for sub in ("loc_cli", "loc_fileio"):
        for name in sorted(os.listdir(os.path.join(GOLD, sub))):
            shutil.copy(os.path.join(GOLD, sub, name), os.path.join(folder, name))
            n += "t" in hulo.load_json(os.path.join(folder, name))
    return n


def test_image_route_from_recorded_results(tmp_path):
    A = GS.amat()
    assert recorded_frames(str(tmp_path)) >= 4
    lines = []
    for name in sorted(os.listdir(tmp_path)):
        r = hulo.load_json(str(tmp_path / name))
        if "t" in r:
            w = GS.world(r["t"], A)
            lines.append(os.path.basename(r["filename"]) + " " + " ".join(repr(float(v)) for v in w))
    lines.append("not_localised.jpg 1.0 2.0 3.0")
    lines.append("broken.jpg 1.0 2.0")
    (tmp_path / "refcoor.txt").write_text("\n".join(lines) + "\n")
    names = globalcoord.load_image_locations(str(tmp_path / "refcoor.txt"))
    world, loc = globalcoord.image_correspondences(str(tmp_path), names)
    assert len(world) == len(lines) - 2 >= 4
    thres = hulo.ReconstructParam.ransacThresTransformWorldCoordinateRefImage
    dev, inl_d = globalcoord.fit_world_transform(world, loc, thres, **QUIET)
    ref, inl_n = globalcoord.fit_world_transform(world, loc, thres, ops=GN.Ops(SEED), **QUIET)
    assert dev.tobytes() == ref.tobytes() and inl_d.tolist() == inl_n.tolist() == list(range(len(world)))
    # fewer than 4 pairs: the message and no model
    said = []
    got, _ = globalcoord.fit_world_transform(world[:3], loc[:3], thres, log=said.append)
    assert got is None and "less than 4 reference points" in said[0]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    """a 30-view map on disk, a project whose reference points are 8 of its landmarks (1 an outlier) and a test folder
    of three queries with precomputed features, the last of which cannot be localised"""
    root = tmp_path_factory.mktemp("globalcoord")
    m = synth.make_map(1, n_views=30, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=130)
    synth.write_map_to_disk(m, str(root / "sfm"), str(root / "matches"))
    A = GS.amat(seed=4, scale=1.7)
    doc = hulo.load_json(str(root / "sfm" / "sfm_data.json"))
    os.makedirs(root / "proj" / "Ref")
    with open(root / "proj" / "Ref" / "refpoints.json", "w") as fh:
        json.dump(GS.ref_points(doc, A, n=8, outliers=(5,)), fh)
    qdir = root / "tests" / "walk1" / "inputImg"
    os.makedirs(qdir)
    (root / "tests" / "notes").mkdir()                          # a folder without inputImg is skipped
    for k in range(3):
        q = synth.make_query(m, 50 + k, n_feat=500, n_copies=180, place=k % 3) if k < 2 else \
            synth.make_query(m, 99, n_feat=300, n_copies=0)
        fileio.write_desc(qdir / f"q{k}.desc", q.desc)
        fileio.write_feat(qdir / f"q{k}.feat", np.concatenate([q.kpt_xy, np.zeros((len(q.kpt_xy), 2), np.float32)], 1))
        (qdir / f"q{k}.jpg").write_bytes(b"")
    return root, A


def test_amat_yml_serves_world_poses(toy):
    root, A = toy
    sfm, matches = str(root / "sfm"), str(root / "matches")
    assert globalcoord.main([str(root / "proj"), matches, sfm, "--ref-points", "-t", str(root / "tests")]) == 0
    got = np.loadtxt(str(root / "proj" / "Ref" / "Amat.txt"))
    loc_dir = root / "tests" / "walk1" / "loc"
    glob = hulo.load_json(str(loc_dir / "loc_global.json"))["locGlobal"]
    assert [("t" in r) for r in glob] == [True, True, False]
    assert (loc_dir / "center.txt").read_text().count("\n") == 2
    log = (root / "tests" / "log.txt").read_text()
    assert "number of localized frame : 3/3" in log and "total result" in log
    A3 = got[:, :3]
    s = np.cbrt(np.linalg.det(A3))
    eng = engine.LocalizeEngine(sfm, matches, str(root / "proj" / "Ref" / "Amat.yml"))
    try:
        np.testing.assert_array_equal(eng.A, got)
        for k, r in enumerate(glob[:2]):
            qdir = root / "tests" / "walk1" / "inputImg"
            desc, kp = fileio.read_desc(qdir / f"q{k}.desc"), fileio.read_feat(qdir / f"q{k}.feat")[:, :2]
            res, _ = eng.localize(desc, kp, 640, 480)
            assert len(res) == 12
            # the file holds the pose to 6 significant digits: the world centre agrees to that, through |A|
            tol = 1e-5 * max(1.0, np.abs(r["t_relative"]).max()) * np.abs(A3).sum(1).max()
            np.testing.assert_allclose(res[:3], r["t"], rtol=0, atol=tol)
            assert r["t"] == np.dot(got, np.concatenate([r["t_relative"], [1]])).tolist()
            # (the engine serves a rotation, A[:, :3] / s; loc_global keeps the reference's R A[:, :3]^T)
            np.testing.assert_allclose(np.array(res[3:]).reshape(3, 3), np.array(r["R"]) / s, rtol=0, atol=1e-5 * 3)
            # and the pose is where the planted map says, to the noise of the reference points
            np.testing.assert_allclose(r["t"], GS.world(r["t_relative"], A), rtol=0, atol=0.05)
    finally:
        eng.close()
