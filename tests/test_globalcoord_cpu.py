"""sfmlocalization_amd.globalcoord on the host: its document functions driven by the NumPy twin (globalcoord_np.Ops)
against what the reference's own functions returned on the same documents (tests/golden/globalcoord_ref, minted by
tests/golden/make_globalcoord_fixtures.py), the bytes of the files it writes, the parameter pins and the command line."""
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

import globalcoord_np as GN  # noqa: E402
import globalcoord_scene as GS  # noqa: E402
from sfmlocalization_amd import fileio, globalcoord, hulo  # noqa: E402

GOLD = os.path.join(HERE, "golden")
with open(os.path.join(GOLD, "globalcoord_ref", "expected.json")) as _fh:
    EXP = json.load(_fh)
SCENES = GS.reduce_scenes()
OPS = GN.Ops(1)


def summary(doc):
    return [[s["key"], [[ob["key"], ob["value"]["id_feat"]] for ob in s["value"]["observations"]]] for s in doc["structure"]]


@pytest.mark.parametrize("name", list(SCENES))
def test_reduce_equals_the_reference(name):
    doc, A, thres, knn, binds = SCENES[name]
    d = copy.deepcopy(doc)
    res = globalcoord.reduce_close_points(d, A, thres, knn, ops=OPS)
    assert summary(d) == EXP["reduce"][name]["kdtree"]          # keeper keys in order, observation lists in order
    assert res["n_absorbed"] == len(doc["structure"]) - len(d["structure"]) > 0
    if not binds:
        assert [k for k, _ in summary(d)] == [k for k, _ in EXP["reduce"][name]["brute"]]
    else:                                                       # the cut list keeps more than the uncut one would
        u = copy.deepcopy(doc)
        globalcoord.reduce_close_points(u, A, thres, 1000, ops=OPS)
        assert len(u["structure"]) < len(d["structure"])


def test_chain_is_not_transitive():
    doc, A, thres, knn, _ = SCENES["chain"]
    res = GN.reduce_points([s["value"]["X"] for s in doc["structure"]], A, thres, knn)
    assert res["owner"].tolist() == [0, 0, 2, 2, 4, 4, 6] and res["rounds"] == 7


def test_file_bytes(tmp_path):
    A = np.array(EXP["Amat"])
    txt, yml = globalcoord.write_amat(str(tmp_path), A)
    assert open(txt).read() == EXP["Amat.txt"] and open(yml).read() == EXP["Amat.yml"]
    back = fileio.read_cv_yaml(yml)["A"]
    assert back.shape == (3, 4) and back.tobytes() == A.tobytes() == np.loadtxt(txt).tobytes()


def test_save_global_sfm(tmp_path):
    doc, A = SCENES["clusters"][:2]
    proj, _, sfm = GS.write_project(str(tmp_path), doc)
    txt, _ = globalcoord.write_amat(os.path.join(proj, "Ref"), A)
    out = os.path.join(sfm, "sfm_data_global.json")
    globalcoord.save_global_sfm(os.path.join(sfm, "sfm_data.json"), txt, out, ops=OPS)
    got, exp = hulo.load_json(out), EXP["saveGlobalSfM"]
    # np.dot against the header's unfused sum of four terms of magnitude <= |A| |X| ~ 200: a few units of 2^-53 x 200
    tol = 1e-13
    for g, e in zip(got["extrinsics"], exp["extrinsics"]):
        assert g["key"] == e["key"]
        np.testing.assert_allclose(g["value"]["center"], e["value"]["center"], rtol=0, atol=tol)
        np.testing.assert_allclose(g["value"]["rotation"], e["value"]["rotation"], rtol=0, atol=tol)
    np.testing.assert_allclose([s["value"]["X"] for s in got["structure"]], exp["X"], rtol=0, atol=tol)
    for k in ("views", "intrinsics", "root_path"):
        assert got[k] == doc[k]


def test_loc_global_arithmetic():
    A = np.array(EXP["Amat"])
    folder = os.path.join(GOLD, "ref_consumers", "loc_cli")
    names = sorted(os.listdir(folder))
    assert len(names) == len(EXP["loc_global"]) == 4
    n_failed = 0
    for name, exp in zip(names, EXP["loc_global"]):
        src = hulo.load_json(os.path.join(folder, name))
        got = globalcoord.to_global(copy.deepcopy(src), A)
        if "t" not in src:
            assert got == src and exp == {}
            n_failed += 1
            continue
        assert {k: got[k] for k in exp} == exp
        assert got["t_relative"] == src["t"] and got["pair"] == src["pair"]
    assert n_failed == 1


def test_parameter_pins():
    with open(os.path.join(GOLD, "ref_params.json")) as fh:
        ref = json.load(fh)["ReconstructParam"]
    for k in ("ransacThresTransformWorldCoordinateRefImage", "ransacThresTransformWorldCoordinateRefPoint"):
        assert getattr(hulo.ReconstructParam, k) == ref[k]
    assert (hulo.ReconstructParam.ransacThresTransformWorldCoordinateRefImage,
            hulo.ReconstructParam.ransacThresTransformWorldCoordinateRefPoint) == (0.3, 0.1)
    assert (globalcoord.REDUCE_THRES, globalcoord.REDUCE_KNN, globalcoord.RANSAC_ROUNDS) == (0.01, 1000, 1000)


def test_arguments_and_refusals(tmp_path, capsys):
    a = globalcoord.parse_args(["p", "m", "s"])
    assert (a.project_dir, a.matches_dir, a.sfm_data_dir, a.test_project_dir, a.output_json_filename) == \
        ("p", "m", "s", None, "loc_global.json")
    assert (a.bow, a.reduce_points, a.ref_points, a.model) == (False, False, False, "similarity")
    a = globalcoord.parse_args(["p", "m", "s", "-t", "T", "-o", "x.json", "--bow", "--reduce-points", "--ref-points",
                                "--model=affine", "--seed=0x10"])
    assert (a.test_project_dir, a.output_json_filename, a.bow, a.reduce_points, a.ref_points, a.model, a.seed) == \
        ("T", "x.json", True, True, True, "affine", 16)
    assert globalcoord.main(["p", "m", "s", "--beacon"], ops=OPS) == 1
    assert "out of scope" in capsys.readouterr().err
    for bad in (["p", "m"], ["p", "m", "s", "--model=rigid"]):
        with pytest.raises(SystemExit):
            globalcoord.parse_args(bad)
    # --bow without a vocabulary, and fewer than 4 reference points: the message, nothing written
    doc = SCENES["clusters"][0]
    proj, matches, sfm = GS.write_project(str(tmp_path), doc, GS.ref_points(doc, GS.amat(), n=3, outliers=()))
    assert globalcoord.main([proj, matches, sfm, "--ref-points", "--bow"], ops=OPS) == 1
    assert globalcoord.main([proj, matches, sfm, "--ref-points"], ops=OPS) == 1
    assert "less than 4 reference points" in capsys.readouterr().out
    assert sorted(os.listdir(os.path.join(proj, "Ref"))) == ["refpoints.json"] and os.listdir(sfm) == ["sfm_data.json"]


def test_ref_points_route_on_the_host(tmp_path):
    """the whole command through the twin: 6 reference landmarks, one an outlier"""
    doc, A = SCENES["clusters"][:2]
    proj, matches, sfm = GS.write_project(str(tmp_path), doc, GS.ref_points(doc, A))
    assert globalcoord.main([proj, matches, sfm, "--ref-points", "--reduce-points"], ops=OPS) == 0
    got = np.loadtxt(os.path.join(proj, "Ref", "Amat.txt"))
    # the planted map: the five inliers carry noise below 1e-3 sqrt(3) and lie among the landmarks, so the fit moves no
    # landmark by more than a few times that (10 x allowed)
    X = np.array([s["value"]["X"] for s in doc["structure"]])
    assert np.abs(GS.world(X, got) - GS.world(X, A)).max() < 10 * 1e-3 * np.sqrt(3)
    assert sorted(os.listdir(sfm)) == ["sfm_data.json", "sfm_data_b4rp.json", "sfm_data_global.json"]
    assert hulo.load_json(os.path.join(sfm, "sfm_data_b4rp.json")) == doc
    thin = hulo.load_json(os.path.join(sfm, "sfm_data.json"))
    assert [k for k, _ in summary(thin)] == [k for k, _ in EXP["reduce"]["clusters"]["kdtree"]]
    # an Amat.txt already there is loaded, not refitted
    np.savetxt(os.path.join(proj, "Ref", "Amat.txt"), A)
    os.remove(os.path.join(proj, "Ref", "refpoints.json"))
    assert globalcoord.main([proj, matches, sfm], ops=OPS) == 0
