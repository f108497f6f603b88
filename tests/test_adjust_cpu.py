"""OpenMVG_BA twin without a GPU: the refusals of both programs, the NumPy restatement of the cleanup on hand-made cases,
the C++ JSON writer against json.dump, the hulo.py pin, and the margin condition of the GPU tests' inputs."""
import json
import math
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import adjust_np as AN  # noqa: E402
from sfmlocalization_amd import adjust, capi, hulo  # noqa: E402

BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVG_BA")


def _programs():
    return [[BIN], [sys.executable, "-m", "sfmlocalization_amd.adjust"]]


def _arrays(views, poses, structure, intrinsics=((0, (800.0, 320.0, 240.0, 0, 0, 0)),)):
    """views: [(id, intrinsic index, pose index)], poses: [(valid, R, C)], structure: [(X, [(view index, x, y)])]"""
    obs_off, obs_view, obs_x = [0], [], []
    for _, obs in structure:
        for v, x, y in obs:
            obs_view.append(v)
            obs_x.append([x, y])
        obs_off.append(len(obs_view))
    return dict(view_id=np.array([v[0] for v in views], np.uint32), view_intrinsic=np.array([v[1] for v in views], np.uint32),
                view_pose=np.array([v[2] for v in views], np.uint32),
                intrinsic_type=np.array([t for t, _ in intrinsics], np.uint32),
                intrinsic=np.array([k for _, k in intrinsics], np.float64),
                pose_valid=np.array([p[0] for p in poses], np.uint8),
                pose_R=np.array([np.asarray(p[1], float).reshape(9) for p in poses]),
                pose_C=np.array([np.asarray(p[2], float) for p in poses]),
                landmark_id=np.arange(len(structure), dtype=np.uint32) * 2 + 1,
                landmark_X=np.array([X for X, _ in structure], np.float64).reshape(-1, 3),
                obs_off=np.array(obs_off, np.uint64), obs_view=np.array(obs_view, np.uint32),
                obs_x=np.array(obs_x, np.float64).reshape(-1, 2))


def test_cli_refusals(tmp_path):
    src = tmp_path / "sfm_data.json"
    src.write_text(json.dumps({"views": [], "intrinsics": []}))
    out = tmp_path / "out.json"
    for prog in _programs():
        r = subprocess.run(prog + [str(src), str(out), "-c=rst"], capture_output=True, text=True, cwd=ROOT)
        assert r.returncode == 1 and "-c" in r.stderr, (prog, r.stderr)
        for args in ([], [str(src)]):
            r = subprocess.run(prog + args, capture_output=True, text=True, cwd=ROOT)
            assert r.returncode == 1 and "Usage" in r.stderr, (prog, args, r.stderr)
    assert sorted(os.listdir(tmp_path)) == ["sfm_data.json"]     # nothing written


def test_residual_zero_and_right_angle():
    R = np.eye(3)
    # a landmark that projects exactly: residual 0; two views 90 degrees apart see it
    X = np.array([0.0, 0.0, 10.0])
    R2 = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])   # looks along +x from (-10, 0, 10)
    C2 = np.array([-10.0, 0.0, 10.0])
    a = _arrays([(0, 0, 0), (1, 0, 1)], [(1, R, [0, 0, 0]), (1, R2, C2)], [(X, [(0, 320.0, 240.0), (1, 320.0, 240.0)])])
    out = AN.clean(a, a["pose_valid"], a["pose_R"], a["pose_C"])
    np.testing.assert_array_equal(out["res"], [0.0, 0.0])
    assert abs(AN.angle_deg(out["min_cos"][0]) - 90.0) < 1e-9
    assert out["landmark_keep"].tolist() == [True]


def test_duplicate_rays_removed():
    R = np.eye(3)
    X = np.array([0.5, 0.2, 10.0])
    u, v = 800 * 0.05 + 320, 800 * 0.02 + 240
    a = _arrays([(0, 0, 0), (1, 0, 1)], [(1, R, [0, 0, 0]), (1, R, [0, 0, 0])], [(X, [(0, u, v), (1, u, v)])])
    out = AN.clean(a, a["pose_valid"], a["pose_R"], a["pose_C"])
    assert out["min_cos"][0] == 1.0 - 1e-8 and AN.angle_deg(out["min_cos"][0]) < 2.0
    assert out["stage"].tolist() == [1] and out["counts"] == [1, 1, 0, 0]


def test_unstable_two_passes_and_orphan_pose():
    """pose 0 has 5 observations: erased in pass 1, which leaves landmarks of pose 1 with one observation; they go, pose
    1 drops to 5 and is erased in pass 2.  Pose 3 is named by no view: 0 observations, erased too."""
    rng = np.random.Generator(np.random.PCG64(3))
    cams = [np.array([-2.0, 0, 0]), np.array([0.0, 0, 0]), np.array([2.0, 0, 0])]
    R = np.eye(3)
    structure = []

    def obs_of(X, views):
        return [(k, 800 * (X[0] - cams[k][0]) / X[2] + 320, 800 * (X[1] - cams[k][1]) / X[2] + 240) for k in views]
    for _ in range(5):                       # seen by views 0 and 1
        X = rng.uniform([-1, -1, 8], [1, 1, 12])
        structure.append((X, obs_of(X, [0, 1])))
    for _ in range(1):                       # views 1 and 2
        X = rng.uniform([-1, -1, 8], [1, 1, 12])
        structure.append((X, obs_of(X, [1, 2])))
    for _ in range(20):                      # views 2 and 3: both stay
        X = rng.uniform([-1, -1, 8], [1, 1, 12])
        structure.append((X, obs_of(X, [2]) + [(3, 0.0, 0.0)]))
    views = [(0, 0, 0), (1, 0, 1), (2, 0, 2), (3, 0, 4)]
    poses = [(1, R, cams[0]), (1, R, cams[1]), (1, R, cams[2]), (1, R, [9, 9, 9]), (1, R, [0, 0, -5.0])]
    a = _arrays(views, poses, structure)
    keep = np.ones(len(a["obs_view"]), bool)
    stage = np.full(len(structure), 3, np.uint8)
    pv, keep2, stage2, passes = AN.unstable(a, a["pose_valid"].astype(bool), keep, stage)
    assert passes == 3                       # two passes remove something, the third finds nothing
    assert pv.tolist() == [False, False, True, False, True]
    assert (stage2[:6] == 2).all() and (stage2[6:] == 3).all()


def test_json_writer_round_trip(tmp_path):
    doc, _ = _scene()
    synth = tmp_path / "synth.json"
    synth.write_text(json.dumps(doc).replace('"root_path": "/data/images"', '"root_path": "/d\\u00e9j\\u00e0/\\ud83d\\ude00\\t"'))
    for src in (os.path.join(HERE, "golden", "files", "sfm_data.json"), str(synth)):
        out = tmp_path / "rt.json"
        capi.sfm_json_rewrite(src, str(out))
        with open(src) as fh:
            want = json.dumps(json.load(fh))
        assert out.read_text() == want


def test_hulo_pin():
    with open(os.path.join(HERE, "golden", "ref_params.json")) as fh:
        ref = json.load(fh)["ReconstructParam"]
    assert os.path.basename(hulo.BUNDLE_ADJUSTMENT_PROJECT_PATH) == os.path.basename(ref["BUNDLE_ADJUSTMENT_PROJECT_PATH"])
    assert hulo.BUNDLE_ADJUSTMENT_PROJECT == ref["BUNDLE_ADJUSTMENT_PROJECT"]


def _scene():
    import adjust_scene as AS
    return AS.make_doc()


def test_margin_condition():
    """The GPU tests' inputs, restated on the CPU with the oracle's poses: no residual within 1e-6 px of 4.0 and no
    landmark's minimum clamped cosine within 1e-9 of cos(2 degrees), so the device's acos cannot flip a decision."""
    import adjust_scene as AS
    from oracle import oracle_c
    oracle_c.build()
    doc, _ = AS.make_doc()
    a, _, _ = adjust.sfm_arrays(doc)
    res, pv, R, C = AS.oracle_resect(a, oracle_c)
    out = AN.clean(a, pv, R, C, rm_unstable=True)
    r = out["res"][np.isfinite(out["res"])]
    mc = out["min_cos"][np.isfinite(out["min_cos"])]
    print("closest residual to 4 px:", np.abs(r - 4.0).min(), "closest cosine to cos 2:",
          np.abs(mc - math.cos(math.radians(2.0))).min())
    assert np.abs(r - 4.0).min() > 1e-6
    assert np.abs(mc - math.cos(math.radians(2.0))).min() > 1e-9
    # the planted cases are there
    assert not res[AS.FAIL_VIEW]["ok"] and res[AS.FAIL_VIEW]["ran"]
    assert all(not res[k]["ran"] for k in AS.FEW_VIEWS + (AS.WEAK_VIEW,))
    assert out["counts"][1] < out["counts"][0] and out["counts"][2] < out["counts"][1]
    assert not out["pose_valid"][-1] and pv[-1]                      # the orphan pose goes with -r=1


def test_unsupported_intrinsic_refused(tmp_path):
    """An intrinsic type other than pinhole / pinhole_radial_k3: sfmloc_sfm_create refuses it with SFMLOC_EIO (before it
    looks for a device), and both programs print that message, exit 1 and write nothing."""
    import adjust_scene as AS
    doc, _ = AS.make_doc()
    doc["intrinsics"][1]["value"]["polymorphic_name"] = "fisheye"
    a, _, _ = adjust.sfm_arrays(doc)
    with pytest.raises(capi.SfmlocError) as ei:
        capi.Sfm(**a)
    assert ei.value.code == capi.EIO and "not supported" in ei.value.message
    for k, prog in enumerate(_programs()):
        d = tmp_path / str(k)
        d.mkdir()
        (d / "sfm_data.json").write_text(json.dumps(doc))
        r = subprocess.run(prog + [str(d / "sfm_data.json"), str(d / "out.json")], capture_output=True, text=True,
                           cwd=ROOT)
        assert r.returncode == 1 and r.stderr.strip() == "OpenMVG_BA: " + ei.value.message, r.stderr
        assert sorted(os.listdir(d)) == ["sfm_data.json"]


def test_nan_cosine_clamps_low():
    """OpenMVG's clamp, max(lo, min(c, hi)): a NaN cosine (a zero ray) becomes lo, i.e. 180 degrees"""
    ray = np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 0.0]])
    rn = np.sqrt((ray * ray).sum(1))
    c = AN.pair_cosines(ray, rn, np.array([0, 1]))
    assert c.tolist() == [AN.LO]
