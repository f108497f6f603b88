"""sfmlocalization_amd.incrementalsfm on the device, on the path scene of tests/incremental_scene.py: the case the tool
exists for (a pair graph without a triplet, which the global chain cannot pose), the written map, its accuracy on
noise-free pixels against the chain of the NumPy twins (tests/incremental_np.py), the -a/-b pair and the run without a
seed.  The twins' figures are computed here and never taken from the code under test."""
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import adjust_np as AN  # noqa: E402
import incremental_np as IN  # noqa: E402
import incremental_scene as IS  # noqa: E402
import register_scene as RS  # noqa: E402
from sfmlocalization_amd import adjust, globalsfm, incrementalsfm  # noqa: E402

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(ROOT, "profiles", "incremental_sfm.json")


@pytest.fixture(scope="module")
def oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


def twin_chain(scene, oc):
    call = {k: v for k, v in IS.pair_call(scene).items() if k != "view_wh"}
    return IN.run(scene, call, IS.true_relative(scene, call), oc)


@pytest.fixture(scope="module")
def noisy(oc, tmp_path_factory):
    """the path scene at 0.3 px, its files, the tool's run on them (once) and the twins' chain"""
    s = IS.make_scene_path()
    folder = tmp_path_factory.mktemp("path")
    path = RS.write_files(s, str(folder))
    lines = []
    rc = incrementalsfm.run(path, str(folder), str(folder / "out"), log=lines.append)
    return dict(scene=s, folder=folder, path=path, rc=rc, lines=lines, twin=twin_chain(s, oc))


def written(out_dir):
    with open(os.path.join(str(out_dir), "sfm_data.json")) as fh:
        return json.load(fh)


def centres(out, scene):
    """the centres of the views with an extrinsic, in view order, and those views"""
    by_key = {e["key"]: e["value"]["center"] for e in out["extrinsics"]}
    views = [k for k, v in enumerate(scene["view_ids"]) if v in by_key]
    return np.array([by_key[scene["view_ids"][k]] for k in views]), views


def test_global_chain_cannot_pose_the_path(noisy, capfd):
    """Test D, the case the feature exists for.  Without --register the global chain FAILS on the path scene: no triplet
    passes, the averaging has no component of two views, and globalposes ends the run with its exit code; nothing is
    posed and no sfm_data.json is written."""
    out_dir = noisy["folder"] / "global"
    capfd.readouterr()
    rc = globalsfm.run(noisy["path"], str(noisy["folder"]), str(out_dir), log=lambda s: None)
    err = capfd.readouterr().err
    assert rc == 1 and "no triplet of the " in err and "pairs passes: no view can be posed" in err
    assert not os.path.exists(out_dir / "sfm_data.json")


def test_tool_poses_every_view_of_the_path(noisy):
    """Test D: the run succeeds, all 10 views have an extrinsic, every kept observation is within the cleanup's own 4.0 px
    of its landmark's projection (adjust_np.observation_terms on the file), and no fewer landmarks are kept than 0.9 of
    what the twins' chain keeps before any adjustment -- 240 of 240 on this scene, so at least 216."""
    s, twin = noisy["scene"], noisy["twin"]
    assert noisy["rc"] == 0, "\n".join(noisy["lines"][-10:])
    out = written(noisy["folder"] / "out")
    assert sorted(e["key"] for e in out["extrinsics"]) == sorted(s["view_ids"]) and len(out["extrinsics"]) == IS.N_VIEWS
    arrays, _, _ = adjust.sfm_arrays(out)
    res = AN.observation_terms(arrays, arrays["pose_R"], arrays["pose_C"])[0]
    assert len(res) == len(arrays["obs_view"]) > 0 and res.max() <= 4.0
    n_twin = int(twin["landmark_keep"].sum())
    assert twin["pose_valid"].all() and n_twin == 240
    print("landmarks kept: tool", len(out["structure"]), "twins", n_twin)
    assert len(out["structure"]) >= 0.9 * n_twin
    assert out["views"] == s["doc"]["views"] and out["intrinsics"] == s["doc"]["intrinsics"] and out["control_points"] == []
    assert all(os.path.exists(noisy["folder"] / "out" / f) for f in ("matches.e.txt", "relative_poses.json"))
    lines = noisy["lines"]
    assert sum(l.startswith("Seed pair: ") for l in lines) == 1 and sum(l.startswith("Registration round ") for l in lines) >= 3
    assert [l for l in lines if l.startswith("Registration: ")][0].split(",")[1].strip().startswith("8 views registered")
    C, views = centres(out, s)
    err = IS.centre_errors(C, np.array([s["poses"][k][1] for k in views]))
    print("largest centre error at 0.3 px, in mean steps between consecutive views:", err.max())
    assert err.max() < 0.5                                     # the views stand in their order along the arc


def test_noise_free_path_is_as_accurate_as_the_twins(oc, tmp_path):
    """Test E: on noise-free pixels (at .feat precision) the tool's largest centre error after a similarity alignment to
    the truth is at most 5 x the largest error of the twins' chain on the same scene, which is computed here (7e-5 mean
    steps between consecutive views on the CPU).  5 x: the tool ends in an adjustment from a different start and must not
    be worse than the unadjusted twins by more than rounding and gauge drift."""
    s = IS.make_scene_path(noise=0.0)
    truth = np.array([p[1] for p in s["poses"]])
    twin = twin_chain(s, oc)
    assert twin["pose_valid"].all()
    e_twin = float(IS.centre_errors(twin["pose_C"][twin["arrays"]["view_pose"]], truth).max())
    path = RS.write_files(s, str(tmp_path))
    lines = []
    assert incrementalsfm.run(path, str(tmp_path), str(tmp_path / "out"), log=lines.append) == 0, "\n".join(lines[-10:])
    out = written(tmp_path / "out")
    C, views = centres(out, s)
    assert views == list(range(IS.N_VIEWS))
    e_tool = float(IS.centre_errors(C, truth).max())
    print("largest centre error, noise-free, in mean steps between consecutive views: tool", e_tool, "twins", e_twin)
    if os.access(os.path.dirname(PROFILE), os.W_OK):
        with open(PROFILE, "w") as fh:
            json.dump({"scene": "incremental_scene.make_scene_path(noise=0.0): 10 views on an arc, pairs (k, k + 1) only, "
                                "240 points in 4 consecutive views each",
                       "unit": "mean distance between consecutive true centres",
                       "largest_centre_error": {"incrementalsfm": e_tool, "incremental_np": e_twin, "bound_factor": 5.0},
                       "landmarks_kept": {"incrementalsfm": len(out["structure"]),
                                          "incremental_np": int(twin["landmark_keep"].sum())}}, fh, indent=1)
            fh.write("\n")
    assert e_tool <= 5.0 * e_twin


def test_refined_intrinsics_are_written(noisy):
    """-f 1: the last adjustment moves the intrinsics too and the file carries them -- every kept observation is within
    4.0 px under the written intrinsics, and the views still stand in their order along the arc.  The focal lengths
    are printed, not bounded: a short arc holds them weakly, and one view alone is on the radial intrinsic."""
    s = noisy["scene"]
    out_dir = noisy["folder"] / "intrinsics"
    lines = []
    assert incrementalsfm.run(noisy["path"], str(noisy["folder"]), str(out_dir), refine_intrinsics=True,
                              log=lines.append) == 0, "\n".join(lines[-10:])
    assert sum("structure, intrinsics" in l for l in lines) == 1
    out = written(out_dir)
    assert len(out["extrinsics"]) == IS.N_VIEWS and out["intrinsics"] != s["doc"]["intrinsics"]
    arrays, _, _ = adjust.sfm_arrays(out)
    assert AN.observation_terms(arrays, arrays["pose_R"], arrays["pose_C"])[0].max() <= 4.0
    f = arrays["intrinsic"][:, 0]
    print("focal lengths written:", f.tolist(), "planted:", [RS.PINHOLE[0], RS.RADIAL[0]])
    C, views = centres(out, s)
    assert IS.centre_errors(C, np.array([s["poses"][k][1] for k in views])).max() < 0.5
    plain = written(noisy["folder"] / "out")
    assert plain["intrinsics"] == s["doc"]["intrinsics"] and len(plain["structure"]) > 0


def test_named_pair_and_no_seed(noisy, capfd):
    """Test F: -a/-b naming an ok pair that is not the best one seeds from it; with --min-seed-inliers above every pair's
    count the run ends with 1 and the "no seed pair" line, and writes no map"""
    s = noisy["scene"]
    chosen = [l for l in noisy["lines"] if l.startswith("Seed pair: ")][0]
    ids = s["view_ids"]
    other = (5, 6) if f"({ids[5]}, {ids[6]})" not in chosen else (3, 4)      # 112 matches each: ok pairs, candidates
    lines = []
    out_dir = noisy["folder"] / "named"
    rc = incrementalsfm.run(noisy["path"], str(noisy["folder"]), str(out_dir), pair_a=f"frame{other[1]:04d}.jpg",
                            pair_b=f"frame{other[0]:04d}.jpg", log=lines.append)
    assert rc == 0, "\n".join(lines[-10:])
    seed = [l for l in lines if l.startswith("Seed pair: ")]
    assert len(seed) == 1 and seed[0].startswith(f"Seed pair: views ({ids[other[0]]}, {ids[other[1]]}), ") and seed[0] != chosen
    assert len(written(out_dir)["extrinsics"]) == IS.N_VIEWS
    capfd.readouterr()
    # a pair that is not ok: refused by name
    rc = incrementalsfm.run(noisy["path"], str(noisy["folder"]), str(noisy["folder"] / "far"), pair_a="frame0000.jpg",
                            pair_b="frame0005.jpg", log=lambda l: None)
    assert rc == 1 and "is not among the" in capfd.readouterr().err
    assert not os.path.exists(noisy["folder"] / "far" / "sfm_data.json")
    # no pair has 1000 used inliers
    rc = incrementalsfm.run(noisy["path"], str(noisy["folder"]), str(noisy["folder"] / "none"), min_seed_inliers=1000,
                            log=lambda l: None)
    err = capfd.readouterr().err
    assert rc == 1 and re.search(r"openMVG_main_IncrementalSfM: no seed pair: \d+ ok pairs, best median angle \d", err), err
    assert not os.path.exists(noisy["folder"] / "none" / "sfm_data.json")
