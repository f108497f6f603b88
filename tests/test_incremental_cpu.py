"""CPU: the path scene of the incremental-SfM tests (tests/incremental_scene.py) has no triplet, and the chain of the
NumPy twins (tests/incremental_np.py: seed, triangulation, growth rounds under the 0.75 rule) poses all of its views from
the planted relative poses; the command line of sfmlocalization_amd.incrementalsfm."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import incremental_np as IN  # noqa: E402
import incremental_scene as IS  # noqa: E402
from sfmlocalization_amd import incrementalsfm  # noqa: E402


@pytest.fixture(scope="module")
def oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


@pytest.fixture(scope="module")
def path(oc):
    """the path scene, its pair-side call, the planted relative poses and the twins' chain on them -- computed once"""
    s = IS.make_scene_path()
    call = {k: v for k, v in IS.pair_call(s).items() if k != "view_wh"}
    rel = IS.true_relative(s, call)
    return s, call, rel, IN.run(s, call, rel, oc)


def test_path_scene_has_no_triplet(path):
    s, call, _, _ = path
    assert call["pairs"].tolist() == [[k, k + 1] for k in range(IS.N_VIEWS - 1)]
    assert IS.triplets(call["pairs"]) == [] and IS.triplets([(0, 1), (1, 2), (0, 2), (2, 3)]) == [(0, 1, 2)]
    assert len(s["points"]) == sum(IS.STARTS) == 240 and not any(s["posed"])
    per_point = np.diff(s["arrays"]["obs_off"].astype(np.int64))
    assert (per_point == IS.SPAN).all()                                   # each point in four consecutive views
    assert s["arrays"]["view_intrinsic"].tolist().count(1) == 1          # one view on the radial intrinsic
    shared = np.diff(call["offsets"].astype(np.int64))
    assert shared.max() > 100 and shared.min() < 100                      # some pairs can seed, the ends cannot


def test_twins_pose_every_view_of_the_path(path):
    s, call, rel, r = path
    k = r["seed"]
    assert k >= 0 and r["scores"][k]["candidate"] and r["scores"][k]["n_used"] >= 100
    cand = [x["cos_median"] for x in r["scores"] if x["candidate"]]
    assert r["scores"][k]["cos_median"] == min(cand) and len(cand) >= 2
    assert 3.0 < np.degrees(np.arccos(r["scores"][k]["cos_median"])) < 60.0
    assert r["kept_after_seed"] == int(np.diff(call["offsets"].astype(np.int64))[k])   # every shared point triangulates
    assert r["pose_valid"].all() and len(r["pose_valid"]) == IS.N_VIEWS
    assert int(r["landmark_keep"].sum()) == 240
    assert len(r["rounds"]) >= 3 and all(reg for _, _, reg in r["rounds"])
    assert sorted(v for _, _, reg in r["rounds"] for v in reg) == sorted(set(range(IS.N_VIEWS)) - set(call["pairs"][k].tolist()))
    for best, min_points, _ in r["rounds"]:
        assert min_points == IN.growth_min_points(best) == incrementalsfm.growth_min_points(best)
    a = r["arrays"]
    err = IS.centre_errors(r["pose_C"][a["view_pose"]], np.array([p[1] for p in s["poses"]]))
    print("largest centre error, in mean steps between consecutive views:", err.max())
    assert err.max() < 0.5                                                # the views stand in their order along the arc


def test_the_rule_of_three_quarters():
    assert [IN.growth_min_points(b) for b in (0, 10, 14, 15, 16, 82, 100)] == [10, 10, 10, 11, 11, 61, 74]
    # with register's test ">": a view is tried when it has at least 0.75 of the best view's tracks
    for best in range(14, 200):
        m = IN.growth_min_points(best)
        assert m + 1 >= 0.75 * best > m


def test_centre_errors_undo_a_similarity():
    rng = np.random.Generator(np.random.PCG64(5))
    T = rng.normal(size=(7, 3))
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    q = q * np.sign(np.linalg.det(q))
    C = 2.5 * (q @ T.T).T + np.array([1.0, -2.0, 3.0])
    assert IS.centre_errors(C, T).max() < 1e-12
    C[3] += 0.1
    assert IS.centre_errors(C, T).max() > 1e-3


def test_command_line():
    base = ["-i", "a.json", "-m", "dir", "-o", "out"]
    kw = incrementalsfm.parse_args(base)
    assert kw == dict(in_path="a.json", match_dir="dir", out_dir="out", min_seed_inliers=100, device=0)
    assert incrementalsfm.parse_args(["--input_file", "a.json", "--matchdir", "dir", "--outdir", "out"]) == kw
    assert incrementalsfm.parse_args(base + ["-a", "f1.jpg", "-b", "f2.jpg"]) == {**kw, "pair_a": "f1.jpg", "pair_b": "f2.jpg"}
    assert incrementalsfm.parse_args(base + ["--initialPairA", "f1.jpg", "--initialPairB", "f2.jpg"]) == \
        {**kw, "pair_a": "f1.jpg", "pair_b": "f2.jpg"}
    assert incrementalsfm.parse_args(base + ["-f", "1"]) == {**kw, "refine_intrinsics": True}
    assert incrementalsfm.parse_args(base + ["-f", "0"]) == kw
    assert incrementalsfm.parse_args(base + ["--min-seed-inliers", "30", "--device=2"]) == \
        {**kw, "min_seed_inliers": 30, "device": 2}
    assert incrementalsfm.parse_args(base + ["--min-seed-inliers=30"]) == {**kw, "min_seed_inliers": 30}
    for bad in (["-i", "a.json", "-m", "dir"], base + ["-a", "f1.jpg"], base + ["-b", "f2.jpg"], base + ["-f", "2"],
                base + ["-a", "f1.jpg", "-b", "f1.jpg"], base + ["--min-seed-inliers", "0"],
                base + ["--min-seed-inliers", "many"], base + ["--device", "-1"], base + ["--register"], base + ["-o"],
                base + ["-f"], []):
        assert incrementalsfm.parse_args(bad) is None, bad
    for word in ("-a", "-b", "-f", "--min-seed-inliers", "--device", "openMVG_main_IncrementalSfM"):
        assert word in incrementalsfm.USAGE
    assert incrementalsfm.main(["-i", "a.json"]) == 1
