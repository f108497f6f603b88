"""sfmloc_sfm_register without a GPU: the restatement (register_np) on Scene A does what the scene was planted to do, its
poses stay within the recorded distance of the planted ones, and the surface is there -- the header's section, the
bindings derived from it, the tools' switches.  `python tests/test_register_cpu.py` rewrites
profiles/register_parity.json."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import register_np as RN  # noqa: E402
import register_scene as RS  # noqa: E402

PARITY = os.path.join(ROOT, "profiles", "register_parity.json")
PARITY_SEEDS = (40, 41, 42, 43, 44)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def grow(sc, oracle_c, **options):
    a = sc["arrays"]
    t = RS.triangulated(a)
    return t, RN.register(a, a["pose_valid"], a["pose_R"], a["pose_C"], t["X"], t["obs_keep"], t["landmark_keep"],
                          oracle_c, **options)


def centre_error(sc, tw):
    """the largest distance of the centres of views 8..11 from the planted ones"""
    return max(float(np.linalg.norm(tw["res"][v]["center"] - sc["poses"][v][1])) for v in range(8, 12))


@pytest.fixture(scope="module")
def grown_a(oracle_c):
    sc = RS.make_scene_a()
    t, tw = grow(sc, oracle_c)
    return sc, t, tw


def test_scene_a_does_what_it_was_planted_to_do(grown_a, oracle_c):
    sc, t, tw = grown_a
    a = sc["arrays"]
    assert t["report"]["landmarks_kept"] == 60 and t["landmark_keep"][:60].all() and not t["landmark_keep"][60:].any()
    assert tw["round"].tolist() == [-1] * 8 + [0, 0, 1, 1, -1, 0]
    assert [r["ok"] for r in tw["res"][8:]] == [True, True, True, True, False, False]
    first, second = tw["rounds"]
    assert first["tried"] == [8, 9, 11, 13] and first["registered"] == [8, 9]          # 10 and 12: 10 or fewer
    assert second["tried"] == [10, 11] and second["registered"] == [10, 11]            # 13: its count did not grow
    assert len(first["lm_added"]) == 60 and second["lm_tried"] == []
    assert not tw["res"][12]["ran"] and tw["res"][13]["ran"] and tw["res"][13]["n_obs"] == 14
    assert tw["res"][10]["n_obs"] == 38 and tw["res"][11]["n_obs"] == 41
    rep = tw["report"]
    assert (rep["rounds"], rep["views_unposed_in"], rep["views_tried"], rep["views_registered"]) == (2, 6, 6, 4)
    # view 11 in round 0: 11 correspondences, 6 of them wrong matches -- tried, and failed
    _, tw0 = grow(sc, oracle_c, max_rounds=1)
    assert tw0["res"][11]["ran"] and not tw0["res"][11]["ok"] and tw0["res"][11]["n_obs"] == 11
    assert not tw0["res"][10]["ran"] and tw0["round"][10] == -1
    # what the call never changes
    posed = a["pose_valid"].astype(bool)
    np.testing.assert_array_equal(bits(tw["pose_R"][posed]), bits(a["pose_R"][posed]))
    np.testing.assert_array_equal(bits(tw["X"][:60]), bits(t["X"][:60]))
    in_posed = posed[a["view_pose"][a["obs_view"]]]
    np.testing.assert_array_equal(tw["obs_keep"][in_posed], t["obs_keep"][in_posed])
    assert tw["pose_valid"].tolist() == [True] * 12 + [False, False]
    # no kept observation in a view without a pose (the cleanup that follows would refuse it)
    assert tw["pose_valid"][a["view_pose"][a["obs_view"]]][tw["obs_keep"]].all()


def test_raw_pixels_give_the_radial_view_another_pose(grown_a, oracle_c):
    sc, t, tw = grown_a
    a = sc["arrays"]
    k = RS.RADIAL_VIEW_A
    assert a["intrinsic_type"][a["view_intrinsic"][k]] == 3
    _, raw = grow(sc, oracle_c, max_rounds=1, undistort=False)
    assert not np.array_equal(bits(raw["res"][k]["P"]), bits(tw["res"][k]["P"]))
    np.testing.assert_array_equal(bits(raw["res"][8]["P"]), bits(tw["res"][8]["P"]))      # a pinhole view: the same
    # and the undistorted one is the better pose
    if raw["res"][k]["ok"]:
        assert np.linalg.norm(tw["res"][k]["center"] - sc["poses"][k][1]) < \
            np.linalg.norm(raw["res"][k]["center"] - sc["poses"][k][1])


def test_one_round_per_call_equals_one_call(grown_a, oracle_c):
    sc, t, tw = grown_a
    a = sc["arrays"]
    s = dict(pose_valid=a["pose_valid"], pose_R=a["pose_R"], pose_C=a["pose_C"], X=t["X"], obs_keep=t["obs_keep"],
             landmark_keep=t["landmark_keep"])
    state = None
    for _ in range(3):
        r = RN.register(a, s["pose_valid"], s["pose_R"], s["pose_C"], s["X"], s["obs_keep"], s["landmark_keep"], oracle_c,
                        max_rounds=1, state=state)
        state = r["state"]
        s = {f: r[f] for f in s}
    assert r["report"]["rounds"] == 0 and r["round"].tolist() == tw["round"].tolist()
    np.testing.assert_array_equal(bits(r["X"]), bits(tw["X"]))
    np.testing.assert_array_equal(bits(r["pose_C"]), bits(tw["pose_C"]))
    np.testing.assert_array_equal(r["obs_keep"], tw["obs_keep"])


def measure(oracle_c):
    return [centre_error(sc, grow(sc, oracle_c)[1]) for sc in (RS.make_scene_a(s) for s in PARITY_SEEDS)]


def test_poses_stay_within_twice_the_recorded_error(grown_a):
    """profiles/register_parity.json holds the twin's centre error of views 8..11 over five scene seeds; a new seed moves
    a P3P pose on 0.3 px noise by about that much, hence twice the maximum.  The device equals the twin bit for bit."""
    sc, t, tw = grown_a
    rec = json.load(open(PARITY))
    assert rec["seeds"] == list(PARITY_SEEDS) and len(rec["centre_error"]) == 5
    assert rec["max"] == max(rec["centre_error"])
    assert centre_error(sc, tw) <= 2.0 * rec["max"]
    assert centre_error(sc, tw) == rec["centre_error"][0]        # (the record is of this code)


def test_surface():
    from sfmlocalization_amd import _abi, capi, globalsfm, structure
    for name in ("sfmloc_register_default_options", "sfmloc_sfm_register", "sfmloc_sfm_register_read",
                 "sfmloc_sfm_register_inliers"):
        assert name in _abi.PROTOTYPES and hasattr(capi._L(), name)
    o = capi.register_default_options()
    assert (o.max_rounds, o.min_points, o.min_inliers, o.tri_min_inliers, o.tri_allow_pairs, o.residual_px) == \
        (16, 10, 0, 3, 1, 4.0)
    assert [f for f, _ in capi.RegisterReport._fields_] == ["rounds", "views_unposed_in", "views_tried",
                                                            "views_registered", "obs_extended", "landmarks_tried",
                                                            "landmarks_added", "device_ms"]
    for f in ("register", "register_read", "register_inliers"):
        assert callable(getattr(capi.Sfm, f))
    base = ["-i", "a", "-m", "b", "-o", "c"]
    assert "register" not in globalsfm.parse_args(base)
    assert globalsfm.parse_args(base + ["--register"]) == {**globalsfm.parse_args(base), "register": True}
    assert "[--register]" in globalsfm.USAGE and "[--register]" in structure.USAGE
    assert structure.REGISTER_ROUNDS == o.max_rounds
    # the tools' command lines: --register is a switch, it takes no value
    assert structure.main(["-i", "a", "-m", "b", "--register"]) == 1                  # (no -o: the usage)
    assert structure.main(base + ["--register", "1"]) == 1


if __name__ == "__main__":
    from oracle import oracle_c as oc
    oc.build()
    values = measure(oc)
    with open(PARITY, "w") as fh:
        json.dump({"what": "register_np on Scene A (tests/register_scene.make_scene_a): the largest distance of the "
                           "centres of views 8..11 from the planted ones, per scene seed; CPU, the device equals the "
                           "twin bit for bit", "seeds": list(PARITY_SEEDS), "centre_error": values, "max": max(values),
                   "unit": "scene units (the cameras' arc has radius 10)"}, fh, indent=1)
        fh.write("\n")
    print(values)
