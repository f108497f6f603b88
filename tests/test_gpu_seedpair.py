"""sfmloc_seed_scores on the device against its restatement (tests/seed_np.py), bit for bit, on the synthetic scene of
tests/seedpair_scene.py (fed R, t and inlier lists directly); the composition RelPoses -> SeedScores -> the choice on the
chain scene; and sfmloc_sfm_register_counts against the counts of the registration twin.  Nothing is compared against the
device's own output."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import incremental_scene as IS  # noqa: E402
import register_np as RN  # noqa: E402
import register_scene as RS  # noqa: E402
import seed_np as tw  # noqa: E402
import seedpair_scene as sc  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def scene():
    """the scene and the twin's records -- computed once, never changed"""
    s = sc.make_scene()
    return dict(s, out=tw.seed_scores(**s["call"]))


def same_records(scores, twin, names):
    assert len(scores) == len(twin)
    for n, r, e in zip(names, scores, twin):
        assert (int(r["n_inliers"]), int(r["n_used"]), int(r["candidate"]), int(r["reserved"])) == \
            (e["n_inliers"], e["n_used"], e["candidate"], 0), n
        assert bits(r["cos_median"]) == bits(e["cos_median"]), (n, float(r["cos_median"]), e["cos_median"])


def test_scores_are_the_twins_bits(scene):
    """Test A: every inlier count around the wave, the workgroup and beyond, even and odd n_used, a third of the points
    behind a camera, the radial intrinsic, the pair next to a pure rotation, duplicated matches, the pair the last radix
    pass decides, use_pair = 0"""
    a = S.SeedScores(**scene["call"])
    same_records(a.scores, scene["out"], scene["names"])
    assert a.ms > 0.0
    b = S.SeedScores(**scene["call"])                          # two runs give the same bits
    assert a.scores.tobytes() == b.scores.tobytes()


def test_a_record_depends_on_its_own_pair_alone(scene):
    for name in ("n257b", "n2049a", "low", "n1a"):
        k = scene["names"].index(name)
        one = S.SeedScores(**sc.sub_call(scene["call"], [k]))
        same_records(one.scores, [scene["out"][k]], [name])
    empty = S.SeedScores(**sc.sub_call(scene["call"], []))
    assert len(empty.scores) == 0 and empty.ms == 0.0 and empty.choose(np.arange(4)) == -1


def test_options_move_the_candidates_only(scene):
    call = scene["call"]
    r = S.SeedScores(**call, min_used=40, max_cos=0.97, min_cos=0.955)
    e = tw.seed_scores(**call, min_used=40, max_cos=0.97, min_cos=0.955)
    same_records(r.scores, e, scene["names"])
    assert [int(x) for x in r.scores["candidate"]] != [x["candidate"] for x in scene["out"]]


def test_composition_with_the_relative_poses():
    """Test B: RelPoses -> SeedScores on the chain scene; the chosen pair is the twin's on the same results"""
    s = RS.make_scene_chain()
    call = IS.pair_call(s)
    rp = S.RelPoses(**call)
    ok = rp.results["ok"].astype(np.uint8)
    assert ok.sum() >= 10
    fed = dict({k: v for k, v in call.items() if k != "view_wh"}, rel_R=rp.results["R"], rel_t=rp.results["t"],
               inl_off=rp.inl_off, inl_idx=rp.inl_idx, use_pair=ok)
    got = S.SeedScores(**fed, min_used=30)
    e = tw.seed_scores(**fed, min_used=30)
    same_records(got.scores, e, [tuple(p) for p in call["pairs"]])
    view_pose = s["arrays"]["view_pose"]
    k = got.choose(view_pose)
    assert k == tw.choose(e, call["pairs"], view_pose) and k >= 0 and ok[k]
    assert k == int(np.argmin([x["cos_median"] if x["candidate"] else 2.0 for x in e]))


def test_register_counts():
    """Test C: the counts of a round as it would stand now, before and after a round; EINVAL before the masks exist; the
    handle is not changed by the call"""
    from oracle import oracle_c
    oracle_c.build()
    a = RS.make_scene_a()["arrays"]
    t = RS.triangulated(a)
    off = a["obs_off"].astype(np.int64)
    obs_lm = np.repeat(np.arange(len(a["landmark_id"])), np.diff(off))

    def twin_counts(landmark_keep):
        return np.bincount(a["obs_view"][np.asarray(landmark_keep, bool)[obs_lm]], minlength=len(a["view_id"]))
    h = S.Sfm(**a)
    with pytest.raises(S.SfmlocError) as ei:
        h.register_counts()
    assert ei.value.code == S.EINVAL and "sfmloc_sfm_register_counts: the keep masks do not exist yet" in ei.value.message
    h.triangulate()
    before, X = h.read(masks=True), h.read_structure()
    c = h.register_counts()
    assert c.dtype == np.uint32 and c.tolist() == twin_counts(t["landmark_keep"]).tolist()
    assert c[8:].tolist() == [40, 40, 8, 11, 6, 14]                       # register_scene's table for scene A
    after = h.read(masks=True)
    for f in before:
        assert before[f].tobytes() == after[f].tobytes(), f
    assert bits(h.read_structure()).tobytes() == bits(X).tobytes()
    assert h.register_read()[1].tolist() == [-1] * len(a["view_id"])       # no round was counted
    h.register(max_rounds=1)
    one = RN.register(a, a["pose_valid"], a["pose_R"], a["pose_C"], t["X"], t["obs_keep"], t["landmark_keep"], oracle_c,
                      max_rounds=1)
    assert one["report"]["landmarks_added"] > 0
    assert h.register_counts().tolist() == twin_counts(one["landmark_keep"]).tolist()
    h.close()
