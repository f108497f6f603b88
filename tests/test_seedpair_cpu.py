"""CPU: the NumPy restatement of sfmloc_seed_scores (tests/seed_np.py) on hand-made pairs -- the rank of the median, the
inliers that are not used, the clamp, the order of the keys, the choice of the seed pair -- the properties the scene of
tests/test_gpu_seedpair.py is built to have, the refusals (which need no device), the declared symbols, and the host side
under the host sanitizers."""
import ctypes as C
import math
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import seed_np as tw  # noqa: E402
import seedpair_scene as sc  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import _abi, capi  # noqa: E402


@pytest.fixture(scope="module")
def scene():
    """the scene and the twin's records by name -- computed once, never changed"""
    s = sc.make_scene()
    return dict(s, out=dict(zip(s["names"], tw.seed_scores(**s["call"]))), index={n: k for k, n in enumerate(s["names"])})


def test_median_is_the_element_of_rank_n_over_two_from_the_top():
    """descending keys, rank n // 2 from 0: OpenMVG's nth_element index on ascending angles"""
    c = np.array([0.3, 0.9, 0.1, 0.7, 0.5])
    assert tw.median_cosine(c) == 0.5                       # odd: the middle
    assert tw.median_cosine(c[:4]) == 0.3                   # even: 0.9 0.7 0.3 0.1 -> rank 2, the lower of the middle two
    assert tw.median_cosine(c[:2]) == 0.3 and tw.median_cosine(c[:1]) == 0.3 and tw.median_cosine(c[:0]) == 0.0
    assert tw.median_cosine(np.array([-0.25, 0.5, -0.75])) == -0.25
    ang = np.degrees(np.arccos(c[:4]))                      # the same element as nth_element(n / 2) on ascending angles
    assert math.isclose(math.degrees(math.acos(tw.median_cosine(c[:4]))), np.sort(ang)[len(ang) // 2])


def test_keys_order_doubles_and_tell_the_zeros_apart():
    v = np.array([-1.0, -0.5, -5e-324, -0.0, 0.0, 5e-324, 0.5, 1.0 - 1e-8])
    k = tw.keys(v)
    assert (np.diff(k.astype(object)) > 0).all()            # strictly ascending: -0.0 below +0.0
    assert tw.unkeys(k).tobytes() == v.tobytes() and (k != 0).all()
    assert int(tw.keys(np.array([0.0]))[0]) == 1 << 63 and int(tw.keys(np.array([-0.0]))[0]) == (1 << 63) - 1
    # rank 1 of (+0.0, -0.0) in descending order is -0.0, whatever order they come in
    for pair in ([0.0, -0.0], [-0.0, 0.0]):
        assert math.copysign(1.0, tw.median_cosine(np.array(pair))) == -1.0
    assert math.copysign(1.0, tw.median_cosine(np.array([-0.0, 0.0, 0.0]))) == 1.0


def test_clamp_and_nan():
    eye = np.eye(3).reshape(9)
    b = np.array([[0.1, -0.2], [0.0, 0.0]])
    assert (tw.cosines(eye, b, b) == tw.HI).all()           # the same ray: 1 -> hi
    flip = np.diag([-1.0, -1.0, -1.0]).reshape(9)
    assert (tw.cosines(flip, b, b) == tw.LO).all()          # the opposite ray: -1 -> lo
    bad = eye.copy()
    bad[4] = np.nan
    assert (tw.cosines(bad, b, b) == tw.LO).all()           # NaN -> lo
    c = tw.cosines(eye, np.array([[0.0, 0.0]]), np.array([[1.0, 0.0]]))
    assert abs(c[0] - math.sqrt(0.5)) < 1e-15 and tw.LO == -1.0 + 1e-8 and tw.HI == 1.0 - 1e-8


def test_scene_has_what_it_is_built_for(scene):
    out, behind = scene["out"], scene["behind"]
    for c in sc.COUNTS:
        a = out[f"n{c}a"]
        assert a["n_inliers"] == c and a["n_used"] == int((~behind[:c]).sum())        # the points behind are skipped
        if c:
            b = out[f"n{c}b"]
            assert b["n_inliers"] == c and abs(b["n_used"] - a["n_used"]) == 1        # one even, one odd
        if c >= 3:
            assert c // 2 <= a["n_used"] < c                                          # about a third is not used
    call = scene["call"]
    assert call["view_intrinsic"][2] == 1 and call["intrinsic_type"][1] == 3
    assert all((call["pairs"][scene["index"][f"n{c}b"]] == (0, 2)).all() for c in sc.COUNTS if c)   # the radial view
    assert out["n0a"] == dict(n_inliers=0, n_used=0, candidate=0, cos_median=0.0)
    assert out["n1b"]["n_used"] == 0 and out["n1b"]["cos_median"] == 0.0 and out["n1b"]["n_inliers"] == 1
    assert out["n5000a"]["candidate"] == 1 and out["n65a"]["candidate"] == 0          # 44 used < min_used
    rot = out["rot"]
    assert rot["n_used"] >= 100 and rot["cos_median"] >= tw.MAX_COS and rot["candidate"] == 0
    assert out["dup"]["n_used"] == out["dup"]["n_inliers"] == 120 and out["dup"]["candidate"] == 1
    assert out["off"] == dict(n_inliers=0, n_used=0, candidate=0, cos_median=0.0)
    assert tw.MAX_COS == math.cos(math.radians(3.0)) and abs(math.cos(math.radians(60.0)) - 0.5) < 1e-15


def test_duplicated_matches_have_equal_keys(scene):
    k = scene["index"]["dup"]
    c, n = tw.pair_cosines(*[scene["call"][f] for f in ("view_off", "kpt_xy", "view_intrinsic", "intrinsics",
                                                       "intrinsic_type", "pairs", "offsets", "match_i", "match_j", "rel_R",
                                                       "rel_t", "inl_off", "inl_idx")], k)
    assert n == 120 and len(np.unique(tw.keys(c))) == 4 and (np.bincount(np.unique(tw.keys(c), return_inverse=True)[1]) == 30).all()


def test_lowest_byte_pair_is_decided_by_the_last_radix_pass(scene):
    k = scene["index"]["low"]
    c, n = tw.pair_cosines(*[scene["call"][f] for f in ("view_off", "kpt_xy", "view_intrinsic", "intrinsics",
                                                       "intrinsic_type", "pairs", "offsets", "match_i", "match_j", "rel_R",
                                                       "rel_t", "inl_off", "inl_idx")], k)
    keys = tw.keys(c)
    assert n == len(c) == 5 and len(np.unique(keys)) == 2
    assert len(np.unique(keys >> np.uint64(8))) == 1 and len(np.unique(keys & np.uint64(255))) == 2
    lo, hi = np.unique(keys)
    assert (keys == np.array([hi, lo, hi, lo, lo])).all()
    # the median is the smaller key: seven passes cannot tell it from the larger one
    assert tw.keys(np.array([scene["out"]["low"]["cos_median"]]))[0] == lo


def test_choice_of_the_seed_pair():
    pairs = [(0, 1), (1, 2), (2, 3), (0, 3), (0, 2)]
    own, rig = np.arange(4), np.array([0, 1, 2, 2])

    def rec(n, cand, c):
        return dict(n_inliers=n, n_used=n, candidate=cand, cos_median=c)

    def both(scores, view_pose):
        arr = np.zeros(len(scores), capi.SEED_SCORE)
        for i, s in enumerate(scores):
            for f, v in s.items():
                arr[i][f] = v
        a, b = tw.choose(scores, pairs, view_pose), capi.seed_choose(arr, pairs, view_pose)
        assert a == b
        return a
    s = [rec(150, 1, 0.98), rec(120, 1, 0.97), rec(400, 0, 0.2), rec(130, 1, 0.97), rec(130, 1, 0.97)]
    assert both(s, own) == 3                 # 0.97 three times: 130 beats 120, pair 3 comes before pair 4
    s[3] = rec(120, 1, 0.97)
    assert both(s, own) == 4
    s[4] = rec(120, 1, 0.97)
    assert both(s, own) == 1                 # all equal: the smallest index
    s[2] = rec(100, 1, 0.6)
    assert both(s, own) == 2 and both(s, rig) == 1          # (2, 3) share an id_pose: skipped
    assert both([rec(r["n_used"], 0, r["cos_median"]) for r in s], own) == -1 and both([], own) == -1


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_seed_\w+|sfmloc_sfm_register_counts)\s*\(", hdr))
    assert names == {"sfmloc_seed_default_options", "sfmloc_seed_scores", "sfmloc_seed_read", "sfmloc_seed_destroy",
                     "sfmloc_seed_last_ms", "sfmloc_sfm_register_counts"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    assert L.sfmloc_abi_version() == 2
    o = capi.seed_default_options()
    assert {k: getattr(o, k) for k in tw.OPTIONS} == tw.OPTIONS == dict(min_used=100, max_cos=0.9986295347545738, min_cos=0.5)
    rec = _abi.struct("sfmloc_seed_score")
    assert capi.SEED_SCORE.itemsize == C.sizeof(rec) == 24 and C.sizeof(_abi.struct("sfmloc_seed_options")) == 24
    assert [capi.SEED_SCORE.fields[f][1] for f, _ in rec._fields_] == [getattr(rec, f).offset for f, _ in rec._fields_]
    with pytest.raises(AttributeError):
        capi.seed_default_options(min_use=3)
    assert hasattr(capi.Sfm, "register_counts")


def test_refusals_need_no_device(scene):
    """every check of sfmloc_seed_scores happens before anything is launched: the refusals come back without a GPU"""
    s = sc.sub_call(scene["call"], [scene["index"][n] for n in ("n63a", "n64b", "rot")])
    bad_R, bad_t, bad_inl, bad_mi = s["rel_R"].copy(), s["rel_t"].copy(), s["inl_idx"].copy(), s["match_i"].copy()
    bad_R[1, 2], bad_t[2, 1] = np.nan, np.inf
    bad_inl[63 + 5] = 70
    bad_mi[66 + 4] = 6000
    for change, code, text in (
            (dict(pairs=[[0, 1], [1, 4], [0, 3]]), capi.EINVAL, "sfmloc_seed_scores: pair 1 = (1, 4) out of range"),
            (dict(pairs=[[0, 1], [2, 2], [0, 3]]), capi.EINVAL, "sfmloc_seed_scores: pair 1 names view 2 twice"),
            (dict(match_i=bad_mi), capi.EINVAL, "sfmloc_seed_scores: pair (0, 2) match 4 out of range"),
            (dict(intrinsic_type=[0, 2]), capi.EINVAL, "sfmloc_seed_scores: intrinsic 1 has type 2"),
            (dict(inl_idx=bad_inl), capi.EINVAL, "sfmloc_seed_scores: pair (0, 2) inlier 5 out of range"),
            (dict(inl_off=[0, 63, 60, 327]), capi.EINVAL, "sfmloc_seed_scores: inlier_off not monotone at pair 1"),
            (dict(rel_R=bad_R), capi.EINVAL, "sfmloc_seed_scores: pair (0, 2) has a non-finite rel_R or rel_t"),
            (dict(rel_t=bad_t), capi.EINVAL, "sfmloc_seed_scores: pair (0, 3) has a non-finite rel_R or rel_t"),
            (dict(min_used=0), capi.EINVAL, "sfmloc_seed_scores: min_used = 0"),
            (dict(max_cos=float("nan")), capi.EINVAL, "sfmloc_seed_scores: max_cos is not a cosine in (-1, 1]"),
            (dict(max_cos=1.5), capi.EINVAL, "sfmloc_seed_scores: max_cos is not a cosine in (-1, 1]"),
            (dict(min_cos=-1.0), capi.EINVAL, "sfmloc_seed_scores: min_cos is not a cosine in (-1, 1]"),
            (dict(min_cos=float("inf")), capi.EINVAL, "sfmloc_seed_scores: min_cos is not a cosine in (-1, 1]"),
            (dict(min_cos=0.9986295347545738), capi.EINVAL, "sfmloc_seed_scores: min_cos must be below max_cos"),
            (dict(min_cos=0.5, max_cos=0.25), capi.EINVAL, "sfmloc_seed_scores: min_cos must be below max_cos")):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.SeedScores(**{**s, **change})
        assert ei.value.code == code and text in ei.value.message, ei.value.message
    for change in (dict(rel_R=s["rel_R"][:2]), dict(inl_off=s["inl_off"][:3]), dict(use_pair=[1, 1]),
                   dict(view_intrinsic=[0, 1])):
        with pytest.raises(ValueError):
            capi.SeedScores(**{**s, **change})


def test_host_side_under_the_host_sanitizers(tmp_path):
    """tests/cpp/seed_host.cpp: a stand-alone host program over seed_host.h and pair_scene.h, CPU only, every refusal and
    the choice.  Where a HIP device is visible the program is built without the sanitizers (they are for CPU machines);
    it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/seed_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "seed_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "seed_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")
