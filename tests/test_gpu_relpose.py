"""Relative poses on the device (sfmloc_relative_poses, sfmloc_debug_five_point, python -m sfmlocalization_amd.relpose)
and bin/ComputeRelativePoses against the NumPy restatement (tests/relpose_np.py) on the planted scene (tests/relpose_scene.py).  The library is built
with -ffp-contract=off and the restatement applies the same operations in the same order: every double is compared as a
bit pattern, no tolerance.  The numeric comparisons against the planted truth take their bounds from
tests/golden/relpose/expected.json (tests/golden/make_relpose_fixtures.py says how each was measured)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import relpose_np as tw  # noqa: E402
import relpose_scene as sc  # noqa: E402
from sfmlocalization_amd import capi, fileio, relpose, structure  # noqa: E402

pytestmark = pytest.mark.gpu

PROGRAMS = [("cpp", [os.path.join(ROOT, "sfmlocalization_amd", "bin", relpose.NAME)]),
            ("py", [sys.executable, "-m", "sfmlocalization_amd.relpose"])]

EXPECTED = os.path.join(HERE, "golden", "relpose", "expected.json")
DOUBLES = ("E", "R", "t", "error_max_px", "nfa")
INTS = ("ok", "n_matches", "n_inliers", "sample", "front", "choice")


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def ref():
    """the scene, the call's arrays, the twin's results and the device's: computed once, left unchanged"""
    s = sc.make_scene()
    args, names = sc.call_arrays(s)
    return {"s": s, "args": args, "names": names, "twin": tw.relative_poses(**args), "got": capi.RelPoses(**args)}


def same_pair(r, inl, want):
    """one device record and its inlier list against a twin result"""
    for f in INTS:
        assert np.array_equal(np.asarray(r[f], np.int64).ravel(), np.asarray(want[f], np.int64).ravel()), f
    for f in DOUBLES:
        assert np.array_equal(bits(r[f]).ravel(), bits(want[f]).ravel()), f
    assert np.array_equal(np.asarray(inl, np.int64), want["inliers"])


def test_solver_gives_the_twins_models(expected):
    rows = np.array([s["x1"] + s["x2"] for s in expected["solver"]])
    n, E = capi.five_point(rows)
    wn, wE = tw.five_point(rows[:, :10].reshape(-1, 5, 2), rows[:, 10:].reshape(-1, 5, 2))
    assert n.tolist() == wn.tolist() == [s["twin_n"] for s in expected["solver"]]
    assert np.array_equal(bits(E), bits(wE))
    rep = [i for i, s in enumerate(expected["solver"]) if s.get("repeated_point")]
    assert len(rep) == 1 and n[rep[0]] == 0 and min(n[i] for i in range(len(n)) if i not in rep) > 0


def test_stage_gives_the_twins_bits(ref):
    got = ref["got"]
    assert len(got.results) == len(ref["names"]) == 13 and got.ms > 0.0
    for k, want in enumerate(ref["twin"]):
        same_pair(got.results[k], got.inliers(k), want)
    by = dict(zip(ref["names"], got.results))
    assert by["f5"]["ok"] == 0 and by["f5"]["n_matches"] == 5 and by["i"]["n_matches"] == 0
    assert by["f12"]["ok"] == 0 and by["h"]["n_matches"] == tw.MAX_LDS_M + 1
    assert by["j"]["n_matches"] == 41


def test_two_runs_and_any_batch_give_the_same_bits(ref):
    args, got = ref["args"], ref["got"]
    again = capi.RelPoses(**args)
    assert again.results.tobytes() == got.results.tobytes() and np.array_equal(again.inl_idx, got.inl_idx)
    n = len(ref["names"])
    rev = capi.RelPoses(**sc.sub_call(args, list(range(n))[::-1]))
    for k in range(n):
        assert rev.results[n - 1 - k].tobytes() == got.results[k].tobytes(), ref["names"][k]
        assert np.array_equal(rev.inliers(n - 1 - k), got.inliers(k))
    for k in range(n):
        one = capi.RelPoses(**sc.sub_call(args, [k]))
        assert one.results[0].tobytes() == got.results[k].tobytes(), ref["names"][k]
        assert np.array_equal(one.inliers(0), got.inliers(k))


def test_planted_outcomes(ref, expected):
    s, args, got = ref["s"], ref["args"], ref["got"]
    by = {n: k for k, n in enumerate(ref["names"])}
    for n in sc.MUST_BE_OK:
        assert got.results[by[n]]["ok"] == 1, n
    good = s["good"]["b"]
    inl = set(got.inliers(by["b"]).tolist())
    assert inl == set(np.nonzero(good)[0].tolist())          # every planted good match, no planted wrong one
    kpt, voff, off = args["kpt_xy"], args["view_off"].astype(np.int64), args["offsets"].astype(np.int64)
    for k, n in enumerate(ref["names"]):
        r = got.results[k]
        if not r["ok"]:
            continue
        vi, vj = int(args["pairs"][k][0]), int(args["pairs"][k][1])
        R, t = r["R"].reshape(3, 3), r["t"]
        assert np.abs(R.T @ R - np.eye(3)).max() <= sc.ROTATION_BOUND and abs(np.linalg.det(R) - 1.0) <= sc.ROTATION_BOUND
        assert abs(np.linalg.norm(t) - 1.0) <= sc.ROTATION_BOUND
        bi = tw.bearings(kpt[voff[vi]:voff[vi + 1]], args["intrinsics"][args["view_intrinsic"][vi]],
                         args["intrinsic_type"][args["view_intrinsic"][vi]])
        bj = tw.bearings(kpt[voff[vj]:voff[vj + 1]], args["intrinsics"][args["view_intrinsic"][vj]],
                         args["intrinsic_type"][args["view_intrinsic"][vj]])
        sel = off[k] + got.inliers(k).astype(np.int64)
        front = int(r["front"][r["choice"]])
        assert front == int(max(r["front"])) > 0
        if np.abs(sc.planted_pose(s, vi, vj)[1]).max() > 0.0:
            # a planted baseline: every inlier in front of both cameras, by the device's count and by NumPy's triangulation
            assert front == int(r["n_inliers"]), n
            d = sc.triangulate_depths(R, t, bi[args["match_i"][sel]], bj[args["match_j"][sel]])
            assert (d > 0.0).all(), n
        else:
            # no planted baseline (sfmloc.h "decision"): the points lie at infinity, the sign of a depth is the noise's, and
            # the pair is ok on front[choice] > 0 alone; what holds is that the count is the device's own triangulation's
            # (the twin's bits, test_stage_gives_the_twins_bits) and that it falls short of the inliers
            assert front < int(r["n_inliers"]), n
            assert front == tw.front_count(r["R"], t, bi[args["match_i"][sel]], bj[args["match_j"][sel]])[0]
        if n in expected["pose"]:
            Rp, tp = sc.planted_pose(s, vi, vj)
            e = expected["pose"][n]
            assert r["sample"].tolist() == e["sample"]
            assert np.abs(R - Rp).max() <= e["bound_R"] and np.abs(t - tp).max() <= e["bound_t"], n
    assert set(sc.MUST_BE_OK) <= set(expected["pose"])


def test_refusals_come_before_any_launch(ref):
    args = ref["args"]
    capi.RelPoses(**sc.sub_call(args, [0]))
    ms = capi.relpose_last_ms()
    assert ms > 0.0

    def refused(code, text, **change):
        a = dict(args)
        a.update(change)
        with pytest.raises(capi.SfmlocError) as ei:
            capi.RelPoses(**a)
        assert ei.value.code == code and text in ei.value.message, ei.value.message
        assert capi.relpose_last_ms() == ms
    pairs = args["pairs"].copy()
    pairs[2] = [1, 11]
    refused(capi.EINVAL, "pair 2 = (1, 11) out of range", pairs=pairs)
    pairs = args["pairs"].copy()
    pairs[3] = [2, 2]
    refused(capi.EINVAL, "pair 3 names view 2 twice", pairs=pairs)
    vi = args["view_intrinsic"].copy()
    vi[5] = 2
    refused(capi.EINVAL, "view 5 names intrinsic 2", view_intrinsic=vi)
    mj = args["match_j"].copy()
    mj[int(args["offsets"][1]) + 4] = 10 ** 6
    refused(capi.EINVAL, "pair (0, 2) match 4 out of range", match_j=mj)
    n = 65537
    big = dict(args, pairs=np.array([[0, 1]], np.uint32), offsets=np.array([0, n], np.uint64),
               match_i=np.zeros(n, np.uint32), match_j=np.zeros(n, np.uint32))
    with pytest.raises(capi.SfmlocError) as ei:
        capi.RelPoses(**big)
    assert ei.value.code == capi.ECAP and "pair (0, 1) has 65537 matches" in ei.value.message
    assert capi.relpose_last_ms() == ms


def test_empty_call(ref):
    e = capi.RelPoses(**sc.sub_call(ref["args"], []))
    assert len(e.results) == 0 and e.inl_off.tolist() == [0] and len(e.inl_idx) == 0


def test_tool_writes_the_calls_values_and_structure_reads_them(ref, tmp_path):
    s, got = ref["s"], ref["got"]
    written = {}
    for name, prog in PROGRAMS:                               # the two programs write the same bytes
        folder = str(tmp_path / name)
        os.makedirs(folder)
        path = sc.write_files(s, folder)
        r = subprocess.run(prog + ["-i", path, "-m", folder], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Relative poses: " in r.stdout
        written[name] = [open(os.path.join(folder, f), "rb").read() for f in ("matches.e.txt", "relative_poses.json")]
    assert written["cpp"] == written["py"]
    with open(os.path.join(folder, "relative_poses.json")) as fh:
        doc = json.load(fh)
    args = ref["args"]
    want = relpose.pose_entries(s["arrays"]["view_id"], args["pairs"], got.results)
    assert doc == {"relative_poses": want} and len(want) == int(sum(int(x["ok"]) for x in got.results))
    assert [(e["I"], e["J"]) for e in want] == sorted((e["I"], e["J"]) for e in want)
    for e, k in zip(want, [k for k in range(len(got.results)) if got.results[k]["ok"]]):
        assert np.array_equal(bits(np.array(e["R"]).ravel()), bits(got.results[k]["R"]))      # json.dump round-trips
    em = fileio.read_matches_txt(os.path.join(folder, "matches.e.txt"))
    wm = relpose.essential_matches(s["arrays"]["view_id"], args["pairs"], args["offsets"], args["match_i"], args["match_j"],
                                   got)
    assert sorted(em) == sorted(wm)
    for key in wm:
        assert np.array_equal(em[key][0], wm[key][0]) and np.array_equal(em[key][1], wm[key][1])
        assert list(zip(em[key][0].tolist(), em[key][1].tolist())) == sorted(zip(em[key][0].tolist(), em[key][1].tolist()))
    # the consumer: the structure tool reads the essential matches (poses planted as extrinsics)
    doc = dict(s["doc"])
    doc["extrinsics"] = [{"key": sc.VIEW_ID[k], "value": {"rotation": s["poses"][k][0].tolist(),
                                                          "center": s["poses"][k][1].tolist()}} for k in range(sc.N_VIEWS)]
    posed = os.path.join(folder, "posed.json")
    with open(posed, "w") as fh:
        json.dump(doc, fh)
    out = os.path.join(folder, "structure.json")
    assert structure.run(posed, folder, out, match_file="matches.e.txt", log=lambda *_: None) == 0
    with open(out) as fh:
        st = json.load(fh)["structure"]
    assert len(st) > 1000                                     # (pair h alone has more than 2000 two-view tracks)


def test_timing_tool_on_a_short_corridor(tmp_path):
    """tools/relpose_time.py at 40 views: the record's fields, and the restatement's subset with the device's bits"""
    out = str(tmp_path / "time.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "relpose_time.py"), "--views", "40", "--repeats", "1",
                        "--out", out, "--commit", "test"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fh:
        rec = json.load(fh)
    assert rec["views"] == 40 and rec["pairs"] > 100 and rec["device_ms"]["best"] > 0.0
    assert rec["pairs_per_s_device"] == rec["pairs"] / (rec["device_ms"]["best"] * 1e-3)
    assert 0 < rec["pairs_ok"] <= rec["pairs"] and rec["numpy_restatement"]["same_bits_as_device"] is True
    assert 1 <= rec["rounds"]["per_pair"]["min"] <= rec["rounds"]["per_pair"]["max"] <= 256
