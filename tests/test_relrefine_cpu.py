"""CPU: the NumPy restatement of the two-view refinement (tests/relrefine_np.py) on the relative-pose scene, fed by the
restatement of the relative poses: its final cost against the independent reference's (SciPy's least_squares,
tests/relrefine_independent.py, recorded in tests/golden/relrefine/expected.json by
tests/golden/make_relrefine_fixtures.py), the planted poses, the pair without a baseline, the gates; the tool's
argument and its output schema; the refusals, which need no device; and the host side under the host sanitizers."""
import ctypes as C
import json
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

import relpose_np as rp_tw  # noqa: E402
import relpose_scene as sc  # noqa: E402
import relrefine_cases as cases  # noqa: E402
import relrefine_np as tw  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import _abi, capi, globalsfm, relpose  # noqa: E402

EXPECTED = os.path.join(HERE, "golden", "relrefine", "expected.json")
RELPOSE_EXPECTED = os.path.join(HERE, "golden", "relpose", "expected.json")
EPS = float(np.finfo(np.float64).eps)
# How far R^T R may move from I in one step (max-norm), by reasoning, not by measurement.  C(w) is orthogonal in exact
# arithmetic.  An entry of the computed C(w) carries at most 8 roundings (w.w 3, the factor 2, the product w_i w_j, the
# difference and the two sums 3) of eps / 2 each on magnitudes below 2: 8 eps.  An entry of C^T C is a sum of three
# products of such entries: 2 x 3 x 8 = 48 eps.  The product C R rounds five times per entry (three products, two sums)
# on magnitudes below 1: 2.5 eps per entry, 2 x 3 x 2.5 = 15 eps in R^T R.  63 eps, rounded up to a power of two, per
# step tried (a step that is not accepted changes nothing); the start is within relpose_scene.ROTATION_BOUND.
ROTATION_STEP_BOUND = 64 * EPS


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def run():
    """the scene, its call (use_pair = ok), the pair names, the twin's results by name -- computed once, never changed"""
    s = sc.make_scene()
    args, names = sc.call_arrays(s)
    call = cases.call_from_twin(args, rp_tw.relative_poses(**args))
    out = tw.refine_relative_poses(**call)
    return dict(scene=s, args=args, names=names, call=call, out=dict(zip(names, out)), index={n: k for k, n in enumerate(names)})


def planted_distance(run, name, R, t):
    k = run["index"][name]
    Rp, tp = sc.planted_pose(run["scene"], int(run["args"]["pairs"][k][0]), int(run["args"]["pairs"][k][1]))
    return float(np.abs(np.asarray(R).reshape(3, 3) - Rp).max()), float(np.abs(np.asarray(t) - tp).max())


def test_cost_is_at_most_the_independent_references(run, expected):
    """a, b, c, d, e, j and h: the twin ends at or below the cost SciPy's least_squares reaches on the same residuals, within
    margin = 10 x the reference's own reproducibility (its runs at tolerances 1e-12 and 1e-15), at least 1e-12"""
    assert expected["margin_floor"] == 1e-12
    for name in ("a", "b", "c", "d", "e", "j", "h"):
        e, o = expected["pairs"][name], run["out"][name]
        assert e["margin"] == max(10.0 * e["repro"], 1e-12)
        assert o["status"] in (1, 3) and o["n_used"] == e["n_used"]
        print(name, "twin", o["cost"], "reference", e["ref_cost"], "margin", e["margin"], "ratio - 1",
              o["cost"] / e["ref_cost"] - 1.0)
        assert o["cost"] <= e["ref_cost"] * (1.0 + e["margin"]), name


def test_cost_never_rises(run):
    n = 0
    for name, o in run["out"].items():
        if o["status"] in (1, 3):
            assert np.isfinite(o["cost"]) and 0.0 <= o["cost"] <= o["cost_initial"], name
            n += 1
        else:
            assert o["cost"] == o["cost_initial"], name
    assert n >= 9


def test_refined_pose_is_closer_to_the_planted_one_than_the_sample(run):
    """dR and dt below the sample's (twin_dR, twin_dt of tests/golden/relpose/expected.json) for a, b, c, e; for j the
    sample's distances are computed here.  Pairs d and f13 are left out on purpose: on the CPU the independent reference
    itself does not move d's rotation closer (forward motion: the epipole is inside the image and the rotation is already
    at 1.1e-4), nor f13's pose (13 inliers); see ref_dR, ref_dt, sample_dR, sample_dt of tests/golden/relrefine/expected.json."""
    with open(RELPOSE_EXPECTED) as fh:
        sample = json.load(fh)["pose"]
    for n in ("a", "b", "c", "e", "j"):
        k, o = run["index"][n], run["out"][n]
        dR, dt = planted_distance(run, n, o["R"], o["t"])
        if n == "j":
            sR, st = planted_distance(run, n, run["call"]["rel_R"][k], run["call"]["rel_t"][k])
        else:
            sR, st = sample[n]["twin_dR"], sample[n]["twin_dt"]
        print(n, "dR", sR, "->", dR, "dt", st, "->", dt)
        assert o["status"] == 1 and dR < sR and dt < st, n


def test_pair_without_a_baseline_stays_a_rotation(run):
    """g (pure rotation): the points lie at infinity, the translation means nothing and nothing is asked of it"""
    o = run["out"]["g"]
    assert o["status"] in (1, 3) and o["n_used"] == 37
    assert all(np.isfinite(o[f]).all() for f in ("R", "t", "E", "cost", "cost_initial"))
    R = o["R"].reshape(3, 3)
    bound = sc.ROTATION_BOUND + ROTATION_STEP_BOUND * o["steps"]
    assert np.abs(R.T @ R - np.eye(3)).max() <= bound and abs(np.linalg.det(R) - 1.0) <= bound


def test_gates(run):
    call, k = run["call"], run["index"]["a"]
    few, enough = (tw.refine_relative_poses(**cases.sub_call(call, [k], first=[n]))[0] for n in (12, 13))
    assert few["status"] == 2 and few["n_used"] == 12 and few["steps"] == 0 and few["cost"] == few["cost_initial"] == 0.0
    assert np.array_equal(few["R"], call["rel_R"][k]) and np.array_equal(few["t"], call["rel_t"][k])
    assert enough["status"] in (1, 3) and enough["n_used"] == 13 and enough["steps"] >= 1
    assert enough["cost"] < enough["cost_initial"]
    off = tw.refine_relative_poses(**cases.sub_call(call, [k], use=[0]))[0]
    assert off["status"] == 0 and off["n_used"] == 0 and off["steps"] == 0 and off["cost"] == off["cost_initial"] == 0.0
    assert np.array_equal(off["R"], call["rel_R"][k]) and np.array_equal(off["t"], call["rel_t"][k])
    E = off["E"].reshape(3, 3)
    t, R = call["rel_t"][k], call["rel_R"][k].reshape(3, 3)
    tx = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]])
    assert abs(np.linalg.norm(E) - 1.0) < 8 * EPS and np.abs(E - tx @ R / np.linalg.norm(tx @ R)).max() < 8 * EPS
    for name in ("f5", "f6", "f12", "i"):                       # not ok: not asked
        assert run["out"][name]["status"] == 0
    assert np.array_equal(run["out"]["i"]["E"], np.zeros(9))    # (no pose at all: t = 0)
    assert tw.refine_relative_poses(**cases.sub_call(call, [k], first=[13], use=[1]), min_points=14)[0]["status"] == 2
    one = tw.refine_relative_poses(**cases.sub_call(call, [k]), max_steps=1)[0]
    assert one["status"] == 3 and one["steps"] == 1 and one["cost"] < one["cost_initial"]


def test_host_side_under_the_host_sanitizers(tmp_path):
    """tests/cpp/relrefine_host.cpp: a stand-alone host program, CPU only, every refusal.  Where a HIP device is visible
    the program is built without the sanitizers (they are for CPU machines); it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/relrefine_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "relrefine_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "relrefine_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_relrefine_\w+|sfmloc_refine_relative_poses)\s*\(", hdr))
    assert names == {"sfmloc_relrefine_default_options", "sfmloc_refine_relative_poses", "sfmloc_relrefine_results",
                     "sfmloc_relrefine_destroy", "sfmloc_relrefine_last_ms"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    o = capi.relrefine_default_options()
    assert {k: getattr(o, k) for k in tw.OPTIONS} == tw.OPTIONS == dict(max_steps=100, min_points=13)
    rec = _abi.struct("sfmloc_relrefine_result")
    assert capi.RELREFINE_RESULT.itemsize == C.sizeof(rec) == 16 + 23 * 8
    assert [capi.RELREFINE_RESULT.fields[f][1] for f, _ in rec._fields_] == [getattr(rec, f).offset for f, _ in rec._fields_]
    with pytest.raises(AttributeError):
        capi.relrefine_default_options(max_step=3)


def test_refusals_need_no_device(run):
    """every check of sfmloc_refine_relative_poses happens before anything is launched"""
    call = run["call"]
    bad_R, bad_inl, bad_mj = call["rel_R"].copy(), call["inl_idx"].copy(), call["match_j"].copy()
    bad_R[1, 4] = np.nan
    bad_inl[int(call["inl_off"][2]) + 3] = 60000
    bad_mj[2] = 5000
    for change, code, text in (
            (dict(max_steps=0), capi.EINVAL, "sfmloc_refine_relative_poses: max_steps = 0"),
            (dict(min_points=5), capi.EINVAL, "sfmloc_refine_relative_poses: min_points = 5"),
            (dict(rel_R=bad_R), capi.EINVAL, "sfmloc_refine_relative_poses: pair (0, 2) has a non-finite rel_R or rel_t"),
            (dict(inl_idx=bad_inl), capi.EINVAL, "sfmloc_refine_relative_poses: pair (1, 2) inlier 3 out of range"),
            (dict(match_j=bad_mj), capi.EINVAL, "sfmloc_refine_relative_poses: pair (0, 1) match 2 out of range"),
            (dict(intrinsic_type=[0, 2]), capi.EINVAL, "sfmloc_refine_relative_poses: intrinsic 1 has type 2")):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.RelRefine(**{**call, **change})
        assert ei.value.code == code and text in ei.value.message, ei.value.message
    for change in (dict(rel_R=call["rel_R"][:2]), dict(inl_off=call["inl_off"][:3]), dict(use_pair=[1, 1])):
        with pytest.raises(ValueError):
            capi.RelRefine(**{**call, **change})


def test_committed_records():
    """profiles/relrefine_time.json and relrefine_parity.json: what tools/relpose_time.py --refine wrote on the corridor
    of 10 000 views; and the kernel's resource remarks"""
    with open(os.path.join(ROOT, "profiles", "relrefine_time.json")) as fh:
        rec = json.load(fh)
    f = rec["refine"]
    assert rec["views"] == 10000 and rec["pairs"] > 40000 and rec["numpy_restatement"]["same_bits_as_device"] is True
    assert f["device_ms"]["best"] == min(f["device_ms"]["all"]) > 0.0 and f["relative_poses_device_ms"] > 0.0
    assert sum(f["status_count"].values()) == rec["pairs"] and f["pairs_asked"] == rec["pairs_ok"]
    assert 1 <= f["steps_per_pair"]["min"] <= f["steps_per_pair"]["median"] <= f["steps_per_pair"]["max"] <= 100
    assert f["numpy_restatement"]["same_bits_as_device"] is True
    with open(os.path.join(ROOT, "profiles", "relrefine_parity.json")) as fh:
        par = json.load(fh)
    assert par["views"] == 10000 and {"pair_rotation_error_deg", "rotation_drift_deg"} <= set(par["sample"]) == set(par["refined"])
    with open(os.path.join(ROOT, "profiles", "relrefine_resources.txt")) as fh:
        text = fh.read()
    assert "k_relrefine" in text and "VGPRs Spill: 0" in text and "ScratchSize" in text


def test_tool_argument_and_schema(capsys):
    base = ["-i", "a.json", "-m", "dir"]
    assert "refine" not in relpose.parse_args(base)
    assert relpose.parse_args(base + ["--refine"]) == {**relpose.parse_args(base), "refine": True}
    assert relpose.parse_args(["--refine", "-s", "s.json"] + base) == {**relpose.parse_args(base), "refine": True,
                                                                        "scales_file": "s.json"}
    assert relpose.parse_args(base + ["--refine", "1"]) is None and "--refine" in relpose.USAGE
    g = ["-i", "a.json", "-m", "dir", "-o", "out"]
    assert globalsfm.parse_args(g + ["--refine"]) == {**globalsfm.parse_args(g), "refine": True}
    assert globalsfm.parse_args(g + ["--refine", "--pair-scales"]) == {**globalsfm.parse_args(g), "refine": True,
                                                                        "pair_scales": True}
    assert "refine" not in globalsfm.parse_args(g) and "--refine" in globalsfm.USAGE
    res = np.zeros(3, capi.RELPOSE_RESULT)
    res["ok"] = [1, 0, 1]
    res["R"][0], res["E"][0], res["t"][0] = np.arange(9) / 7.0, np.arange(9) / 3.0, [0.1, 0.2, 0.3]
    res["R"][2], res["t"][2] = np.arange(9) / 11.0, [0.3, 0.2, 0.1]
    fine = np.zeros(3, capi.RELREFINE_RESULT)
    fine["status"], fine["n_used"], fine["steps"] = [1, 0, 4], [58, 0, 39], [9, 0, 2]
    fine["R"][0], fine["E"][0], fine["t"][0] = np.arange(9) / 13.0, np.arange(9) / 17.0, [0.4, 0.5, 0.6]
    fine["R"][2] = 9.0
    fine["cost_initial"][0], fine["cost"][0] = 0.25, 0.125
    assert relpose.pose_entries([4, 9, 11], [(0, 1), (0, 2), (1, 2)], res) == \
        relpose.pose_entries([4, 9, 11], [(0, 1), (0, 2), (1, 2)], res, None)
    out = json.loads(json.dumps(relpose.pose_entries(np.array([4, 9, 11]), [(0, 1), (0, 2), (1, 2)], res, fine)))
    assert [(e["I"], e["J"]) for e in out] == [(4, 9), (9, 11)] and list(out[0])[-1] == "refine"
    assert out[0]["refine"] == {"status": 1, "n_used": 58, "steps": 9, "cost_initial": 0.25, "cost": 0.125}
    assert np.array_equal(np.array(out[0]["R"]), (np.arange(9) / 13.0).reshape(3, 3)) and out[0]["t"] == [0.4, 0.5, 0.6]
    assert np.array_equal(np.array(out[0]["E"]), (np.arange(9) / 17.0).reshape(3, 3))
    assert out[1]["refine"]["status"] == 4 and out[1]["t"] == [0.3, 0.2, 0.1]          # not moved: the sample's pose
    assert np.array_equal(np.array(out[1]["R"]), (np.arange(9) / 11.0).reshape(3, 3))
    R, t = relpose.refined_poses(res, fine)
    assert np.array_equal(R[0], fine["R"][0]) and np.array_equal(R[2], res["R"][2]) and np.array_equal(t[0], fine["t"][0])
