"""CPU: the NumPy restatement of the relative poses (tests/relpose_np.py) against a second, independent five-point solver
and decomposition (tests/relpose_independent.py) within the bounds of tests/golden/relpose/expected.json
(tests/golden/make_relpose_fixtures.py says how each was measured: 1000 x the problem's own conditioning); the tool's
argument parsing and output schema; the refusals, which need no device; and the host side of the call under the host
sanitizers."""
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

import relpose_independent as ind  # noqa: E402
import relpose_np as tw  # noqa: E402
import relpose_scene as sc  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import _abi, capi, relpose  # noqa: E402

EXPECTED = os.path.join(HERE, "golden", "relpose", "expected.json")


@pytest.fixture(scope="module")
def expected():
    with open(EXPECTED) as fh:
        return json.load(fh)


def test_twin_models_match_the_independent_solver(expected):
    assert expected["factor"] == 1000.0
    for s in expected["solver"]:
        x1, x2 = np.array(s["x1"]).reshape(5, 2), np.array(s["x2"]).reshape(5, 2)
        nm, E = tw.five_point(x1[None], x2[None])
        ref = ind.five_point(x1, x2)
        if s.get("repeated_point"):
            assert nm[0] == 0
            continue
        assert s["bound"] == 1000.0 * s["cond"] and s["separation"] > s["bound"] > 0.0
        assert nm[0] == len(ref) == s["n_ref"] > 0
        for k in range(nm[0]):
            assert abs(np.linalg.norm(E[0, k]) - 1.0) < 1e-15 * 8
            assert ind.align_distance(E[0, k], ref) <= s["bound"]
        assert ind.align_distance(s["E_planted"], ref) <= s["bound"]
        assert ind.align_distance(s["E_planted"], E[0, :nm[0]]) <= s["bound"]


def test_twin_decomposition_matches_the_svd(expected):
    """the four candidates against numpy.linalg.svd's, within 1000 x the decomposition's own one-ulp conditioning
    (decompose_bound of expected.json); R a rotation within sc.ROTATION_BOUND"""
    n = 0
    for s in expected["solver"]:
        if s.get("repeated_point"):
            continue
        assert s["decompose_bound"] == 1000.0 * s["decompose_cond"] > 0.0
        E = np.array(s["E_planted"])
        R4, t4 = tw.decompose(E)
        ref = ind.decompose(E)
        for c in range(4):                                     # the same four candidates, in some order
            Rc = R4[c].reshape(3, 3)
            d = min(np.abs(Rc - R).max() + np.abs(t4[c] - t).max() for R, t in ref)
            assert d <= s["decompose_bound"]
            assert np.abs(Rc.T @ Rc - np.eye(3)).max() <= sc.ROTATION_BOUND
            assert abs(np.linalg.det(Rc) - 1.0) <= sc.ROTATION_BOUND
            assert abs(np.linalg.norm(t4[c]) - 1.0) <= sc.ROTATION_BOUND
        assert np.array_equal(R4[0], R4[1]) and np.array_equal(t4[0], -t4[1]) and np.array_equal(t4[0], t4[2])
        n += 1
    assert n >= 10


def test_twin_poses_within_the_independent_solvers_own_error(expected):
    s = sc.make_scene()
    args, names = sc.call_arrays(s)
    keep = [k for k, n in enumerate(names) if n in ("a", "b", "d", "f5", "f6", "f12", "f13", "i")]
    res = tw.relative_poses(**sc.sub_call(args, keep))
    for k, r in zip(keep, res):
        n = names[k]
        if n in ("f5", "i"):
            assert r["ok"] == 0 and r["n_inliers"] == 0 and r["rounds"] == 0
            continue
        if n in ("f6", "f12"):
            assert r["ok"] == 0 and r["n_inliers"] <= 12        # 2.5 x 5 = 12.5: twelve inliers are not enough
            continue
        assert r["ok"] == 1
        e = expected["pose"][n]
        Rp, tp = sc.planted_pose(s, int(args["pairs"][k][0]), int(args["pairs"][k][1]))
        assert r["sample"].tolist() == e["sample"]
        assert np.abs(r["R"].reshape(3, 3) - Rp).max() <= e["bound_R"]
        assert np.abs(r["t"] - tp).max() <= e["bound_t"]
        assert e["bound_R"] == e["ref_dR"] + 1000.0 * e["cond_R"] and e["bound_t"] == e["ref_dt"] + 1000.0 * e["cond_t"]
        if n == "b":
            assert set(r["inliers"].tolist()) == set(np.nonzero(s["good"]["b"])[0].tolist())


def test_sampler_is_keyed_by_the_pair_and_gives_sorted_distinct_positions():
    a = tw.sample5(60, tw.SEED, 3, 7, np.arange(200))
    assert (np.diff(a, axis=1) > 0).all() and a.min() >= 0 and a.max() < 60
    assert not np.array_equal(a, tw.sample5(60, tw.SEED, 7, 3, np.arange(200)))
    assert not np.array_equal(a, tw.sample5(60, tw.SEED + 1, 3, 7, np.arange(200)))
    assert np.array_equal(a[50:60], tw.sample5(60, tw.SEED, 3, 7, np.arange(50, 60)))
    assert (np.sort(tw.sample5(6, tw.SEED, 0, 1, np.arange(300)), axis=1).max(1) <= 5).all()


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_relpose_\w+|sfmloc_relative_poses|sfmloc_debug_five_point)\s*\(", hdr))
    assert names == {"sfmloc_relpose_default_options", "sfmloc_relative_poses", "sfmloc_relpose_results",
                     "sfmloc_relpose_inliers", "sfmloc_relpose_destroy", "sfmloc_relpose_last_ms", "sfmloc_debug_five_point"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    assert L.sfmloc_abi_version() == 2
    o = capi.relpose_default_options()
    assert (o.max_iteration, o.precision_px, o.seed) == (256, 2.5, tw.SEED)
    # sizes and every field offset of sfmloc_relpose_options / _result (RELPOSE_RESULT's E and nfa among them) against
    # the compiler: tests/test_abi.py; what stays here is that the record and the bound struct are one layout
    assert capi.RelposeOptions is _abi.struct("sfmloc_relpose_options")
    res = _abi.struct("sfmloc_relpose_result")
    assert [C.sizeof(capi.RelposeOptions), capi.RELPOSE_RESULT.itemsize, capi.RELPOSE_RESULT.fields["E"][1],
            capi.RELPOSE_RESULT.fields["nfa"][1]] == [24, C.sizeof(res), res.E.offset, res.nfa.offset]


def test_refusals_need_no_device():
    """every check of sfmloc_relative_poses happens before anything is launched: the refusals come back without a GPU"""
    base = dict(view_off=[0, 3, 6], kpt_xy=np.zeros((6, 2), np.float32), view_wh=[[640, 480]] * 2, view_intrinsic=[0, 0],
                intrinsics=[[700.0, 320.0, 240.0, 0, 0, 0]], intrinsic_type=[0])
    for extra, code, text in (
            (dict(pairs=[[0, 2]], offsets=[0, 1], match_i=[0], match_j=[0]), capi.EINVAL, "pair 0 = (0, 2) out of range"),
            (dict(pairs=[[1, 1]], offsets=[0, 1], match_i=[0], match_j=[0]), capi.EINVAL, "pair 0 names view 1 twice"),
            (dict(pairs=[[0, 1]], offsets=[0, 2], match_i=[0, 1], match_j=[0, 3]), capi.EINVAL,
             "pair (0, 1) match 1 out of range"),
            (dict(pairs=[[0, 1]], offsets=[0, 65537], match_i=np.zeros(65537), match_j=np.zeros(65537)), capi.ECAP,
             "pair (0, 1) has 65537 matches"),
            (dict(pairs=[[0, 1]], offsets=[0, 1], match_i=[0], match_j=[0], view_intrinsic=[0, 1]), capi.EINVAL,
             "view 1 names intrinsic 1 of 1")):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.RelPoses(**{**base, **extra})
        assert ei.value.code == code and text in ei.value.message


def test_host_side_under_the_host_sanitizers(tmp_path):
    """tests/cpp/relpose_host.cpp: a stand-alone host program, CPU only.  Where a HIP device is visible the program is
    built without the sanitizers (they are for CPU machines); it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/relpose_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "relpose_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "relpose_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_shared_scene_checks_under_the_host_sanitizers(tmp_path):
    """tests/cpp/pair_scene.cpp: csrc/pair_scene.h, the checks the four pair-side calls share, under each caller's name
    and switches and with two faults at once; a stand-alone host program, CPU only, built as the one above"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/pair_scene.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "pair_scene")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pair_scene.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_host_instantiation_of_the_solver_gives_the_twins_bits(tmp_path, expected):
    """tests/cpp/essential_host.cpp: csrc/essential_device.h compiled for the host (the lanes of a group one after the
    other), unfused as the library is, on the fixture's samples and a seeded batch: the restatement's counts and bits"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/essential_host.cpp")
    exe = str(tmp_path / "essential_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "essential_host.cpp")], check=True, timeout=300)
    rng = np.random.Generator(np.random.PCG64(5))
    rows = np.concatenate([np.array([s["x1"] + s["x2"] for s in expected["solver"]]), rng.uniform(-0.4, 0.4, (24, 20)),
                           np.zeros((1, 20))])
    with open(tmp_path / "in.bin", "wb") as fh:
        fh.write(np.int32(len(rows)).tobytes())
        fh.write(rows.tobytes())
    r = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("OK"), r.stdout[-2000:] + r.stderr[-2000:]
    out = np.fromfile(tmp_path / "out.bin", np.float64).reshape(len(rows), 91)
    nm, E = tw.five_point(rows[:, :10].reshape(-1, 5, 2), rows[:, 10:].reshape(-1, 5, 2))
    assert out[:, 0].astype(np.int64).tolist() == nm.tolist() and nm.max() >= 4 and nm[-1] == 0
    assert np.array_equal(np.ascontiguousarray(out[:, 1:]).view(np.uint64), E.reshape(len(rows), 90).view(np.uint64))


def test_tool_argument_parsing(tmp_path, capsys):
    kw = relpose.parse_args(["-i", "a.json", "-m", "dir"])
    assert kw == dict(in_path="a.json", match_dir="dir", match_file="matches.f.txt", out_file="matches.e.txt",
                      poses_file="relative_poses.json", max_iteration=256, precision_px=2.5, seed=None, device=0)
    kw = relpose.parse_args(["--input_file", "a.json", "--match_dir", "d", "-f", "m.txt", "-o", "e.txt", "-p", "p.json", "-n",
                             "64", "-t", "1.5", "--seed", "0x10", "--device=1"])
    assert (kw["match_file"], kw["out_file"], kw["poses_file"], kw["max_iteration"], kw["precision_px"], kw["seed"],
            kw["device"]) == ("m.txt", "e.txt", "p.json", 64, 1.5, 16, 1)
    for bad in (["-i", "a.json"], ["-m", "d"], ["-i", "a", "-m", "d", "-n", "x"], ["-i", "a", "-m", "d", "--what"],
                ["-i", "a", "-m", "d", "-t"], ["-i", "a", "-m", "d", "-t", "-1"]):
        assert relpose.parse_args(bad) is None
        assert relpose.main(bad) == 1
        assert relpose.NAME in capsys.readouterr().err
    s = sc.make_scene()
    path = sc.write_files(s, str(tmp_path))
    assert relpose.main(["-i", path, "-m", str(tmp_path), "-f", "nothing.txt"]) == 1
    assert "Invalid matches file." in capsys.readouterr().err
    assert relpose.main(["-i", str(tmp_path / "none.json"), "-m", str(tmp_path)]) == 1
    assert "cannot be read" in capsys.readouterr().err
    assert not os.path.exists(os.path.join(str(tmp_path), "matches.e.txt"))


def test_relative_poses_json_schema():
    res = np.zeros(3, capi.RELPOSE_RESULT)
    res["ok"] = [1, 0, 1]
    res["n_matches"], res["n_inliers"] = [60, 6, 40], [58, 6, 39]
    res["R"][0], res["E"][0], res["t"][0] = np.arange(9) / 7.0, np.arange(9) / 3.0, [0.1, 0.2, 0.3]
    res["front"][0], res["choice"][0], res["error_max_px"][0] = [0, 0, 58, 0], 2, 0.75
    out = relpose.pose_entries(np.array([4, 9, 11]), [(0, 1), (0, 2), (1, 2)], res)
    assert [(e["I"], e["J"]) for e in out] == [(4, 9), (9, 11)]
    e = json.loads(json.dumps({"relative_poses": out}))["relative_poses"][0]
    assert sorted(e) == sorted(["I", "J", "n_matches", "n_inliers", "R", "t", "E", "error_max", "front", "choice"])
    assert np.array_equal(np.array(e["R"]), (np.arange(9) / 7.0).reshape(3, 3)) and e["front"] == [0, 0, 58, 0]
    assert (e["n_matches"], e["n_inliers"], e["choice"], e["error_max"], e["t"]) == (60, 58, 2, 0.75, [0.1, 0.2, 0.3])


def test_committed_timing_record():
    """profiles/relpose_time.json: what tools/relpose_time.py wrote on the corridor of 10 000 views"""
    with open(os.path.join(ROOT, "profiles", "relpose_time.json")) as fh:
        rec = json.load(fh)
    assert rec["views"] == 10000 and rec["pairs"] > 40000 and rec["matches"] > 5 * 10 ** 7
    assert rec["device_ms"]["best"] == min(rec["device_ms"]["all"]) > 0.0
    assert abs(rec["pairs_per_s_device"] - rec["pairs"] / (rec["device_ms"]["best"] * 1e-3)) < 1e-6
    assert rec["numpy_restatement"]["same_bits_as_device"] is True and rec["rounds"]["per_pair"]["max"] <= 256
    assert "OpenMVG was not run" in rec["note"]
