"""CPU: the NumPy restatement of the global poses (tests/globalposes_np.py) against the planted truth of
tests/globalposes_scene.py within the figures of tests/golden/globalposes/expected.json
(tests/golden/make_globalposes_fixtures.py says how each was measured), its two solvers against each other, the
committed parity record, the tool's argument parsing and id mapping, the refusals, which need no device, and the host
side of the call under the host sanitizers."""
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
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, ROOT)

import globalposes_np as tw  # noqa: E402
import globalposes_scene as sc  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from make_globalposes_fixtures import FLOOR, bound, distances, run  # noqa: E402
from sfmlocalization_amd import _abi, capi, globalposes  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "globalposes")
PARITY = os.path.join(ROOT, "profiles", "globalposes_parity.json")
QUANTITIES = {"R", "C", "rot_residual", "trans_residual", "cost"}


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "expected.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def small():
    """the scenes (a) and (b) and the restatement's two results on each: computed once, left unchanged"""
    out = {}
    for name, make in (("triplet", sc.scene_triplet), ("ring", sc.scene_ring)):
        s = make()
        out[name] = (s, run(s, "pcg"), run(s, "dense"))
    return out


@pytest.mark.parametrize("name", ["triplet", "ring"])
def test_restatement_recovers_the_planted_poses(small, expected, name):
    s, a, _ = small[name]
    rot, cen = sc.errors(s, a["in_component"], a["root"], a["R"], a["C"])
    e = expected[name]
    assert (rot, cen) == pytest.approx((e["rotation_deg"], e["centre"]), rel=1e-6)
    # the planted noise is 0.2 / 0.4 degrees per pair and 0.005 / 0.01 rad per direction: the average is no worse
    assert rot <= {"triplet": 0.2, "ring": 0.4}[name] and cen <= {"triplet": 0.005, "ring": 0.01}[name]
    assert (a["n_component_views"], a["root"], a["n_pairs_kept"], a["n_triplets_total"], a["n_triplets_ok_total"]) == \
        (e["n_component_views"], e["root"], e["n_pairs_kept"], e["n_triplets"], e["n_triplets_ok"])
    assert a["rot_stop"] in (0, 2) and a["trans_stop"] == 0 and a["chordal_stop"] == 0
    assert a["trans_cost_final"] < a["trans_cost_initial"] and a["rot_cost_final"] <= a["rot_cost_initial"]


def test_restatement_on_the_planted_faults(small):
    s, a, _ = small["ring"]
    assert not a["kept"][s["wrong"]].any() and a["n_triplets"][s["wrong"]].all()
    assert not a["in_component"][s["pendant"]] and not a["in_component"][s["other_component"]].any()
    assert a["in_component"][:12].all()
    assert a["kept"][s["rotation_only"]] and not a["used_t"][s["rotation_only"]]
    assert (a["n_rotation_pairs"], a["n_translation_pairs"]) == (33, 32)


def test_expected_figures_of_the_large_scene(expected):
    """scene (c) is run by the fixture maker only (half a minute): its figures are of the planted noise's size, and the
    scene crosses what it is there to cross"""
    e = expected["large"]
    assert e["rotation_deg"] <= 0.6 and e["centre"] <= 0.01 and e["n_component_views"] == 1101
    s = sc.scene_large()
    off, nbr, pe = tw.adjacency(s["n_views"], s["pairs"])
    deg = np.diff(off.astype(np.int64))
    assert s["n_views"] > 4 * 256 and deg[s["hub"]] == 300 > 64 and (deg[:s["hub"]] <= 64).all()
    assert all((np.diff(nbr[off[v]:off[v + 1]].astype(np.int64)) > 0).all() for v in (0, 5, s["hub"]))
    with np.load(os.path.join(GOLDEN, "scene_large.npz")) as z:
        assert z["R"].shape == (1101, 3, 3) and int(z["in_component"].sum()) == 1101 and int(z["kept"].sum()) == e["n_pairs_kept"]


@pytest.mark.parametrize("name", ["triplet", "ring"])
def test_two_solvers_leave_what_the_record_says(small, expected, name):
    s, a, b = small[name]
    d = distances(s, a, b)
    with open(PARITY) as fh:
        doc = json.load(fh)
    assert set(d) == QUANTITIES == set(doc["twin_" + name]) == set(expected["chain"]["parity"])
    assert "bound" not in doc and doc["floor"] == FLOOR == 16 * np.finfo(np.float64).eps
    for q in QUANTITIES:
        assert doc["twin_" + name][q] == expected[name]["parity"][q]
        # the same run on another machine's BLAS: the figure's size, not its bits
        assert d[q] <= 10.0 * max(expected[name]["parity"][q], 1e-14)
        # every scene is held to its own figure, never below the floor, and the bound stays a solver's, not a scene's
        assert bound(doc["twin_" + name])[q] == 4.0 * max(doc["twin_" + name][q], FLOOR) < 1e-6
    for f in ("n_triplets", "n_triplets_ok", "kept", "used_t", "in_component"):
        assert np.array_equal(a[f], b[f])
    assert (a["rot_steps_tried"], a["trans_steps_tried"]) == (b["rot_steps_tried"], b["trans_steps_tried"]) == \
        tuple(expected[name]["steps"])


def test_pcg_follows_the_stated_rule():
    rng = np.random.default_rng(5)
    M = rng.normal(size=(12, 12))
    A = M @ M.T + 12 * np.eye(12)
    b = rng.normal(size=(12, 1))
    x, it, stop, res = tw.pcg(lambda p: A @ p, lambda r: r / np.diag(A)[:, None], b, 1e-8, 100)
    assert stop == 0 and it <= 12 and res <= 1e-8 and np.allclose(x, np.linalg.solve(A, b), atol=1e-8)
    assert tw.pcg(lambda p: A @ p, lambda r: r, b, 1e-30, 3)[1:3] == (3, 1)              # max_pcg
    assert tw.pcg(lambda p: -(A @ p), lambda r: r, b, 1e-8, 100)[1:3] == (0, 2)           # p.Ap not positive
    assert tw.pcg(lambda p: A @ p, lambda r: r, np.zeros((12, 1)), 1e-8, 100)[1:3] == (0, 0)


def test_pieces_of_the_restatement():
    rng = np.random.default_rng(7)
    R = sc.random_rotation(rng, 1.0)
    noisy = R + 1e-3 * rng.normal(size=(3, 3))
    P = tw.nearest_rotation(noisy)
    U, _, Vt = np.linalg.svd(noisy)
    assert np.allclose(P, U @ Vt, atol=1e-12) and np.linalg.det(P) > 0
    assert np.linalg.det(tw.nearest_rotation(noisy @ np.diag([1.0, 1.0, -1.0]))) > 0
    x = np.array([0.02, -0.05, 0.01])
    Cx = tw.cayley(x)
    assert np.allclose(Cx @ Cx.T, np.eye(3), atol=1e-15)
    g, ok = tw.gibbs(np.stack([np.eye(3), np.eye(3)]), np.array([0]), np.array([1]), Cx[None])
    assert ok.all() and np.allclose(g[0], x, atol=1e-15)                       # |g| = tan(theta / 2), g of Cayley(x) = x
    half_turn = np.diag([1.0, -1.0, -1.0])
    assert not tw.gibbs(np.stack([np.eye(3), np.eye(3)]), np.array([0]), np.array([1]), half_turn[None])[1][0]
    w, rho = tw.huber(np.array([0.5, 1.0, 4.0]), 1.0)
    assert np.allclose(w, [1.0, 1.0, 0.25]) and np.allclose(rho, [0.125, 0.5, 3.5])
    inc, root, size = tw.component(7, [[5, 6], [1, 2], [3, 4], [2, 3], [0, 6]], [1, 1, 1, 0, 1])
    assert (root, size) == (0, 3) and inc.tolist() == [1, 0, 0, 0, 0, 1, 1]      # 3 views twice: the smallest label wins
    assert tw.component(3, [[0, 1]], [0])[2] == 0


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_gposes_\w+|sfmloc_global_poses)\s*\(", hdr))
    assert names == {"sfmloc_gposes_default_options", "sfmloc_global_poses", "sfmloc_gposes_views", "sfmloc_gposes_pairs",
                     "sfmloc_gposes_report_read", "sfmloc_gposes_destroy", "sfmloc_gposes_last_ms"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    assert L.sfmloc_abi_version() == 2
    o = capi.gposes_default_options()
    assert [getattr(o, k) for k in tw.OPTIONS] == list(tw.OPTIONS.values())
    pair = _abi.struct("sfmloc_gposes_pair")
    assert capi.GPOSES_PAIR.itemsize == C.sizeof(pair) == 32
    assert [capi.GPOSES_PAIR.fields[f][1] for f, _ in pair._fields_] == [getattr(pair, f).offset for f, _ in pair._fields_]
    assert set(globalposes.REPORT_FIELDS) == {f for f, _ in capi.GposesReport._fields_}


def test_refusals_need_no_device():
    """every check of sfmloc_global_poses happens before anything is launched: the refusals come back without a GPU"""
    s = sc.scene_triplet()
    for change, text in (
            (dict(pairs=[[0, 1], [1, 3], [2, 0]]), "pair 1 = (1, 3) out of range"),
            (dict(pairs=[[0, 1], [2, 2], [2, 0]]), "pair 1 names view 2 twice"),
            (dict(pairs=[[0, 1], [1, 2], [1, 0]]), "pair 2 lists the views (0, 1) of pair 0 again"),
            (dict(rel_t=np.array([[0, 1, 0], [0, np.nan, 0], [1, 0, 0]], float)), "pair 1 = (1, 2) has a non-finite entry"),
            (dict(rel_R=s["rel_R"] * np.array([1, 1.0001, 1])[:, None, None]), "pair 1 = (1, 2): rel_R is not orthonormal"),
            (dict(rel_t=s["rel_t"] * np.array([1, 1, 0.999])[:, None]), "pair 2 = (2, 0): rel_t is not of unit length")):
        a = {**{k: s[k] for k in ("pairs", "rel_R", "rel_t")}, **change}
        with pytest.raises(capi.SfmlocError) as ei:
            capi.GlobalPoses(3, a["pairs"], a["rel_R"], a["rel_t"])
        assert ei.value.code == capi.EINVAL and text in ei.value.message, ei.value.message
    with pytest.raises(ValueError):
        capi.GlobalPoses(3, s["pairs"], s["rel_R"][:2], s["rel_t"])


def test_host_side_under_the_host_sanitizers(tmp_path):
    """tests/cpp/globalposes_host.cpp: a stand-alone host program, CPU only.  Where a HIP device is visible the program
    is built without the sanitizers (they are for CPU machines); it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/globalposes_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "globalposes_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "globalposes_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_adjacency_of_the_restatement_is_the_hosts():
    """the worked case of tests/cpp/globalposes_host.cpp"""
    off, nbr, pe = tw.adjacency(5, [[3, 1], [0, 1], [1, 2], [4, 0]])
    D = 0x80000000
    assert off.tolist() == [0, 2, 5, 6, 7, 8] and nbr.tolist() == [1, 4, 0, 2, 3, 1, 1, 0]
    assert pe.tolist() == [1, 3 | D, 1 | D, 2, 0 | D, 2 | D, 0, 3]


def test_tool_argument_parsing(capsys):
    kw = globalposes.parse_args(["-i", "a.json", "-p", "p.json", "-o", "o.json"])
    assert kw == dict(in_path="a.json", poses_path="p.json", out_path="o.json", triplet_angle=5.0, report_path=None, device=0)
    kw = globalposes.parse_args(["--input_file", "a", "--poses_file", "p", "--output_file", "o", "--triplet-angle", "3.5",
                                 "--device=1", "-r", "rep.json"])
    assert (kw["triplet_angle"], kw["device"], kw["report_path"]) == (3.5, 1, "rep.json")
    assert globalposes.parse_args(["--triplet-angle=2", "-i", "a", "-p", "p", "-o", "o"])["triplet_angle"] == 2.0
    for bad in (["-i", "a", "-p", "p"], ["-i", "a", "-p", "p", "-o"], ["-i", "a", "-p", "p", "-o", "o", "-x", "1"],
                ["-i", "a", "-p", "p", "-o", "o", "--triplet-angle", "zero"],
                ["-i", "a", "-p", "p", "-o", "o", "--triplet-angle", "0"], ["-i", "a", "-p", "p", "-o", "o", "--device=x"]):
        assert globalposes.parse_args(bad) is None
    assert globalposes.main(["-i", "a"]) == 1
    assert capsys.readouterr().err == globalposes.USAGE


def test_tool_maps_ids_to_indices_and_back(tmp_path, capsys):
    view_id = np.array([2, 3, 5, 8], np.uint32)
    entries = [{"I": 5, "J": 2, "R": np.eye(3).tolist(), "t": [0.0, 0.0, 1.0], "front": [3, 40, 0, 0], "choice": 1,
                "n_inliers": 40},
               {"I": 3, "J": 8, "R": [[0, -1, 0], [1, 0, 0], [0, 0, 1]], "t": [1.0, 0.0, 0.0], "front": [39, 0, 0, 0],
                "choice": 0, "n_inliers": 40}]
    pairs, rel_R, rel_t, use_t = globalposes.pose_arrays(entries, view_id)
    assert pairs.tolist() == [[2, 0], [1, 3]] and use_t.tolist() == [1, 0]      # front[choice] == n_inliers
    assert rel_R[1].tolist() == entries[1]["R"] and rel_t[0].tolist() == [0.0, 0.0, 1.0]
    with pytest.raises(KeyError):
        globalposes.pose_arrays([dict(entries[0], J=4)], view_id)
    assert globalposes.pose_arrays([], view_id)[0].shape == (0, 2)
    R = np.stack([np.eye(3) * (k + 1) for k in range(4)])
    Cc = np.arange(12.0).reshape(4, 3)
    ext = globalposes.extrinsics([7, 4, 9, 4], np.array([1, 1, 0, 1], bool), R, Cc)
    assert [e["key"] for e in ext] == [4, 7]                                     # by id_pose, ascending; view 2 is out
    assert ext[0]["value"] == {"rotation": (2 * np.eye(3)).tolist(), "center": [3.0, 4.0, 5.0]}   # the first view of pose 4
    assert ext[1]["value"]["center"] == [0.0, 1.0, 2.0]
    assert globalposes.run(str(tmp_path / "none.json"), "p", "o") == 1
    assert "cannot be read" in capsys.readouterr().err
