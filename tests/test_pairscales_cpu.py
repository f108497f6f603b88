"""CPU: the NumPy restatement of the wedge scales (tests/pairscales_np.py) against the planted baselines of
tests/pairscales_scene.py, its median and cap rules on hand-made lists, the header's new symbols and their bindings, the
refusals, which need no device, and the host side of the call under the host sanitizers."""
import ctypes as C
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

import pairscales_np as tw  # noqa: E402
import pairscales_scene as sc  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import _abi, capi  # noqa: E402


def log_errors(s, records):
    """|log(ratio / (b_l / b_k))| of every record against the planted baselines"""
    return np.array([abs(np.log(q * s["b_true"][k] / s["b_true"][l])) for _, k, l, _, q in records])


def test_restatement_recovers_the_planted_baseline_ratios():
    """The corridor with exact relative poses, 0.3 px of noise at f = 800 (0.0004 rad per bearing, 0.0005 rad on a
    parallax).  A point on a wall 2 units off the axis at depth z has parallax b 2 / (z^2 + 4): 0.05 rad at the typical
    z = 6, b = 1 (1 % per depth) and 0.005 rad at the worst z = 15, b = 0.6 (10 %).  The median of n >= 19 quotients has
    1.25 / sqrt(n) of a quotient's error and a quotient sqrt(2) of a depth's: 0.4 % typical, 4 % at the very worst."""
    s = sc.scene_corridor(wrong=False, rot_noise=0.0, dir_noise=0.0)
    r = tw.wedge_scales(**s["call"])
    rec = r["records"]
    assert len(rec) == r["n_candidates"] == 158 and min(x[3] for x in rec) >= 19
    err = log_errors(s, rec)
    print("log error of the ratios: median %.5f, largest %.5f" % (np.median(err), err.max()))
    assert np.median(err) <= 0.004 and err.max() <= 0.04
    assert rec == sorted(rec, key=lambda x: (x[1], x[2], x[0])) and all(k < l for _, k, l, _, _ in rec)
    pairs = s["pairs"].tolist()
    assert all(v in pairs[k] and v in pairs[l] for v, k, l, _, _ in rec)


def test_a_record_depends_on_its_two_pairs_alone():
    """the planted wrong direction moves the wedges of its pair and no other bit; leaving the pair out removes them"""
    clean, s = sc.scene_corridor(wrong=False), sc.scene_corridor()
    w = s["wrong_pair"]
    a, b = tw.wedge_scales(**clean["call"])["records"], tw.wedge_scales(**s["call"])["records"]
    assert [x for x in a if w not in x[1:3]] == [x for x in b if w not in x[1:3]]
    moved = [(x, y) for x, y in zip(a, b) if w in x[1:3]]
    assert len(a) == len(b) and len(moved) == 10 and all(x[4] != y[4] for x, y in moved)
    use = np.ones(len(s["pairs"]), np.uint8)
    use[w] = 0
    c = tw.wedge_scales(**s["call"], use_pair=use)
    assert c["records"] == [x for x in b if w not in x[1:3]] and c["n_candidates"] == len(c["records"])


def test_median_and_cap_rules_on_hand_made_lists():
    f = np.arange(10, 16)
    # the lower median: element (n - 1) // 2 of the sorted quotients
    assert tw.wedge_ratio(f, [4.0, 1.0, 3.0, 2.0, 6.0, 5.0], f, np.ones(6)) == (6, 3.0)
    assert tw.wedge_ratio(f[:5], [4.0, 1.0, 3.0, 2.0, 6.0], f[:5], np.ones(5)) == (5, 3.0)
    assert tw.wedge_ratio(f[:1], [7.0], f[:1], [2.0]) == (1, 3.5)
    # only the shared features count, wherever they stand in either list
    assert tw.wedge_ratio([1, 4, 6, 9], [1.0, 8.0, 3.0, 5.0], [0, 4, 5, 9, 11], [9.0, 2.0, 9.0, 10.0, 9.0]) == (2, 0.5)
    assert tw.wedge_ratio([1, 2], [1.0, 1.0], [3, 4], [1.0, 1.0]) == (0, 0.0)
    # the cap takes the first max_shared shared features in feature order, and n_shared still counts them all
    z = np.array([9.0, 8.0, 7.0, 1.0, 2.0, 3.0])
    assert tw.wedge_ratio(f, z, f, np.ones(6), max_shared=3) == (6, 8.0)
    assert tw.wedge_ratio(f, z, f, np.ones(6), max_shared=1) == (6, 9.0)
    # equal quotients: the order (value, feature) picks the same value either way
    assert tw.wedge_ratio(f[:4], [2.0, 2.0, 1.0, 3.0], f[:4], np.ones(4)) == (4, 2.0)
    # a feature named twice on one side keeps its first depth in the order of the inlier list
    assert [x.tolist() for x in tw.side_list([7, 3, 7, 5, 3], [1.0, 2.0, 3.0, 4.0, 5.0])] == [[3, 5, 7], [2.0, 4.0, 1.0]]
    assert [len(x) for x in tw.side_list([], [])] == [0, 0]
    # the candidates of a view: its used pairs ascending, every two of them
    ent = tw.view_pairs(5, [[3, 1], [0, 1], [1, 2], [4, 0]])
    assert ent == [[(1, 0), (3, 1)], [(0, 1), (1, 1), (2, 0)], [(2, 1)], [(0, 0)], [(3, 0)]]       # tests/cpp/pairscales_host.cpp
    assert tw.view_pairs(5, [[3, 1], [0, 1], [1, 2], [4, 0]], [1, 0, 1, 1])[1] == [(0, 1), (2, 0)]


def test_depths_are_the_planted_ones_on_exact_bearings():
    rng = np.random.default_rng(3)
    Rj, Cj = sc.gs.random_rotation(rng, 0.3), np.array([0.6, -0.3, 0.2])
    X = rng.uniform(-1.0, 1.0, (30, 3)) + np.array([0.0, 0.0, 5.0])
    b = float(np.linalg.norm(Cj))
    Xj = (X - Cj) @ Rj.T
    t = -(Rj @ Cj) / b                                       # X_J = R X_I + t in units of the baseline
    zi, zj, ok = tw.two_view_depths(Rj.reshape(9), t, X[:, :2] / X[:, 2:], Xj[:, :2] / Xj[:, 2:])
    assert ok.all() and np.allclose(zi * b, X[:, 2], rtol=1e-9) and np.allclose(zj * b, Xj[:, 2], rtol=1e-9)
    zi, zj, ok = tw.two_view_depths(Rj.reshape(9), -t, X[:, :2] / X[:, 2:], Xj[:, :2] / Xj[:, 2:])
    assert (zi < 0).all() and (zj < 0).all()                   # the reversed baseline: behind both cameras


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_wscales_\w+|sfmloc_wedge_scales)\s*\(", hdr))
    assert names == {"sfmloc_wscales_default_options", "sfmloc_wedge_scales", "sfmloc_wscales_count", "sfmloc_wscales_read",
                     "sfmloc_wscales_report_read", "sfmloc_wscales_destroy", "sfmloc_wscales_last_ms"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    assert L.sfmloc_abi_version() == 2
    o = capi.wscales_default_options()
    assert {k: getattr(o, k) for k in tw.OPTIONS} == tw.OPTIONS
    rec = _abi.struct("sfmloc_wscale")
    assert capi.WSCALE.itemsize == C.sizeof(rec) == 24
    assert [capi.WSCALE.fields[f][1] for f, _ in rec._fields_] == [getattr(rec, f).offset for f, _ in rec._fields_]
    with pytest.raises(AttributeError):
        capi.wscales_default_options(min_share=3)


def test_refusals_need_no_device():
    """every check of sfmloc_wedge_scales happens before anything is launched: the refusals come back without a GPU"""
    s = sc.scene_triplet()["call"]
    bad_R, bad_t = s["rel_R"].copy(), s["rel_t"].copy()
    bad_R[1, 2, 0], bad_t[2, 1] = np.nan, np.inf
    bad_inl = s["inl_idx"].copy()
    bad_inl[45] = 40
    bad_mi = s["match_i"].copy()
    bad_mi[85] = 40
    for change, code, text in (
            (dict(pairs=[[0, 1], [1, 3], [2, 0]]), capi.EINVAL, "sfmloc_wedge_scales: pair 1 = (1, 3) out of range"),
            (dict(pairs=[[0, 1], [2, 2], [2, 0]]), capi.EINVAL, "sfmloc_wedge_scales: pair 1 names view 2 twice"),
            (dict(match_i=bad_mi), capi.EINVAL, "sfmloc_wedge_scales: pair (2, 0) match 5 out of range"),
            (dict(intrinsic_type=[0, 2]), capi.EINVAL, "sfmloc_wedge_scales: intrinsic 1 has type 2"),
            (dict(inl_idx=bad_inl), capi.EINVAL, "pair (1, 2) inlier 5 out of range"),
            (dict(inl_off=[0, 40, 30, 120]), capi.EINVAL, "inlier_off not monotone at pair 1"),
            (dict(rel_R=bad_R), capi.EINVAL, "pair (1, 2) has a non-finite rel_R or rel_t"),
            (dict(rel_t=bad_t), capi.EINVAL, "pair (2, 0) has a non-finite rel_R or rel_t"),
            (dict(min_shared=0), capi.EINVAL, "min_shared = 0"),
            (dict(max_shared=0), capi.EINVAL, "max_shared = 0"),
            (dict(max_shared=2049), capi.EINVAL, "max_shared = 2049")):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.WedgeScales(**{**s, **change})
        assert ei.value.code == code and text in ei.value.message, ei.value.message
    for change in (dict(rel_R=s["rel_R"][:2]), dict(inl_off=s["inl_off"][:3]), dict(use_pair=[1, 1]),
                   dict(view_intrinsic=[0, 1])):
        with pytest.raises(ValueError):
            capi.WedgeScales(**{**s, **change})


def test_host_side_under_the_host_sanitizers(tmp_path):
    """tests/cpp/pairscales_host.cpp: a stand-alone host program, CPU only.  Where a HIP device is visible the program
    is built without the sanitizers (they are for CPU machines); it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/pairscales_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "pairscales_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "pairscales_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_boundary_scene_crosses_what_it_is_there_to_cross():
    """scene (c) of tests/test_gpu_pairscales.py, without running the restatement on it"""
    s = sc.scene_boundaries()
    c = s["call"]
    deg = np.bincount(c["pairs"].ravel(), minlength=s["n_views"])
    assert len(c["pairs"]) > 256 and deg[s["hub"]] == 80 > 64 and np.delete(deg, s["hub"]).max() <= 64
    assert sum(d * (d - 1) // 2 for d in deg) > 4 * 256 and int(c["inl_off"][-1]) > 4 * 1024
    per_pair = np.diff(c["offsets"].astype(np.int64))
    assert (per_pair[s["big"]["pairs"]] == 2100).all() and per_pair[s["big"]["pairs"]].min() > tw.OPTIONS["max_shared"]
    k = s["repeat"]["pairs"][0]
    mi = c["match_i"][int(c["offsets"][k]):int(c["offsets"][k + 1])]
    assert sorted(np.nonzero(np.bincount(mi) == 2)[0].tolist()) == sorted(s["repeat"]["features"])


def test_pair_scales_json_round_trips_through_both_codecs(tmp_path):
    from sfmlocalization_amd import fileio
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/pair_scales_file.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "pair_scales_file")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe, os.path.join(ROOT, "tests", "cpp", "pair_scales_file.cpp")], check=True, timeout=300)
    rec = [(7, (3, 7), (7, 12), 40, 1.0 / 3.0), (4294967295, (0, 4294967295), (4294967295, 9), 8, 2.0090651911371125),
           (2, (2, 5), (1, 2), 2100, 1e-300), (5, (5, 6), (5, 9), 9, 123456789012345680000.0), (1, (1, 2), (1, 3), 8, 1.0)]
    a, b, c = (str(tmp_path / n) for n in ("a.json", "b.json", "c.json"))
    HEAD = '{"pair_scales_version": 1, "min_shared": 8, "max_shared": 9, "pair_scales": ['
    fileio.write_pair_scales(a, rec, 8, 2048)
    assert fileio.read_pair_scales(a) == (rec, 8, 2048)                      # the doubles read back as themselves
    r = subprocess.run([exe, a, b], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout == "OK 5 records, min_shared 8, max_shared 2048\n", r.stdout + r.stderr
    assert open(a, "rb").read() == open(b, "rb").read()                      # the same bytes from both writers
    fileio.write_pair_scales(a, [], 3, 16)
    assert subprocess.run([exe, a, b], capture_output=True, timeout=60).returncode == 0
    assert open(b).read() == '{"pair_scales_version": 1, "min_shared": 3, "max_shared": 16, "pair_scales": []}'
    with open(c, "w") as fh:
        fh.write(HEAD + '{"view": 1, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": 2}]}')
    assert fileio.read_pair_scales(c)[0] == [(1, (1, 2), (1, 3), 8, 2.0)]      # an integer is a number to both readers
    assert subprocess.run([exe, c, b], capture_output=True, timeout=60).returncode == 0
    for text in ('{"pair_scales_version": 2, "min_shared": 8, "max_shared": 9, "pair_scales": []}', '[]', '{"pair_scales": []}',
                 '{"pair_scales_version": 1, "min_shared": 8, "max_shared": 9, "pair_scales": [{"view": 1}]}',
                 '{"pair_scales_version": 1, "min_shared": 8, "pair_scales": []}',
                 # what one reader refuses the other refuses: ids and counts are JSON integers of 32 bits without a sign,
                 # a ratio is a JSON number, the version is the integer 1
                 *[HEAD + entry + "]}" for entry in (
                     '{"view": 3.7, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": 1.0}',
                     '{"view": "5", "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": 1.0}',
                     '{"view": -1, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": 1.0}',
                     '{"view": 4294967296, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": 1.0}',
                     '{"view": 1, "k": [1, 2, 3], "l": [1, 3], "n_shared": 8, "ratio": 1.0}',
                     '{"view": 1, "k": [1, 2], "l": [1, true], "n_shared": 8, "ratio": 1.0}',
                     '{"view": 1, "k": [1, 2], "l": [1, 3], "n_shared": 8.0, "ratio": 1.0}',
                     '{"view": 1, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": "1.0"}',
                     '{"view": 1, "k": [1, 2], "l": [1, 3], "n_shared": 8, "ratio": null}',
                     '{"view": 1, "k": [1, 2], "l": [1, 3], "n_shared": 8}', '7')],
                 '{"pair_scales_version": 1.0, "min_shared": 8, "max_shared": 9, "pair_scales": []}',
                 '{"pair_scales_version": 1, "min_shared": -8, "max_shared": 9, "pair_scales": []}',
                 '{"pair_scales_version": 1, "min_shared": 8, "max_shared": 9, "pair_scales": {}}'):
        with open(c, "w") as fh:
            fh.write(text)
        with pytest.raises(ValueError) as ei:
            fileio.read_pair_scales(c)
        assert c in str(ei.value), text
        r = subprocess.run([exe, c, b], capture_output=True, text=True, timeout=60)
        assert r.returncode == 1 and r.stdout.startswith("refused: "), r.stdout + r.stderr


def test_relpose_tool_scales_switch_and_id_mapping():
    from sfmlocalization_amd import relpose
    base = ["-i", "a.json", "-m", "dir"]
    assert "scales_file" not in relpose.parse_args(base)                     # without the switch the tool is what it was
    assert relpose.parse_args(base + ["-s", "pair_scales.json"])["scales_file"] == "pair_scales.json"
    assert relpose.parse_args(base + ["--scales_file", "x.json", "-n", "8"])["scales_file"] == "x.json"
    assert relpose.parse_args(base + ["-s"]) is None
    assert "[-s|--scales_file]" in relpose.USAGE
    res = np.zeros(4, capi.RELPOSE_RESULT)
    res["ok"], res["n_inliers"], res["choice"] = [1, 1, 0, 1], [30, 30, 30, 12], [2, 0, 1, 3]
    res["front"] = [[0, 0, 30, 0], [29, 0, 0, 0], [0, 30, 0, 0], [0, 0, 0, 12]]
    assert relpose.scale_pairs(res).tolist() == [1, 0, 0, 1]                 # ok, and every inlier in front
    records = np.zeros(2, capi.WSCALE)
    records[0], records[1] = (1, 0, 2, 40, 0.5), (3, 1, 2, 9, 2.25)
    out = relpose.scale_entries(np.array([4, 9, 11, 20]), [(0, 1), (3, 2), (1, 3)], records)
    assert out == [(9, (4, 9), (9, 20), 40, 0.5), (20, (20, 11), (9, 20), 9, 2.25)]


# ---- sfmloc_global_poses_scaled ------------------------------------------------------------------------------------------

def test_scaled_restatement_keeps_the_corridors_spacing():
    """Scene (b) at the committed seed, both solvers: the baselines against the planted ones (in the unit of their lower
    median), the centres against the planted ones, and the three bounds of the device test that carries the feature.
    The figures are those of tests/golden/pairscales_parity.json."""
    import json
    import globalposes_np as gp
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_pairscales_fixtures import wedges_of
    with open(os.path.join(HERE, "golden", "pairscales_parity.json")) as fh:
        gold = json.load(fh)["corridor"]
    s = sc.scene_corridor()
    kl, ratio = wedges_of(tw.wedge_scales(**s["call"]))
    u = gp.global_poses(14, s["pairs"], s["rel_R"], s["rel_t"])
    e_plain = sc.gs.errors(s, u["in_component"], u["root"], u["R"], u["C"])[1]
    bt = s["b_true"] / tw.lower_median(s["b_true"])
    for solver in ("pcg", "dense"):
        g = tw.global_poses_scaled(14, s["pairs"], s["rel_R"], s["rel_t"], kl, ratio, solver=solver)
        assert g["in_component"].all() and g["used_t"].all() and (g["root"], g["scale_first_pair"]) == (0, 0)
        e_scaled = sc.gs.errors(s, g["in_component"], u["root"], g["R"], g["C"])[1]
        rel = np.abs(g["baselines"] / bt - 1.0)
        print(solver, "centre error scaled", e_scaled, "unscaled", e_plain, "baselines: wrong pair", rel[s["wrong_pair"]],
              "others", np.delete(rel, s["wrong_pair"]).max())
        assert e_scaled <= 0.03 and e_scaled <= e_plain / 3.0 and e_plain > 0.05
        assert abs(e_scaled - gold["centre_error_scaled"]) < 1e-8 and abs(e_plain - gold["centre_error_unscaled"]) < 1e-8
        # the wrong pair's baseline is off and its wedges are weighed down; the others lie within 15 %: their ratios are
        # good to 4 % (above), but the wrong pair's ten wedges pull at their neighbours with weight delta / |r| each
        assert rel[s["wrong_pair"]] > 0.5 and np.delete(rel, s["wrong_pair"]).max() < 0.15
        mine = (kl == s["wrong_pair"]).any(1)
        down = g["wedge_weights"] < 1.0                    # weighed down: wedges of the wrong pair, and only such
        assert mine.sum() == 10 and down.sum() >= 2 and (mine[down]).all() and (g["wedge_weights"] > 0.0).all()
        assert lower_median_is_one(g["baselines"])
        assert (g["scale_stop"], g["trans_stop"]) == (0, 0) and g["scale_steps_accepted"] == gold["scale_steps_accepted"]
    # without the wrong direction and without noise on the poses the spacing is the planted one to the ratios' accuracy
    c = sc.scene_corridor(wrong=False, rot_noise=0.0, dir_noise=0.0)
    kl, ratio = wedges_of(tw.wedge_scales(**c["call"]))
    g = tw.global_poses_scaled(14, c["pairs"], c["rel_R"], c["rel_t"], kl, ratio)
    rel = np.abs(g["baselines"] / (c["b_true"] / tw.lower_median(c["b_true"])) - 1.0)
    e = sc.gs.errors(c, g["in_component"], g["root"], np.where(g["in_component"][:, None, None], g["R"], 0.0), g["C"])[1]
    print("clean corridor: baselines", rel.max(), "centres", e)
    assert rel.max() < 0.04 and e < 0.01


def lower_median_is_one(b):
    return tw.lower_median(b[b > 0]) == 1.0


def test_scaled_restatement_rules_on_hand_made_graphs():
    """four views in a square with both diagonals (every pair in two passing triplets); hand-made wedges"""
    Ct = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0], [2.0, 1.0, 0.0], [0.0, 1.0, 0.5]])
    plist = [(0, 1), (1, 2), (2, 3), (3, 0), (0, 2), (1, 3)]
    rel_R = np.stack([np.eye(3)] * 6)
    rel_t = np.array([-(Ct[b] - Ct[a]) / np.linalg.norm(Ct[b] - Ct[a]) for a, b in plist])
    bt = np.array([np.linalg.norm(Ct[b] - Ct[a]) for a, b in plist])
    allw = [(k, l) for k in range(6) for l in range(k + 1, 6) if set(plist[k]) & set(plist[l])]
    ratio = np.array([bt[l] / bt[k] for k, l in allw])
    g = tw.global_poses_scaled(4, plist, rel_R, rel_t, allw, ratio)
    assert np.allclose(g["baselines"], bt / tw.lower_median(bt), rtol=1e-12) and (g["wedge_weights"] == 1.0).all()
    assert np.allclose(tw.gp.align_similarity(g["C"], Ct), Ct, atol=1e-9)
    # two components of the scale graph: the larger wins, the smaller pair index on a tie; pairs outside drop out
    g = tw.global_poses_scaled(4, plist, rel_R, rel_t, [(0, 1), (2, 3), (3, 5)], [bt[1] / bt[0], bt[3] / bt[2], bt[5] / bt[3]])
    assert g["used_t"].tolist() == [0, 0, 1, 1, 0, 1] and (g["scale_first_pair"], g["scale_n_scaled_pairs"]) == (2, 3)
    assert g["in_component"].all() and g["root"] == 0
    g = tw.global_poses_scaled(4, plist, rel_R, rel_t, [(0, 1), (2, 3)], [bt[1] / bt[0], bt[3] / bt[2]])
    assert g["used_t"].tolist() == [1, 1, 0, 0, 0, 0] and g["in_component"].tolist() == [1, 1, 1, 0] and not g["R"][3].any()
    # a ratio that is not a finite positive number is no edge; use_t = 0 takes a pair's wedges with it
    g = tw.global_poses_scaled(4, plist, rel_R, rel_t, [(0, 1), (2, 3), (3, 5)], [np.nan, bt[3] / bt[2], -1.0])
    assert g["used_t"].tolist() == [0, 0, 1, 1, 0, 0] and g["scale_n_wedges_used"] == 1
    g = tw.global_poses_scaled(4, plist, rel_R, rel_t, [(0, 1), (2, 3), (3, 5)], [1.0, 1.0, 1.0], use_t=[1, 1, 1, 0, 1, 1])
    assert g["used_t"].tolist() == [1, 1, 0, 0, 0, 0]
    for wedges in (([], []), ([(0, 1)], [0.0])):
        g = tw.global_poses_scaled(4, plist, rel_R, rel_t, *wedges)
        assert not g["in_component"].any() and not g["used_t"].any() and g["n_component_views"] == 0 and g["kept"].all()


def test_scaled_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_gpscale_\w+|sfmloc_global_poses_scaled)\s*\(", hdr))
    assert names == {"sfmloc_gpscale_default_options", "sfmloc_global_poses_scaled", "sfmloc_gpscale_baselines",
                     "sfmloc_gpscale_weights", "sfmloc_gpscale_report_read"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    o = capi.gpscale_default_options()
    assert {k: getattr(o, k) for k in tw.SCALE_OPTIONS} == tw.SCALE_OPTIONS
    from sfmlocalization_amd import globalposes
    assert set(globalposes.SCALE_REPORT_FIELDS) == {f for f, _ in capi.GpscaleReport._fields_}
    with pytest.raises(AttributeError):
        capi.gpscale_default_options(delta=3)


def test_scaled_refusals_need_no_device():
    s = sc.scene_triplet()

    def refused(kl, ratio, text, **kw):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.GlobalPoses(3, s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl, ratio), **kw)
        assert ei.value.code == capi.EINVAL and text in ei.value.message, ei.value.message
    refused([[0, 3]], [1.0], "sfmloc_global_poses_scaled: wedge 0 = pairs (0, 3) out of range")
    refused([[0, 1], [2, 1]], [1.0, 1.0], "wedge 1 = pairs (2, 1): k must be below l")
    refused([[1, 1]], [1.0], "k must be below l")
    refused([[0, 1], [0, 2], [0, 1]], [1.0, 1.0, 1.0], "the wedge of pairs (0, 1) is listed twice")
    refused([[0, 1]], [1.0], "scale_delta or a tolerance is out of range", scale=dict(scale_delta=-1.0))
    refused([[0, 1]], [1.0], "max_pcg = 0", scale=dict(max_pcg=0))
    four = dict(pairs=[[0, 1], [2, 3]], rel_R=np.stack([np.eye(3)] * 2), rel_t=[[1.0, 0, 0], [0, 1.0, 0]])
    with pytest.raises(capi.SfmlocError) as ei:
        capi.GlobalPoses(4, four["pairs"], four["rel_R"], four["rel_t"], wedges=([[0, 1]], [1.0]))
    assert "wedge 0 = pairs (0, 1) share no view" in ei.value.message
    with pytest.raises(capi.SfmlocError) as ei:                                # the unscaled call's checks come first
        capi.GlobalPoses(2, four["pairs"], four["rel_R"], four["rel_t"], wedges=([[0, 1]], [1.0]))
    assert "sfmloc_global_poses: pair 1 = (2, 3) out of range" in ei.value.message
    with pytest.raises(ValueError):
        capi.GlobalPoses(3, s["pairs"], s["rel_R"], s["rel_t"], wedges=([[0, 1]], [1.0, 2.0]))
    with pytest.raises(ValueError):
        capi.GlobalPoses(3, s["pairs"], s["rel_R"], s["rel_t"], scale=dict(scale_delta=0.2))


def test_globalposes_and_globalsfm_scales_switches_and_id_mapping():
    from sfmlocalization_amd import globalposes, globalsfm
    base = ["-i", "a.json", "-p", "p.json", "-o", "o.json"]
    assert "scales_path" not in globalposes.parse_args(base)                 # without the switch the tool is what it was
    assert globalposes.parse_args(base + ["-s", "ps.json"])["scales_path"] == "ps.json"
    assert globalposes.parse_args(base + ["--scales_file", "x.json", "-r", "r.json"])["scales_path"] == "x.json"
    assert globalposes.parse_args(base + ["-s"]) is None
    assert "[-s|--scales_file]" in globalposes.USAGE
    base = ["-i", "a.json", "-m", "dir", "-o", "out"]
    assert "pair_scales" not in globalsfm.parse_args(base)
    assert globalsfm.parse_args(base + ["--pair-scales"])["pair_scales"] is True
    assert globalsfm.parse_args(["--pair-scales"] + base + ["--device=1"]) == dict(
        in_path="a.json", match_dir="dir", out_dir="out", triplet_angle=5.0, device=1, pair_scales=True)
    assert globalsfm.parse_args(base + ["--pair-scales", "1"]) is None and "[--pair-scales]" in globalsfm.USAGE
    # a record names its pairs by view ids in the pair list's order; they are looked up in the poses file's entries
    entries = [{"I": 9, "J": 4}, {"I": 4, "J": 20}, {"I": 20, "J": 11}]
    kl, ratio = globalposes.wedge_arrays([(4, (9, 4), (4, 20), 40, 0.5), (20, (4, 20), (20, 11), 9, 2.25)], entries)
    assert kl.tolist() == [[0, 1], [1, 2]] and kl.dtype == np.uint32 and ratio.tolist() == [0.5, 2.25]
    with pytest.raises(KeyError):
        globalposes.wedge_arrays([(4, (4, 9), (4, 20), 40, 0.5)], entries)    # (4, 9) is not (9, 4)
    assert globalposes.wedge_arrays([], entries)[0].shape == (0, 2)
