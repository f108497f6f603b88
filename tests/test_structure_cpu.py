"""CPU: the NumPy restatement of sfmloc_tracks and sfmloc_sfm_triangulate (tests/structure_np.py) on the planted scene
(tests/structure_scene.py) -- its tracks against a plain union-find, its fixed-sweep eigen-solve against
numpy.linalg.svd on every A of the scene, its points against the scene's ground truth -- plus what needs no device: the
declared symbols, the host side of sfmloc_tracks_build under the host sanitizers, and the tool's refusals.

The two numeric bounds are one figure: what the SVD triangulation itself leaves on this scene (the N-view null vector
by numpy.linalg.svd over all posed observations of every plain track, against the ground truth: the pixel noise's share),
times 4 for the different operation order, as test_gpu_adjust_ba.py takes its margin.  profiles/structure_parity.json
records it (python tests/test_structure_cpu.py writes the file)."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

import sfmlocalization_amd as S
from sfmlocalization_amd import _abi, capi, structure

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import structure_np as tw  # noqa: E402
import structure_scene as sc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARITY = os.path.join(ROOT, "profiles", "structure_parity.json")
MARGIN = 4.0

_cache = {}


def scene():
    if not _cache:
        s = sc.make_scene()
        pairs, off, mi, mj = sc.pair_list(s)
        trk = tw.tracks(s["view_off"], pairs, off, mi, mj)
        a, pts, extra = sc.scene_arrays(s, trk)
        A = s["arrays"]
        _cache.update(s=s, pair_list=(pairs, off, mi, mj), trk=trk, a=a, pts=pts, extra=extra,
                      tri=tw.triangulate(a, A["pose_valid"], A["pose_R"], A["pose_C"]))
    return _cache


def union_find_tracks(view_off, pairs, offsets, mi, mj, view_use=None, min_length=2):
    """the plain statement: a dictionary union-find over (view, feature) -> sorted list of tracks [(view, feat), ...]"""
    parent = {}

    def find(x):
        while parent.setdefault(x, x) != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for k, (va, vb) in enumerate(pairs):
        if view_use is not None and not (view_use[va] and view_use[vb]):
            continue
        for t in range(int(offsets[k]), int(offsets[k + 1])):
            parent[find((int(va), int(mi[t])))] = find((int(vb), int(mj[t])))
    comps = {}
    for x in list(parent):
        comps.setdefault(find(x), []).append(x)
    out, conflict, short = [], 0, 0
    for c in comps.values():
        c.sort()
        if len({v for v, _ in c}) != len(c):
            conflict += 1
        elif len(c) < min_length:
            short += 1
        else:
            out.append(c)
    out.sort(key=lambda c: int(view_off[c[0][0]]) + c[0][1])        # ascending smallest row
    return out, [len(comps), conflict, short, len(out)]


@pytest.mark.parametrize("masked", [False, True])
def test_twin_tracks_equal_a_plain_union_find(masked):
    c = scene()
    s = c["s"]
    pairs, off, mi, mj = c["pair_list"]
    use = sc.view_use(s) if masked else None
    t = tw.tracks(s["view_off"], pairs, off, mi, mj, view_use=use)
    exp, counts = union_find_tracks(s["view_off"], pairs, off, mi, mj, view_use=use)
    assert t["counts"] == counts
    got = [[(int(t["view"][o]), int(t["feat"][o])) for o in range(int(t["off"][k]), int(t["off"][k + 1]))]
           for k in range(len(t["off"]) - 1)]
    assert got == exp
    assert len(mi) > 1024 and t["passes"] >= 3, "the scene must need several passes and span several workgroups"
    if not masked:
        lengths = set(np.diff(t["off"]).astype(int).tolist())
        assert {2, 3, 8} <= lengths and t["counts"][1] == 2        # the planted conflict and the nine-pair chain
        ea, eb = tw.edges(s["view_off"], pairs, off, mi, mj)
        assert int(s["view_off"][-1]) - len(set(ea.tolist()) | set(eb.tolist())) == 24      # three singletons per view


def measure():
    """-> dict of the figures profiles/structure_parity.json records"""
    c = scene()
    s, a, pts, tri = c["s"], c["a"], c["pts"], c["tri"]
    A = s["arrays"]
    off = a["obs_off"].astype(np.int64)
    ra, rb = tw.rows(a, tw.projections(a, A["pose_R"], A["pose_C"]), tw.undistorted(a))
    posed = A["pose_valid"].astype(bool)[a["view_pose"][a["obs_view"].astype(np.int64)].astype(np.int64)]

    def stacked(idx):
        return np.concatenate([np.stack([ra[o], rb[o]]) for o in idx])
    svd_err = 0.0
    for l in np.nonzero(pts >= sc.FIRST_PLAIN)[0]:
        idx = np.arange(off[l], off[l + 1])[posed[off[l]:off[l + 1]]]
        svd_err = max(svd_err, float(np.abs(sc.svd_point(stacked(idx)) - s["X"][pts[l]]).max()))
    # the twin's points: every plain track, the tracks with planted outliers, the 33-observation and NaN-pixel landmarks
    truth = {l: s["X"][pts[l]] for l in np.nonzero((pts >= sc.FIRST_PLAIN) | (pts == 3) | (pts == 4))[0]}
    truth[int(np.nonzero(pts == -100)[0][0])] = c["extra"][0]
    truth[int(np.nonzero(pts == -101)[0][0])] = c["extra"][1]
    twin_err = max(float(np.abs(tri["X"][l] - x).max()) for l, x in truth.items())
    assert all(tri["landmark_keep"][l] for l in truth)
    # the twin's eigen-solve against the SVD of the same A: every two-view round, then every final N-view solve
    h = tri["hyp"]
    eig, n_a = 0.0, 0
    systems = [(stacked(o), x, ok) for o, x, ok in zip(h["obs"], h["X"], h["ok"])]
    for l in np.nonzero(tri["landmark_keep"])[0]:
        w = np.nonzero(h["landmark"] == l)[0][tri["winner"][l]]
        idx = np.arange(off[l], off[l + 1])[posed[off[l]:off[l + 1]]]
        inl, _ = tw.inliers(a, A["pose_R"], A["pose_C"], h["X"][w], idx, 4.0)
        systems.append((stacked(idx[inl[0]]), tri["X"][l], True))
    for M, x, ok in systems:
        if not np.isfinite(M).all():
            assert not ok                                    # (a NaN pixel: no hypothesis, nothing to compare)
            continue
        assert ok                                            # (the parallel rays too: a point some 6e7 away)
        n_a += 1
        eig = max(eig, float(np.abs(x - sc.svd_point(M)).max()))
    return {"svd_err_max": svd_err, "margin": MARGIN, "bound": MARGIN * svd_err, "twin_point_err_max": twin_err,
            "twin_vs_svd_max": eig, "systems_compared": n_a,
            "landmarks_checked": len(truth)}


def test_twin_eigen_solve_and_points_within_the_svd_triangulations_own_error():
    m = measure()
    with open(PARITY) as fh:
        rec = json.load(fh)
    print(json.dumps(m))
    assert rec["bound"] == pytest.approx(m["bound"], rel=1e-9), "profiles/structure_parity.json is out of date"
    assert m["systems_compared"] > 800
    assert m["twin_vs_svd_max"] <= m["bound"]
    assert m["twin_point_err_max"] <= m["bound"]


def test_twin_planted_cases():
    c = scene()
    s, a, pts, tri = c["s"], c["a"], c["pts"], c["tri"]
    off = a["obs_off"].astype(np.int64)

    def lm(p):
        return int(np.nonzero(pts == p)[0][0])

    def mask(p):
        return tri["obs_keep"][off[lm(p)]:off[lm(p) + 1]]

    def views(p):
        return a["obs_view"][off[lm(p)]:off[lm(p) + 1]]
    for p, outliers in ((3, [3]), (4, [1, 5])):
        assert tri["landmark_keep"][lm(p)]
        assert sorted(views(p)[~mask(p)].tolist()) == sorted(outliers + [sc.UNPOSED_VIEW])
    assert tri["landmark_keep"][lm(5)] and not mask(5)[views(5) == 0].any()      # behind camera 0: zero residual, no inlier
    assert mask(5)[(views(5) != 0) & (views(5) != sc.UNPOSED_VIEW)].all()
    assert tri["status"][lm(6)] != 0 and not tri["X"][lm(6)].any()               # parallel rays
    assert tri["landmark_keep"][lm(0)] and mask(0).all()                           # a pair is kept on two inliers
    assert tri["landmark_keep"][lm(2)] and mask(2).sum() == 7
    assert (~mask(-100)).sum() == 3 and len(mask(-100)) == 33
    assert tri["landmark_keep"][lm(-101)] and mask(-101).tolist() == [True, False, True, True]
    assert tri["status"][lm(-102)] == 1
    rep = tri["report"]
    assert rep["failed_posed"] == 1 and rep["landmarks_kept"] + rep["failed_posed"] + rep["failed_hypothesis"] + \
        rep["failed_inliers"] == rep["landmarks_in"] == len(pts)
    strict = tw.triangulate(a, s["arrays"]["pose_valid"], s["arrays"]["pose_R"], s["arrays"]["pose_C"], allow_pairs=False)
    assert strict["status"][lm(0)] == 3
    blind = tw.triangulate(a, s["arrays"]["pose_valid"], s["arrays"]["pose_R"], s["arrays"]["pose_C"], mode=tw.BLIND)
    assert blind["report"]["rounds"] == 0 and blind["landmark_keep"][lm(3)]
    assert blind["obs_keep"][off[lm(3)]:off[lm(3) + 1]].sum() == 7                # the depth test alone keeps the outlier


def test_new_symbols_are_declared():
    with open(os.path.join(ROOT, "include", "sfmloc.h")) as f:
        hdr = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    names = set(re.findall(r"\b(sfmloc_tracks_\w+|sfmloc_triangulate_\w+|sfmloc_sfm_triangulate)\s*\(", hdr))
    assert names == {"sfmloc_tracks_build", "sfmloc_tracks_counts", "sfmloc_tracks_read", "sfmloc_tracks_destroy",
                     "sfmloc_tracks_last_ms", "sfmloc_triangulate_default_options", "sfmloc_sfm_triangulate"}
    assert names <= set(capi.SYMBOLS)
    L = capi._L()
    for n in names:
        getattr(L, n)
    assert L.sfmloc_abi_version() == 2
    assert hasattr(capi, "Tracks") and hasattr(capi.Sfm, "triangulate")
    o = capi.triangulate_default_options()
    assert (o.mode, o.min_inliers, o.allow_pairs, o.residual_px) == (capi.TRI_ROBUST, 3, 1, 4.0)
    assert L.sfmloc_sfm_triangulate(None, None, None) == -1                  # SFMLOC_EINVAL, no device needed
    assert L.sfmloc_tracks_last_ms.restype is C.c_double and L.sfmloc_tracks_last_ms() >= 0.0
    # sizes and every field offset of sfmloc_triangulate_options / _report against the compiler: tests/test_abi.py
    assert capi.TriangulateOptions is _abi.struct("sfmloc_triangulate_options")
    assert capi.TriangulateReport is _abi.struct("sfmloc_triangulate_report")


def test_tracks_refusals_need_no_device():
    """every check of sfmloc_tracks_build happens before anything is launched: the refusals come back without a GPU"""
    for args, code, text in (
            (([0, 3, 6], [[0, 2]], [0, 1], [0], [0]), capi.EINVAL, "pair 0 = (0, 2) out of range"),
            (([0, 3, 6], [[0, 1]], [0, 2], [0, 1], [0, 3]), capi.EINVAL, "pair (0, 1) match 1 out of range"),
            (([0, 3, 2 ** 32 - 1], [[0, 1]], [0, 1], [0], [0]), capi.ECAP, "feature rows")):
        with pytest.raises(capi.SfmlocError) as ei:
            capi.Tracks(*args)
        assert ei.value.code == code and text in ei.value.message


def test_host_side_of_tracks_under_the_host_sanitizers(tmp_path):
    """tests/cpp/tracks_host.cpp: a stand-alone host program, CPU only.  Where a HIP device is visible the program is
    built without the sanitizers (they are for CPU machines); it checks the same things."""
    cxx = shutil.which("g++") or shutil.which("c++")
    if cxx is None:
        pytest.fail("no host C++ compiler (g++ / c++) to build tests/cpp/tracks_host.cpp")
    san = [] if S.device_count() > 0 else ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    exe = str(tmp_path / "tracks_host")
    subprocess.run([cxx, "-O1", "-g", "-std=c++17", "-Wall", *san, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "tracks_host.cpp")], check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.startswith("OK")


def test_tool_refuses_what_it_cannot_read(tmp_path, capsys):
    s = scene()["s"]
    path = sc.write_files(s, str(tmp_path))
    out = str(tmp_path / "out.json")
    assert [np.array_equal(S.fileio.read_feat(os.path.join(str(tmp_path), stem + ".feat")), f)
            for stem, f in zip(structure.view_files(s["doc"]), s["feats"])] == [True] * 8
    assert structure.main(["-i", path, "-m", str(tmp_path), "-f", "nothing.txt", "-o", out]) == 1
    assert "Invalid matches file." in capsys.readouterr().err and not os.path.exists(out)
    assert structure.main(["-i", str(tmp_path / "none.json"), "-m", str(tmp_path), "-o", out]) == 1
    assert "cannot be read" in capsys.readouterr().err
    os.remove(os.path.join(str(tmp_path), "frame0003.feat"))
    assert structure.main(["-i", path, "-m", str(tmp_path), "-o", out]) == 1
    assert "Invalid features." in capsys.readouterr().err and not os.path.exists(out)
    assert structure.main(["-i", path, "-m", str(tmp_path)]) == 1
    assert structure.NAME in capsys.readouterr().err


if __name__ == "__main__":
    rec = measure()
    rec["what"] = ("bounds of tests/test_structure_cpu.py on the scene of tests/structure_scene.py: svd_err_max = the "
                   "largest coordinate error of the N-view SVD triangulation of the plain tracks against the ground truth; "
                   "bound = margin x svd_err_max; the twin's figures beside it")
    with open(PARITY, "w") as fh:
        json.dump(rec, fh, indent=1)
        fh.write("\n")
    print(json.dumps(rec, indent=1))
