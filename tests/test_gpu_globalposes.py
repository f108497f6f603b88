"""Global poses on the device (sfmloc_global_poses, python -m sfmlocalization_amd.globalposes) against the NumPy
restatement (tests/globalposes_np.py) on the planted scenes of tests/globalposes_scene.py: (a) three views, (b) the
12-view ring with its planted faults, (c) 1 101 views, more than one workgroup and one view above the wave-per-view
threshold (its restatement is read from tests/golden/globalposes/scene_large.npz: it takes NumPy half a minute).

Integers are compared exactly.  Doubles are compared per quantity within four times what the restatement's two solvers
(its own PCG, numpy.linalg.solve) leave between them -- four times because the kernels order their sums differently
from both, the margin and the reasoning of test_gpu_adjust_joint.  Each scene is held to its own figures, the
"twin_<scene>" section of profiles/globalposes_parity.json, written by tests/golden/make_globalposes_fixtures.py (which
says how each was measured and why the bound has a floor of 16 eps), never taken from the device.  The planted accuracy is asked of the device itself: at most the
restatement's own error (tests/golden/globalposes/expected.json) plus the parity bound."""
import json
import os
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
from make_globalposes_fixtures import COSTS, bound as bound_of, distances  # noqa: E402
from sfmlocalization_amd import capi, globalposes, globalsfm  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "globalposes")
PARITY = os.path.join(ROOT, "profiles", "globalposes_parity.json")
SCENES = {"triplet": sc.scene_triplet, "ring": sc.scene_ring, "large": sc.scene_large}


def call(s, **kw):
    return capi.GlobalPoses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"], **kw)


def as_dict(g):
    """a device result with the restatement's keys"""
    out = {"in_component": g.in_component, "root": int(g.report.root), "R": g.R, "C": g.C}
    out.update({k: g.pairs[k] for k in ("n_triplets", "n_triplets_ok", "kept", "used_t", "rot_residual", "trans_residual")})
    out.update({k: getattr(g.report, k) for k in COSTS})
    return out


@pytest.fixture(scope="module")
def expected():
    with open(os.path.join(GOLDEN, "expected.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def bound():
    """scene -> quantity -> the device's bound there"""
    with open(PARITY) as fh:
        doc = json.load(fh)
    return {name: bound_of(doc["twin_" + name]) for name in SCENES}


@pytest.fixture(scope="module")
def ref():
    """per scene: the scene, the restatement's result and the device's; computed once, left unchanged"""
    out = {}
    for name, make in SCENES.items():
        s = make()
        if name == "large":
            with np.load(os.path.join(GOLDEN, "scene_large.npz")) as z:
                twin = {k: (z[k].item() if z[k].ndim == 0 else z[k]) for k in z.files}
        else:
            twin = tw.global_poses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"])
        out[name] = {"s": s, "twin": twin, "got": call(s)}
    return out


def record(section, values):
    """profiles/globalposes_parity.json keeps the last measured distances (best effort: a read-only tree is fine)"""
    try:
        with open(PARITY) as fh:
            doc = json.load(fh)
        doc[section] = values
        with open(PARITY, "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
    except (OSError, ValueError):
        pass


@pytest.mark.parametrize("name", list(SCENES))
def test_integers_equal_the_restatement(ref, expected, name):
    twin, g = ref[name]["twin"], ref[name]["got"]
    for f in ("n_triplets", "n_triplets_ok", "kept", "used_t"):
        assert np.array_equal(g.pairs[f].astype(np.int64), np.asarray(twin[f]).astype(np.int64)), f
    assert np.array_equal(g.in_component, np.asarray(twin["in_component"]).astype(bool))
    e, rep = expected[name], g.report
    assert (rep.root, rep.n_component_views, rep.n_pairs_kept, rep.n_triplets, rep.n_triplets_ok) == \
        (e["root"], e["n_component_views"], e["n_pairs_kept"], e["n_triplets"], e["n_triplets_ok"])
    assert (rep.n_views, rep.n_pairs) == (ref[name]["s"]["n_views"], len(ref[name]["s"]["pairs"]))
    pairs = ref[name]["s"]["pairs"].astype(np.int64)
    assert rep.n_rotation_pairs == int(np.sum(g.pairs["kept"].astype(bool) & g.in_component[pairs[:, 0]] &
                                              g.in_component[pairs[:, 1]]))
    assert rep.n_translation_pairs == int(g.pairs["used_t"].sum())
    assert rep.launches > 0 and rep.device_ms > 0.0
    assert rep.chordal_stop == 0 and rep.rot_stop in (0, 2) and rep.trans_stop == 0
    out = ~g.in_component
    assert not g.R[out].any() and not g.C[out].any()
    assert np.array_equal(g.R[rep.root], np.eye(3)) and not g.C[rep.root].any()


def test_planted_faults_of_the_ring(ref):
    s, g = ref["ring"]["s"], ref["ring"]["got"]
    assert not g.pairs["kept"][s["wrong"]].any() and not g.pairs["n_triplets_ok"][s["wrong"]].any()
    assert g.pairs["n_triplets"][s["wrong"]].all()
    assert not g.in_component[s["pendant"]] and not g.in_component[s["other_component"]].any()
    assert g.in_component[:12].all() and g.report.n_component_views == 12
    k = s["rotation_only"]                                   # feeds the rotations only
    assert g.pairs["kept"][k] and not g.pairs["used_t"][k]
    assert g.pairs["rot_residual"][k] > 0.0 and g.pairs["trans_residual"][k] == 0.0
    other = [k for k, p in enumerate(s["pairs"].tolist()) if p[0] in s["other_component"]]
    assert g.pairs["kept"][other].all() and not g.pairs["used_t"][other].any()      # kept, and not the component chosen
    assert g.report.n_rotation_pairs == 33 and g.report.n_translation_pairs == 32


@pytest.mark.parametrize("name", list(SCENES))
def test_doubles_within_the_two_solvers_distance(ref, bound, name):
    s, twin, g = ref[name]["s"], ref[name]["twin"], ref[name]["got"]
    d = distances(s, as_dict(g), twin)
    print(name, "device - restatement", d, "bound", bound[name], "steps", g.report.rot_steps_tried,
          g.report.trans_steps_tried, "pcg", g.report.chordal_pcg, g.report.rot_pcg_total, g.report.trans_pcg_total,
          "launches", g.report.launches, "ms", g.report.device_ms)
    record("device_" + name, d)
    for q in bound[name]:
        assert d[q] <= bound[name][q], (q, d[q], bound[name][q])
    assert g.report.rot_cost_final <= g.report.rot_cost_initial
    assert g.report.trans_cost_final < g.report.trans_cost_initial


@pytest.mark.parametrize("name", list(SCENES))
def test_planted_accuracy_on_the_device(ref, expected, bound, name):
    s, g = ref[name]["s"], ref[name]["got"]
    rot, cen = sc.errors(s, g.in_component, int(g.report.root), g.R, g.C)
    print(name, "rotation", rot, "deg, centre", cen, "of the extent; the restatement's:", expected[name]["rotation_deg"],
          expected[name]["centre"])
    # (an entry of R off by e turns it by at most about 3 e radians)
    assert rot <= expected[name]["rotation_deg"] + np.degrees(3.0 * bound[name]["R"])
    assert cen <= expected[name]["centre"] + bound[name]["C"]
    RtR = g.R[g.in_component].transpose(0, 2, 1) @ g.R[g.in_component]
    assert np.max(np.abs(RtR - np.eye(3))) <= 256 * np.finfo(np.float64).eps     # (relpose_scene.ROTATION_BOUND's count)


@pytest.mark.parametrize("name", list(SCENES))
def test_two_runs_and_a_reversed_pair_list_give_the_same_bits(ref, name):
    s, g = ref[name]["s"], ref[name]["got"]
    again = call(s)
    rev = capi.GlobalPoses(s["n_views"], s["pairs"][::-1], s["rel_R"][::-1], s["rel_t"][::-1], s["use_t"][::-1])
    for other, pairs in ((again, again.pairs), (rev, rev.pairs[::-1])):
        assert g.R.tobytes() == other.R.tobytes() and g.C.tobytes() == other.C.tobytes()
        assert np.array_equal(g.in_component, other.in_component)
        assert g.pairs.tobytes() == np.ascontiguousarray(pairs).tobytes()
        for f, _ in capi.GposesReport._fields_:
            if not f.endswith("_ms") and f != "launches":   # (times; the component search's passes depend on scheduling)
                assert getattr(g.report, f) == getattr(other.report, f), f


def test_no_triplet_passes_and_empty_calls(ref):
    s = ref["ring"]["s"]
    chain = [k for k, p in enumerate(s["pairs"].tolist()) if p[1] == p[0] + 1 and p[1] < 12]    # a path: no triangle
    g = capi.GlobalPoses(s["n_views"], s["pairs"][chain], s["rel_R"][chain], s["rel_t"][chain])
    assert not g.in_component.any() and not g.R.any() and not g.C.any()
    assert (g.report.n_component_views, g.report.n_pairs_kept, g.report.n_triplets) == (0, 0, 0)
    assert g.report.n_pairs == len(chain) and not g.pairs["kept"].any()
    g = capi.GlobalPoses(5, np.zeros((0, 2)), np.zeros((0, 3, 3)), np.zeros((0, 3)))
    assert not g.in_component.any() and len(g.pairs) == 0 and g.report.n_views == 5 and g.report.launches == 0
    t = ref["triplet"]["s"]                                   # every translation masked out: no component either
    g = capi.GlobalPoses(3, t["pairs"], t["rel_R"], t["rel_t"], np.zeros(3, np.uint8))
    assert g.pairs["kept"].all() and not g.in_component.any()


def test_refusals_come_before_any_launch(ref):
    s = ref["ring"]["s"]
    call(ref["triplet"]["s"])
    ms = capi.gposes_last_ms()
    assert ms > 0.0

    def refused(text, **change):
        a = {k: s[k].copy() for k in ("pairs", "rel_R", "rel_t")}
        for k, (at, v) in change.items():
            a[k][at] = v
        with pytest.raises(capi.SfmlocError) as ei:
            capi.GlobalPoses(s["n_views"], a["pairs"], a["rel_R"], a["rel_t"], s["use_t"])
        assert ei.value.code == capi.EINVAL and text in ei.value.message, ei.value.message
        assert capi.gposes_last_ms() == ms
    refused("pair 2 = (0, 16) out of range", pairs=(2, [0, 16]))
    refused("pair 3 names view 1 twice", pairs=(3, [1, 1]))
    refused("pair 5 lists the views (0, 1) of pair 0 again", pairs=(5, [1, 0]))
    refused("pair 7 = (2, 4) has a non-finite entry", rel_R=((7, 1, 2), np.nan))
    refused("pair 8 = (2, 5) has a non-finite entry", rel_t=((8, 0), np.inf))
    refused("pair 9 = (3, 4): rel_R is not orthonormal", rel_R=(9, 1.00001 * s["rel_R"][9]))
    refused("pair 9 = (3, 4): rel_t is not of unit length", rel_t=(9, 1.00001 * s["rel_t"][9]))
    with pytest.raises(capi.SfmlocError) as ei:
        call(s, triplet_angle_deg=0.0)
    assert ei.value.code == capi.EINVAL and capi.gposes_last_ms() == ms


def test_both_programs_write_the_same_bytes(ref, tmp_path):
    """python -m sfmlocalization_amd.globalposes and bin/ComputeGlobalPoses on the ring: view ids mapped to indices and
    back, the component's poses keyed by id_pose, the report; the two write the same bytes, and the readers of the next
    stage take the document (adjust.sfm_arrays is structure.run's parser; the end-to-end test runs it and sfmloc_open)"""
    import subprocess
    from sfmlocalization_amd.adjust import sfm_arrays
    s, g = ref["ring"]["s"], ref["ring"]["got"]
    ids = [10 + 3 * v for v in range(s["n_views"])]
    doc = {"sfm_data_version": "0.3", "root_path": "/", "views": [{"key": i, "value": {"ptr_wrapper": {"data": {
        "filename": f"f{i}.jpg", "width": 640, "height": 480, "id_view": i, "id_intrinsic": 0, "id_pose": i + 100}}}}
        for i in ids], "intrinsics": [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole",
                                                            "ptr_wrapper": {"id": 1, "data": {
                                                                "width": 640, "height": 480, "focal_length": 700.0,
                                                                "principal_point": [320.0, 240.0]}}}}],
        "structure": [{"key": 0}], "note": "kept"}                  # (no extrinsics, no control_points: both are added)
    entries = [{"I": ids[a], "J": ids[b], "R": s["rel_R"][k].tolist(), "t": s["rel_t"][k].tolist(), "n_inliers": 50,
                "front": [0, 50 if s["use_t"][k] else 49, 0, 0], "choice": 1}
               for k, (a, b) in enumerate(s["pairs"].tolist())]
    (tmp_path / "in.json").write_text(json.dumps(doc))
    (tmp_path / "poses.json").write_text(json.dumps({"relative_poses": entries}))
    (tmp_path / "poses2.json").write_text(json.dumps({"relative_poses": entries[:2]}))       # no triangle
    programs = {"py": [sys.executable, "-m", "sfmlocalization_amd.globalposes"],
                "cpp": [os.path.join(ROOT, "sfmlocalization_amd", "bin", globalposes.NAME)]}
    written = {}
    for name, prog in programs.items():
        o, r = tmp_path / f"out_{name}.json", tmp_path / f"rep_{name}.json"
        p = subprocess.run(prog + ["-i", str(tmp_path / "in.json"), "-p", str(tmp_path / "poses.json"), "-o", str(o),
                                   "-r", str(r), "--triplet-angle", "5"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-1000:]
        lines = p.stdout.splitlines()
        assert lines[0] == "#views: 16; #pairs: 40, with a translation: 39"        # (one pair's use_t is 0)
        assert lines[-1].startswith("Global poses: 12 of 16 views; 36 of 40 pairs kept; steps: rotation ")
        written[name] = (o.read_bytes(), json.loads(r.read_text()))
        # no triplet passes: a message, exit 1, no output; a bad command line: the usage, exit 1
        p = subprocess.run(prog + ["-i", str(tmp_path / "in.json"), "-p", str(tmp_path / "poses2.json"), "-o",
                                   str(tmp_path / f"none_{name}.json")], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 1 and "no triplet of the 2 pairs passes" in p.stderr
        assert not (tmp_path / f"none_{name}.json").exists()
        p = subprocess.run(prog + ["-i", "x", "-p", "y"], capture_output=True, text=True, cwd=ROOT, timeout=300)
        assert p.returncode == 1 and p.stderr == globalposes.USAGE
    assert written["py"][0] == written["cpp"][0]
    timed = [k for k in globalposes.REPORT_FIELDS if k.endswith("_ms")] + ["launches"]
    assert list(written["py"][1]) == list(written["cpp"][1]) == list(globalposes.REPORT_FIELDS)
    assert {k: v for k, v in written["py"][1].items() if k not in timed} == \
        {k: v for k, v in written["cpp"][1].items() if k not in timed}
    out = json.loads(written["py"][0])
    assert list(out) == ["sfm_data_version", "root_path", "views", "intrinsics", "structure", "note", "extrinsics",
                         "control_points"]
    assert out["views"] == doc["views"] and out["structure"] == [] and out["control_points"] == []
    assert [e["key"] for e in out["extrinsics"]] == [i + 100 for i in ids[:12]]
    # (json.dump writes the shortest text that reads back as the same double)
    assert np.array_equal(np.array([e["value"]["rotation"] for e in out["extrinsics"]]), g.R[:12])
    assert np.array_equal(np.array([e["value"]["center"] for e in out["extrinsics"]]), g.C[:12])
    arrays, pose_id, _ = sfm_arrays(out)
    assert int(arrays["pose_valid"].sum()) == 12 and pose_id == [i + 100 for i in ids]
    rep = written["py"][1]
    assert rep["n_component_views"] == 12 and rep["device_ms"] > 0 and rep["chordal_cost"] > 0


def test_end_to_end_from_features_and_matches(expected, tmp_path):
    """globalsfm.run on the planted six views: relative poses, global poses, tracks, triangulation, cleanup and the joint
    adjustment; the centres against the planted ones within what the CPU chain of the two restatements leaves"""
    s = sc.scene_files(str(tmp_path))
    lines = []
    assert globalsfm.run(s["path"], str(tmp_path), str(tmp_path / "out"), log=lines.append) == 0
    out = json.loads((tmp_path / "out" / "sfm_data.json").read_text())
    assert [e["key"] for e in out["extrinsics"]] == sc.E2E_VIEW_ID and len(out["structure"]) > 100
    assert os.path.exists(tmp_path / "out" / "matches.e.txt") and os.path.exists(tmp_path / "out" / "relative_poses.json")
    R = np.array([e["value"]["rotation"] for e in out["extrinsics"]])
    C = np.array([e["value"]["center"] for e in out["extrinsics"]])
    rot, cen = sc.errors(s, np.ones(6, bool), 0, R @ R[0].T, C)
    print("end to end: rotation", rot, "deg, centre", cen, "of the extent; the CPU chain's:", expected["chain"], lines[-6:])
    margin = bound_of(expected["chain"]["parity"])           # (the chain scene's own two-solver distances)
    assert cen <= expected["chain"]["centre"] + margin["C"]
    assert rot <= expected["chain"]["rotation_deg"] + np.degrees(3.0 * margin["R"])
    # sfmloc_open reads the result as it reads any map (the descriptors it wants beside the features: zeros)
    from sfmlocalization_amd import fileio
    import sfmlocalization_amd as S
    for k, f in enumerate(s["feats"]):
        fileio.write_desc(str(tmp_path / f"frame{k:04d}.desc"), np.zeros((len(f), 64), np.uint8))
    with S.Map.open(str(tmp_path / "out"), str(tmp_path)) as m:
        info = m.info()
        assert info["n_views"] == 6 and info["n_landmarks"] == len(out["structure"])
        assert np.array_equal(m.view_id, sc.E2E_VIEW_ID) and np.allclose(m.view_center, C, atol=0)


def test_timing_tool_writes_its_record(tmp_path):
    import subprocess
    out = tmp_path / "time.json"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "globalposes_time.py"), "--views", "40", "--repeats", "1",
                        "--out", str(out), "--commit", "test"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    doc = json.loads(out.read_text())
    assert (doc["commit"], doc["views"], doc["pairs"], len(doc["runs"])) == ("test", 40, 185, 1)
    run = doc["runs"][0]
    assert set(globalposes.REPORT_FIELDS) | {"wall_s", "rotation_error_deg", "centre_error"} == set(run)
    assert run["n_component_views"] == 40 and run["launches"] > 0 and run["trans_pcg_total"] > 0
    assert 0.0 < run["graph_ms"] + run["rotation_ms"] + run["translation_ms"] <= run["device_ms"]
    assert doc["numpy"]["wall_s"] > 0.0 and doc["numpy_note"] == "a restatement, not a competitor"
