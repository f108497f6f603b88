"""The separable bundle adjustment on the device (sfmloc_sfm_adjust, bin/OpenMVG_BA -c, python -m
sfmlocalization_amd.adjust -c) against the CPU twin (adjust_ba_np) on the scene of adjust_ba_scene.  The bounds are
multiples of what the twin's two solvers leave between them (d_ref, c_ref: test_adjust_ba_cpu), four times because the
kernels' reduction tree orders the sums differently from both."""
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

import adjust_ba_np as BN  # noqa: E402
import adjust_ba_scene as BS  # noqa: E402
import adjust_np as AN  # noqa: E402
from sfmlocalization_amd import adjust  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402
from test_adjust_ba_cpu import NAMES, bits, record_parity  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVG_BA")
PROGRAMS = (("cpp", [BIN]), ("py", [sys.executable, "-m", "sfmlocalization_amd.adjust"]))


@pytest.fixture(scope="module")
def ref():
    return BS.reference()


def adjusted(a, what):
    """a fresh handle, the first cleanup, one adjustment -> (report, poses, X, masks)"""
    h = S.Sfm(**a)
    try:
        counts = h.clean(*BS.FIRST_CLEAN, False)
        rep = h.adjust(what)
        return rep, h.read(), h.read_structure(), counts
    finally:
        h.close()


@pytest.fixture(scope="module")
def device(ref):
    return {what: adjusted(ref["a"], what) for what in BS.COMMANDS}


@pytest.mark.parametrize("what", BS.COMMANDS)
def test_parity_with_the_twin(ref, device, what):
    a, c = ref["a"], ref["cmd"][what]
    rep, got, X, counts = device[what]
    tw = c["scipy"]
    blocks = np.array(tw["blocks"])
    assert counts == ref["first_counts"]
    np.testing.assert_array_equal(got["obs_keep"], ref["obs_keep"])
    np.testing.assert_array_equal(got["landmark_keep"], ref["landmark_keep"])
    R, C = got["pose_R"].reshape(-1, 9), got["pose_C"]
    if what == 8:
        x = X[blocks]
    else:
        aa = np.array([BN.nearest_angle_axis(BN.angle_axis(R[p]), tw["aa"][p]) for p in blocks])
        t = BN.t_of(R[blocks], C[blocks])
        x = aa if what == 1 else t if what == 2 else np.concatenate([aa, t], 1)
    dist = BS.block_distances(what, x, tw["x"])
    # (r holds t: the cost is evaluated at the input's t, not at -R C of the centre the device derived from it)
    cost = BN.block_costs(a, what, R, C, X, ref["obs_keep"], ref["landmark_keep"],
                          t=BN.t_of(a["pose_R"], a["pose_C"]) if what == 1 else None)
    cost1 = np.array([cost[int(b)] for b in blocks])
    c_dist = float((np.abs(cost1 - tw["cost1"]) / tw["cost1"]).max())
    print(NAMES[what], "distance to the twin", dist, "d_ref", c["d_ref"], "relative cost distance", c_dist, "c_ref",
          c["c_ref"], "largest step count", rep.max_iterations, "unchanged", rep.n_unchanged)
    record_parity("device_" + NAMES[what], {"distance": dist, "cost_distance": c_dist, "max_iterations": rep.max_iterations})
    for kind, d in dist.items():
        assert d <= 4.0 * c["d_ref"][kind], (kind, d, c["d_ref"][kind])
    assert c_dist <= 4.0 * c["c_ref"], (c_dist, c["c_ref"])
    # conditions
    assert (cost1 <= tw["cost0"]).all()                                     # no block above its input cost
    assert rep.n_blocks == len(blocks) and rep.n_at_cap == 0 and rep.n_unchanged == 0
    assert rep.cost_final < rep.cost_initial
    assert abs(rep.cost_initial - tw["cost0"].sum()) <= 1e-9 * tw["cost0"].sum()
    assert abs(rep.cost_final - tw["cost1"].sum()) <= 1e-9 * tw["cost1"].sum()
    assert np.isfinite(X).all() and np.isfinite(R).all() and np.isfinite(C).all()
    if what == 8:                                                           # the poses and the dropped landmark keep their bits
        np.testing.assert_array_equal(bits(R), bits(a["pose_R"]))
        np.testing.assert_array_equal(bits(C), bits(a["pose_C"]))
        np.testing.assert_array_equal(bits(X[BS.LM_DROPPED]), bits(a["landmark_X"][BS.LM_DROPPED]))
        assert np.isfinite(X[BS.LM_PARALLEL]).all() and (X[BS.LM_PARALLEL] != a["landmark_X"][BS.LM_PARALLEL]).any()
    else:
        np.testing.assert_array_equal(bits(X), bits(a["landmark_X"]))
        for p in (int(a["view_pose"][BS.VIEW_UNSEEN]), ref["pose_id"].index(BS.ORPHAN_POSE)):
            np.testing.assert_array_equal(bits(R[p]), bits(a["pose_R"][p]))
            np.testing.assert_array_equal(bits(C[p]), bits(a["pose_C"][p]))
        if what == 2:                                                       # t holds the rotation's bits
            np.testing.assert_array_equal(bits(R), bits(a["pose_R"]))
        if what == 1:                                                       # r holds t and moves the centre
            assert np.abs(BN.t_of(R[blocks], C[blocks]) - BN.t_of(a["pose_R"][blocks], a["pose_C"][blocks])).max() < 1e-13
            assert (np.abs(C[blocks] - a["pose_C"][blocks]).max(1) > 1e-4).all()


def test_nothing_and_refused(ref):
    a = ref["a"]
    h = S.Sfm(**a)
    try:
        for what in (0, 11, 4, 9, 16):
            if what:
                with pytest.raises(S.SfmlocError) as ei:
                    h.adjust(what)
                assert ei.value.code == S.EINVAL and "-c" in ei.value.message
            else:
                rep = h.adjust(0)
                assert rep.n_blocks == 0 and rep.max_iterations == 0
            got = h.read(masks=False)
            np.testing.assert_array_equal(bits(got["pose_R"].reshape(-1, 9)), bits(a["pose_R"]))
            np.testing.assert_array_equal(bits(got["pose_C"]), bits(a["pose_C"]))
            np.testing.assert_array_equal(bits(h.read_structure()), bits(a["landmark_X"]))
    finally:
        h.close()


def test_view_without_pose_is_named(ref):
    a = dict(ref["a"])
    v = 12
    a["pose_valid"] = a["pose_valid"].copy()
    a["pose_valid"][a["view_pose"][v]] = 0
    h = S.Sfm(**a)
    try:
        for what in (8, 3):
            with pytest.raises(S.SfmlocError) as ei:
                h.adjust(what)
            assert ei.value.code == S.EINVAL and f"view {int(a['view_id'][v])} " in ei.value.message
        np.testing.assert_array_equal(bits(h.read_structure()), bits(a["landmark_X"]))
    finally:
        h.close()


def test_two_runs_same_bits(ref, device):
    for what in (8, 3):
        rep, got, X, _ = adjusted(ref["a"], what)
        rep0, got0, X0, _ = device[what]
        np.testing.assert_array_equal(bits(X), bits(X0))
        np.testing.assert_array_equal(bits(got["pose_R"]), bits(got0["pose_R"]))
        np.testing.assert_array_equal(bits(got["pose_C"]), bits(got0["pose_C"]))
        assert (rep.cost_final, rep.max_iterations) == (rep0.cost_final, rep0.max_iterations)


def test_clean_after_adjust_and_again(ref):
    """adjust, clean, adjust, clean on one handle: the second cleanup works on what the first kept"""
    a = ref["a"]
    h = S.Sfm(**a)
    try:
        h.adjust(3)
        p1, X0 = h.read(masks=False), h.read_structure()
        c1 = h.clean(4.0, 2.0, True)
        m1 = h.read()
        want = AN.clean(a, a["pose_valid"], p1["pose_R"].reshape(-1, 9), p1["pose_C"], rm_unstable=True)
        assert c1 == want["counts"]
        np.testing.assert_array_equal(m1["obs_keep"], want["obs_keep"])
        np.testing.assert_array_equal(m1["landmark_keep"], want["landmark_keep"])
        rep = h.adjust(8)
        assert rep.n_blocks == c1[3] and rep.n_at_cap == 0
        X1 = h.read_structure()
        gone = ~m1["landmark_keep"]
        np.testing.assert_array_equal(bits(X1[gone]), bits(X0[gone]))
        c2 = h.clean(4.0, 2.0, True)
        m2 = h.read()
        assert c2[0] == c1[3] and c2[3] <= c2[0]
        assert not (m2["landmark_keep"] & ~m1["landmark_keep"]).any() and not (m2["obs_keep"] & ~m1["obs_keep"]).any()
    finally:
        h.close()


def _run(prog, args):
    return subprocess.run(prog + args, capture_output=True, text=True, cwd=ROOT, timeout=300)


def _lines(stdout):
    return [ln for ln in stdout.splitlines() if not ln.startswith("Reading")]


def test_tool_commands(ref, tmp_path):
    doc = ref["doc"]
    outs = {}
    for cmd in (["-c=s"], ["-c=rt,sc", "-r=1"], ["-c=c"], []):
        for name, prog in PROGRAMS:
            d = tmp_path / (name + "_" + "_".join(cmd).replace("=", "").replace(",", "+"))
            d.mkdir()
            (d / "sfm_data.json").write_text(json.dumps(doc))
            r = _run(prog, [str(d / "sfm_data.json"), str(d / "out.json")] + cmd)
            assert r.returncode == 0, (name, cmd, r.stderr)             # (-c=s: status 1 before this feature)
            outs[name, tuple(cmd)] = ((d / "out.json").read_bytes(), (d / "sfm_data_b4bd.json").read_bytes(), _lines(r.stdout))
        assert outs["cpp", tuple(cmd)] == outs["py", tuple(cmd)], cmd
    head = ["Start bundle adjustment over sfm_data.json.", "Warning: there is/are frames with too few matches."]
    # -c=s
    out, b4, lines = outs["cpp", ("-c=s",)]
    assert lines == head + ["", "Bundle adjustment over structure, "]
    o, b = json.loads(out), json.loads(b4)
    assert json.dumps(o) == out.decode() and list(o) == list(doc)
    assert o["extrinsics"] == b["extrinsics"] and len(o["structure"]) == len(doc["structure"])
    assert [e["value"]["observations"] for e in o["structure"]] == [e["value"]["observations"] for e in doc["structure"]]
    moved = sum(e["value"]["X"] != f["value"]["X"] for e, f in zip(o["structure"], doc["structure"]))
    assert moved == len(doc["structure"])
    # -c=rt,sc -r=1 against the twin from the poses the tool resected (sfm_data_b4bd.json)
    out, b4, lines = outs["cpp", ("-c=rt,sc", "-r=1")]
    a, _, _ = adjust.sfm_arrays(json.loads(b4))
    rt = BN.adjust(a, 3, a["pose_R"], a["pose_C"], a["landmark_X"])
    s = BN.adjust(a, 8, rt["pose_R"], rt["pose_C"], a["landmark_X"])
    want = _clean_with(a, s)
    assert lines == head + ["", "Bundle adjustment over rotations, translations, ", "", "Bundle adjustment over structure, ",
                            f"Number of points before cleanup : {want['counts'][0]}",
                            f"Number of points residual error : {want['counts'][1]}",
                            f"Number of points angle error : {want['counts'][2]}",
                            f"Number of points after cleanup : {want['counts'][3]}"]
    o = json.loads(out)
    assert len(o["structure"]) == want["counts"][3]
    assert [e["key"] for e in o["structure"]] == [int(k) for k in a["landmark_id"][want["landmark_keep"]]]
    ext = {e["key"]: e["value"] for e in o["extrinsics"]}
    assert sorted(ext) == [p for p, ok in zip(ref["pose_id"], want["pose_valid"]) if ok]
    for i, p in enumerate(ref["pose_id"]):
        if want["pose_valid"][i] and i in rt["blocks"]:
            assert np.abs(np.array(ext[p]["center"]) - rt["pose_C"][i]).max() < 1e-6
            assert np.abs(np.array(ext[p]["rotation"]).ravel() - rt["pose_R"][i]).max() < 1e-6
    for e in o["structure"]:
        l = int(np.searchsorted(a["landmark_id"], e["key"]))
        assert np.abs(np.array(e["value"]["X"]) - s["X"][l]).max() < 1e-5
    # -c=c adjusts nothing and cleans: the bytes of the run without -c; so does run() itself, the unchanged path
    assert outs["cpp", ("-c=c",)][:2] == outs["cpp", ()][:2]
    assert outs["cpp", ("-c=c",)][2] == head + ["", "Bundle adjustment over "] + outs["cpp", ()][2][len(head):]
    d = tmp_path / "run"
    d.mkdir()
    (d / "sfm_data.json").write_text(json.dumps(doc))
    assert adjust.run(str(d / "sfm_data.json"), str(d / "out.json"), log=lambda s: None) == 0
    assert (d / "out.json").read_bytes() == outs["py", ()][0] and (d / "sfm_data_b4bd.json").read_bytes() == outs["py", ()][1]


def _clean_with(a, s):
    """adjust_np.clean on the twin's adjusted scene (its X in place of the input's)"""
    b = dict(a)
    b["landmark_X"] = s["X"]
    return AN.clean(b, a["pose_valid"], s["pose_R"], s["pose_C"], rm_unstable=True)
