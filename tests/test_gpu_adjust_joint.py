"""The joint bundle adjustment on the device (sfmloc_sfm_adjust_joint, bin/OpenMVG_BA -j=1, python -m
sfmlocalization_amd.adjust -j=1) against the CPU twin (adjust_joint_np) on the scenes of adjust_joint_scene.

Only gauge-invariant quantities are compared for the commands with a gauge freedom: the residual vectors at the solution
and the total cost.  The bounds are four times what the twin's two solvers leave between them (r_ref, c_ref, d_ref:
test_adjust_joint_cpu), four times because the kernels order their sums differently from both, as in
test_gpu_adjust_ba.  profiles/ba_joint_parity.json records both sides of every bound."""
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
import adjust_joint_np as JN  # noqa: E402
import adjust_joint_scene as JS  # noqa: E402
import adjust_np as AN  # noqa: E402
from sfmlocalization_amd import adjust  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402
from test_adjust_joint_cpu import bits, record_parity  # noqa: E402

pytestmark = pytest.mark.gpu
BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVG_BA")
PROGRAMS = (("cpp", [BIN]), ("py", [sys.executable, "-m", "sfmlocalization_amd.adjust"]))
# the twin's own stop (adjust_joint_np.FTOL), so that both stop by one rule; the linear solves nearly exact
TIGHT = dict(function_tolerance=JN.FTOL, pcg_tolerance=1e-10, max_steps=200, max_pcg=2000)


@pytest.fixture(scope="module")
def ref():
    return JS.reference()


def adjusted(a, what, first_clean=BS.FIRST_CLEAN, **options):
    """a fresh handle, the first cleanup, one joint adjustment -> (report, poses, X, K)"""
    h = S.Sfm(**a)
    try:
        if first_clean:
            h.clean(*first_clean, False)
        rep = h.adjust_joint(what, **options)
        return rep, h.read(masks=bool(first_clean)), h.read_structure(), h.read_intrinsics()
    finally:
        h.close()


@pytest.fixture(scope="module")
def device(ref):
    return {what: adjusted(ref["a"], what, **TIGHT) for what in JS.COMMANDS}


@pytest.fixture(scope="module")
def separable_cost(ref):
    """the cost a recipe of the separable path leaves that the joint command can beat, each on a handle of its own: one
    rt then one s for rst and rsti; rs holds t and rti holds X, so they cannot reach that and face r alone and rt alone"""
    a = ref["a"]
    out = {}
    for what, recipe in ((11, (3, 8)), (15, (3, 8)), (9, (1,)), (7, (3,))):
        h = S.Sfm(**a)
        try:
            h.clean(*BS.FIRST_CLEAN, False)
            for w in recipe:
                h.adjust(w)
            p, X = h.read(), h.read_structure()
        finally:
            h.close()
        t = BN.t_of(a["pose_R"], a["pose_C"]) if recipe == (1,) else None
        out[what] = JN.total_cost(a, p["pose_R"].reshape(-1, 9), p["pose_C"], a["intrinsic"], X, ref["obs_keep"],
                                  ref["landmark_keep"], t=t)
    return out


def check_conditions(a, what, rep, got, X, K, keep=(None, None)):
    """what every joint call must leave: finite, orthonormal, the held parts bit-identical"""
    R, C = got["pose_R"].reshape(-1, 9), got["pose_C"]
    assert np.isfinite(R).all() and np.isfinite(C).all() and np.isfinite(X).all() and np.isfinite(K).all()
    RR = np.einsum("nij,nkj->nik", R.reshape(-1, 3, 3), R.reshape(-1, 3, 3))
    assert np.abs(RR - np.eye(3)).max() < 1e-12
    if not what & 4:
        np.testing.assert_array_equal(bits(K), bits(a["intrinsic"]))
    if not what & 8:
        np.testing.assert_array_equal(bits(X), bits(a["landmark_X"]))
    if not what & 1:
        np.testing.assert_array_equal(bits(R), bits(a["pose_R"]))
    c0 = JN.total_cost(a, a["pose_R"], a["pose_C"], a["intrinsic"], a["landmark_X"], *keep)
    t = BN.t_of(a["pose_R"], a["pose_C"]) if not what & 2 else None
    c1 = JN.total_cost(a, R, C, K, X, *keep, t=t)
    assert abs(rep.cost_initial - c0) <= 1e-9 * c0 and abs(rep.cost_final - c1) <= 1e-9 * c1
    assert rep.cost_final < rep.cost_initial
    return c1


@pytest.mark.parametrize("what", JS.COMMANDS)
def test_parity_with_the_twin(ref, device, separable_cost, what):
    a, c = ref["a"], ref["cmd"][what]
    keep = (ref["obs_keep"], ref["landmark_keep"])
    rep, got, X, K = device[what]
    tw = c["lm"]
    np.testing.assert_array_equal(got["obs_keep"], ref["obs_keep"])
    R, C = got["pose_R"].reshape(-1, 9), got["pose_C"]
    t = BN.t_of(a["pose_R"], a["pose_C"]) if not what & 2 else None          # (r holds t: its bits are the input's)
    r = JN.residuals(a, R, C, K, X, *keep, t=t)
    r_dist = float(np.abs(r - tw["residual"]).max())
    c1 = check_conditions(a, what, rep, got, X, K, keep)
    c_dist = abs(c1 - tw["cost1"]) / tw["cost1"]
    c_bound = 4.0 * c["c_ref"]
    print(JS.NAMES[what], "residual distance", r_dist, "r_ref", c["r_ref"], "cost distance", c_dist, "c_ref", c["c_ref"],
          "cost bound", c_bound, "steps", rep.steps_tried, rep.steps_accepted, "pcg", rep.pcg_total, rep.pcg_max, "stop",
          rep.stop, "cost", rep.cost_initial, "->", rep.cost_final, "separable recipe", separable_cost.get(what))
    values = {"residual_distance": r_dist, "cost_distance": c_dist, "steps_tried": rep.steps_tried,
              "pcg_total": rep.pcg_total, "pcg_max": rep.pcg_max, "stop": rep.stop, "cost_bound": c_bound,
              "residual_bound": 4.0 * c["r_ref"]}
    if what == 7:                                                            # no gauge freedom: the parameters too
        blocks = np.nonzero(JN.Joint(a, 7, a["pose_R"], a["pose_C"], a["intrinsic"], a["landmark_X"], *keep).pose_in)[0]

        def params(s_R, s_t, s_K, near=None):
            aa = np.array([BN.angle_axis(s_R[p]) for p in blocks])
            if near is not None:
                aa = np.array([BN.nearest_angle_axis(w, n) for w, n in zip(aa, near)])
            return aa, s_t[blocks], s_K
        ref_aa, ref_t, ref_K = params(tw["pose_R"], tw["t"], tw["K"])
        sc = c["scipy"]
        sc_aa, sc_t, sc_K = params(sc["pose_R"], sc["t"], sc["K"], ref_aa)
        dv_aa, dv_t, dv_K = params(R, BN.t_of(R, C), K, ref_aa)
        d_ref = {"rotation": float(np.abs(sc_aa - ref_aa).max()), "translation": float(np.abs(sc_t - ref_t).max()),
                 "focal_pp": float(np.abs(sc_K[:, :3] - ref_K[:, :3]).max()), "k": float(np.abs(sc_K[:, 3:] - ref_K[:, 3:]).max())}
        dist = {"rotation": float(np.abs(dv_aa - ref_aa).max()), "translation": float(np.abs(dv_t - ref_t).max()),
                "focal_pp": float(np.abs(dv_K[:, :3] - ref_K[:, :3]).max()), "k": float(np.abs(dv_K[:, 3:] - ref_K[:, 3:]).max())}
        print("rti parameter distances", dist, "d_ref", d_ref)
        values.update(distance=dist, d_ref=d_ref)
    record_parity("device_" + JS.NAMES[what], values)
    assert rep.stop == 0
    assert r_dist <= 4.0 * c["r_ref"], (r_dist, c["r_ref"])
    assert c_dist <= c_bound, (c_dist, c_bound)
    if what == 7:
        for kind, d in dist.items():
            assert d <= 4.0 * d_ref[kind], (kind, d, d_ref[kind])
    if what in separable_cost:
        assert rep.cost_final <= separable_cost[what]
    # what must keep its bits
    for p in (int(a["view_pose"][BS.VIEW_UNSEEN]), ref["pose_id"].index(BS.ORPHAN_POSE)):
        np.testing.assert_array_equal(bits(R[p]), bits(a["pose_R"][p]))
        np.testing.assert_array_equal(bits(C[p]), bits(a["pose_C"][p]))
    np.testing.assert_array_equal(bits(X[BS.LM_DROPPED]), bits(a["landmark_X"][BS.LM_DROPPED]))
    moved = JN.Joint(a, what, a["pose_R"], a["pose_C"], a["intrinsic"], a["landmark_X"], *keep).pose_in
    np.testing.assert_array_equal(bits(R[~moved]), bits(a["pose_R"][~moved]))
    np.testing.assert_array_equal(bits(C[~moved]), bits(a["pose_C"][~moved]))
    assert rep.n_pose_blocks == moved.sum() and (moved.sum() > 1024 if what & 3 else moved.sum() == 0) and rep.n_intrinsic_blocks == (2 if what & 4 else 0)
    assert rep.n_landmark_blocks == (BS.N_LM - 1 if what & 8 else 0)
    if what == 9:
        assert np.abs(BN.t_of(R, C) - BN.t_of(a["pose_R"], a["pose_C"])).max() < 1e-13
    if what & 4:
        np.testing.assert_array_equal(bits(K[0, 3:]), bits(a["intrinsic"][0, 3:]))
    # the shared pose: one block, one R, C for both its views
    assert a["view_pose"][BS.VIEW_SHARED[0]] == a["view_pose"][BS.VIEW_SHARED[1]]
    assert bool(moved[a["view_pose"][BS.VIEW_SHARED[0]]]) == bool(what & 3)


def test_refused_and_view_without_pose(ref):
    a = dict(ref["a"])
    h = S.Sfm(**a)
    try:
        for what in (0, 16, 31):
            with pytest.raises(S.SfmlocError) as ei:
                h.adjust_joint(what)
            assert ei.value.code == S.EINVAL
    finally:
        h.close()
    v = 12
    a["pose_valid"] = a["pose_valid"].copy()
    a["pose_valid"][a["view_pose"][v]] = 0
    h = S.Sfm(**a)
    try:
        for what in (11, 4):
            with pytest.raises(S.SfmlocError) as ei:
                h.adjust_joint(what)
            assert ei.value.code == S.EINVAL and f"view {int(a['view_id'][v])} " in ei.value.message
        np.testing.assert_array_equal(bits(h.read_structure()), bits(a["landmark_X"]))
        np.testing.assert_array_equal(bits(h.read_intrinsics()), bits(a["intrinsic"]))
    finally:
        h.close()


def test_two_runs_same_bits(ref, device):
    for what in (11, 15):
        rep, got, X, K = adjusted(ref["a"], what, **TIGHT)
        rep0, got0, X0, K0 = device[what]
        np.testing.assert_array_equal(bits(X), bits(X0))
        np.testing.assert_array_equal(bits(K), bits(K0))
        np.testing.assert_array_equal(bits(got["pose_R"]), bits(got0["pose_R"]))
        np.testing.assert_array_equal(bits(got["pose_C"]), bits(got0["pose_C"]))
        assert (rep.cost_final, rep.steps_tried, rep.pcg_total) == (rep0.cost_final, rep0.steps_tried, rep0.pcg_total)


def test_default_options(ref):
    a = ref["a"]
    rep, got, X, K = adjusted(a, 15)
    print("rsti at the default options: steps", rep.steps_tried, rep.steps_accepted, "pcg", rep.pcg_total, rep.pcg_max,
          "stop", rep.stop, "cost", rep.cost_initial, "->", rep.cost_final)
    assert rep.stop in (0, 1) and rep.steps_tried <= 50 and rep.pcg_max <= 500
    check_conditions(a, 15, rep, got, X, K, (ref["obs_keep"], ref["landmark_keep"]))


@pytest.mark.parametrize("second", (False, True))
def test_small_scene(second):
    """3 views, 8 landmarks, everything inside one wave; with `second` an intrinsic nothing refers to"""
    a = JS.small(second)
    for what in (11, 7):
        c = JS.twins(a, what)
        rep, got, X, K = adjusted(a, what, first_clean=None, **TIGHT)
        c1 = check_conditions(a, what, rep, got, X, K)
        t = BN.t_of(a["pose_R"], a["pose_C"]) if not what & 2 else None
        r = JN.residuals(a, got["pose_R"].reshape(-1, 9), got["pose_C"], K, X, t=t)
        r_dist, c_dist = float(np.abs(r - c["lm"]["residual"]).max()), abs(c1 - c["lm"]["cost1"]) / c["lm"]["cost1"]
        print("small", JS.NAMES[what], "residual distance", r_dist, "r_ref", c["r_ref"], "cost distance", c_dist, "c_ref",
              c["c_ref"], "steps", rep.steps_tried, "pcg", rep.pcg_total, "stop", rep.stop)
        assert rep.stop == 0
        assert r_dist <= 4.0 * c["r_ref"] and c_dist <= 4.0 * c["c_ref"]
        if second:
            np.testing.assert_array_equal(bits(K[2]), bits(a["intrinsic"][2]))
    rep, got, X, K = adjusted(a, 15, first_clean=None, **TIGHT)
    check_conditions(a, 15, rep, got, X, K)
    assert rep.n_intrinsic_blocks == 2
    if second:
        np.testing.assert_array_equal(bits(K[2]), bits(a["intrinsic"][2]))


def test_sequencing_on_one_handle(ref):
    """joint 15, clean, joint 11, clean: a cleanup sees the adjusted poses, X and intrinsics; the second works on what
    the first kept; the separable entry point still refuses 11"""
    a = ref["a"]
    h = S.Sfm(**a)
    try:
        h.adjust_joint(15)
        p1, X1, K1 = h.read(masks=False), h.read_structure(), h.read_intrinsics()
        assert (K1[:, :3] != a["intrinsic"][:, :3]).all()
        c1 = h.clean(4.0, 2.0, True)
        m1 = h.read()
        b = dict(a, landmark_X=X1, intrinsic=K1)
        want = AN.clean(b, a["pose_valid"], p1["pose_R"].reshape(-1, 9), p1["pose_C"], rm_unstable=True)
        assert c1 == want["counts"]
        np.testing.assert_array_equal(m1["obs_keep"], want["obs_keep"])
        np.testing.assert_array_equal(m1["landmark_keep"], want["landmark_keep"])
        rep = h.adjust_joint(11)
        assert rep.n_landmark_blocks == c1[3] and rep.cost_final < rep.cost_initial
        np.testing.assert_array_equal(bits(h.read_intrinsics()), bits(K1))
        gone = ~m1["landmark_keep"]
        np.testing.assert_array_equal(bits(h.read_structure()[gone]), bits(X1[gone]))
        c2 = h.clean(4.0, 2.0, True)
        m2 = h.read()
        assert c2[0] == c1[3] and c2[3] <= c2[0]
        assert not (m2["landmark_keep"] & ~m1["landmark_keep"]).any() and not (m2["obs_keep"] & ~m1["obs_keep"]).any()
        with pytest.raises(S.SfmlocError) as ei:
            h.adjust(11)
        assert ei.value.code == S.EINVAL and "-c" in ei.value.message
    finally:
        h.close()


def _run(prog, args):
    return subprocess.run(prog + args, capture_output=True, text=True, cwd=ROOT, timeout=300)


def _lines(stdout):
    return [ln for ln in stdout.splitlines() if not ln.startswith("Reading")]


def test_tools(tmp_path):
    doc = BS.reference()["doc"]
    outs = {}
    for tag, args in (("joint", ["IN", "OUT", "-c=rst,rstic", "-r=1", "-j=1"]), ("first", ["-j=1", "IN", "OUT", "-c=rst,rstic", "-r=1"]),
                      ("sep_j", ["IN", "OUT", "-c=rt,sc", "-r=1", "--joint=1"]), ("sep", ["IN", "OUT", "-c=rt,sc", "-r=1"])):
        for name, prog in PROGRAMS:
            if tag in ("first", "sep") and name == "py":
                continue
            d = tmp_path / (name + "_" + tag)
            d.mkdir()
            (d / "sfm_data.json").write_text(json.dumps(doc))
            r = _run(prog, [{"IN": str(d / "sfm_data.json"), "OUT": str(d / "out.json")}.get(x, x) for x in args])
            assert r.returncode == 0, (name, tag, r.stderr)                 # (status 1 before this feature)
            outs[name, tag] = ((d / "out.json").read_bytes(), (d / "sfm_data_b4bd.json").read_bytes(), _lines(r.stdout))
    assert outs["cpp", "joint"] == outs["py", "joint"] == outs["cpp", "first"]
    assert outs["cpp", "sep_j"] == outs["py", "sep_j"] == outs["cpp", "sep"]
    out, b4, lines = outs["cpp", "joint"]
    # the C calls in the tool's order, from the poses the tool resected
    a, pose_id, _ = adjust.sfm_arrays(doc)
    h = S.Sfm(**a, params=S.sfm_default_params())
    try:
        h.resect()
        h.adjust_joint(11)
        h.adjust_joint(15)
        counts = h.clean(adjust.RESIDUAL_PX, adjust.ANGLE_DEG, True)
        q, X, K = h.read(), h.read_structure(), h.read_intrinsics()
    finally:
        h.close()
    head = ["Start bundle adjustment over sfm_data.json.", "Warning: there is/are frames with too few matches."]
    assert lines == head + ["", "Bundle adjustment over rotations, translations, structure, ", "",
                            "Bundle adjustment over rotations, translations, intrinsic params, structure, ",
                            f"Number of points before cleanup : {counts[0]}", f"Number of points residual error : {counts[1]}",
                            f"Number of points angle error : {counts[2]}", f"Number of points after cleanup : {counts[3]}"]
    o, b = json.loads(out), json.loads(b4)
    assert json.dumps(o) == out.decode() and list(o) == list(doc)
    assert b["intrinsics"] == doc["intrinsics"] and b["structure"] == doc["structure"]
    ao, _, _ = adjust.sfm_arrays(o)
    np.testing.assert_array_equal(bits(ao["intrinsic"]), bits(K))
    assert (K[:, :3] != a["intrinsic"][:, :3]).all()
    np.testing.assert_array_equal(bits(ao["landmark_X"]), bits(X[q["landmark_keep"]]))
    ext = {e["key"]: e["value"] for e in o["extrinsics"]}
    assert sorted(ext) == [p for p, ok in zip(pose_id, q["pose_valid"]) if ok]
    for i, p in enumerate(pose_id):
        if q["pose_valid"][i]:
            np.testing.assert_array_equal(bits(np.array(ext[p]["rotation"]).ravel()), bits(q["pose_R"][i].ravel()))
            np.testing.assert_array_equal(bits(np.array(ext[p]["center"])), bits(q["pose_C"][i]))
