"""GPU: sfmloc_wedge_scales against its NumPy restatement (tests/pairscales_np.py) on the scenes of
tests/pairscales_scene.py.  The stage is order-fixed f64 arithmetic up to the depths and a selection afterwards, so the
records are compared bit for bit."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import pairscales_np as tw  # noqa: E402
import pairscales_scene as sc  # noqa: E402
import globalposes_scene as gs  # noqa: E402
from sfmlocalization_amd import capi, fileio, relpose  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(HERE)
PROGRAMS = [("cpp", [os.path.join(ROOT, "sfmlocalization_amd", "bin", relpose.NAME)]),
            ("py", [sys.executable, "-m", "sfmlocalization_amd.relpose"])]
MAKERS = dict(triplet=sc.scene_triplet, corridor=sc.scene_corridor, boundaries=sc.scene_boundaries)


@pytest.fixture(scope="module")
def scenes():
    """every scene with the restatement's result on it: computed once, left unchanged"""
    out = {}
    for name, make in MAKERS.items():
        s = make()
        out[name] = (s, tw.wedge_scales(**s["call"]))
    return out


def as_records(ref):
    """the restatement's list as the device's record array"""
    rec = np.zeros(len(ref), capi.WSCALE)
    for i, r in enumerate(ref):
        rec[i] = r
    return rec


def same_bits(got, want):
    assert got.dtype == want.dtype == capi.WSCALE and len(got) == len(want)
    for f in ("view", "k", "l", "n_shared"):
        assert np.array_equal(got[f], want[f]), f
    bad = np.nonzero(got["ratio"].view(np.uint64) != want["ratio"].view(np.uint64))[0]
    assert len(bad) == 0, (len(bad), got[bad[:5]], want[bad[:5]])


def permuted(call, perm):
    """the same call with pair perm[i] in place i"""
    c = dict(call)
    c["pairs"], c["rel_R"], c["rel_t"] = call["pairs"][perm], call["rel_R"][perm], call["rel_t"][perm]
    for off, names in (("offsets", ("match_i", "match_j")), ("inl_off", ("inl_idx",))):
        o = call[off].astype(np.int64)
        c[off] = np.concatenate([[0], np.cumsum((o[1:] - o[:-1])[perm])]).astype(np.uint64)
        for n in names:
            c[n] = np.concatenate([call[n][o[k]:o[k + 1]] for k in perm])
    return c


@pytest.mark.parametrize("name", list(MAKERS))
def test_records_are_the_restatements_bits(scenes, name):
    s, ref = scenes[name]
    w = capi.WedgeScales(**s["call"])
    same_bits(w.records, as_records(ref["records"]))
    rep = w.report
    P = len(s["pairs"])
    assert (rep.n_pairs, rep.n_pairs_used, rep.n_inliers) == (P, P, int(s["call"]["inl_off"][-1]))
    assert (rep.n_depths, rep.n_candidates, rep.n_wedges) == (ref["n_depths"], ref["n_candidates"], len(ref["records"]))
    assert rep.launches > 0 and rep.device_ms > 0.0 and w.ms == rep.device_ms
    assert len(w.records) == {"triplet": 3, "corridor": 158}.get(name, len(w.records)) > 0


def test_boundary_scene_takes_every_path(scenes):
    s, ref = scenes["boundaries"]
    rec = capi.WedgeScales(**s["call"]).records

    def of(group):
        return rec[np.isin(rec["k"], s[group]["pairs"]) | np.isin(rec["l"], s[group]["pairs"])]
    assert len(rec) > 256 and ref["n_candidates"] > len(rec)                   # candidates that are not emitted
    hub = rec[rec["view"] == s["hub"]]
    assert 0 < len(hub) < 80 * 79 // 2                                         # the wave's view
    assert len(of("short")) == 0                                               # min_shared - 1 shared features
    assert of("exact")["n_shared"].tolist() == [8] and of("exact")["view"].tolist() == [s["exact"]["views"][0]]
    big = of("big")
    assert big["n_shared"].tolist() == [2100] * 3 and sorted(big["view"].tolist()) == s["big"]["views"]
    c, lists = s["call"], ref["lists"]
    k, l = s["big"]["pairs"][:2]
    uncapped = tw.wedge_ratio(*lists[(k, 0)], *lists[(l, 1)], max_shared=2100)
    capped = tw.wedge_ratio(*lists[(k, 0)], *lists[(l, 1)], max_shared=2048)
    assert uncapped[1] != capped[1] == big[0]["ratio"]                         # the cap is what the device applied
    rp = of("repeat")
    assert rp["n_shared"].tolist() == [20]                                     # a feature named twice counts once
    k = s["repeat"]["pairs"][0]
    assert len(lists[(k, 0)][0]) == len(set(c["match_i"][int(c["offsets"][k]):int(c["offsets"][k + 1])].tolist()))
    assert len(of("behind")[np.isin(of("behind")["k"], s["behind"]["pairs"][:1])]) == 0   # nothing in front: no list
    assert len(lists[(s["behind"]["pairs"][0], 0)][0]) == 0


def test_two_runs_give_the_same_bits(scenes):
    s, _ = scenes["boundaries"]
    a, b = capi.WedgeScales(**s["call"]), capi.WedgeScales(**s["call"])
    assert a.records.tobytes() == b.records.tobytes()


@pytest.mark.parametrize("name", ["corridor", "boundaries"])
def test_a_permuted_pair_list_gives_the_same_records(scenes, name):
    """a record depends on its two pairs alone; the order of the list only decides which of them is k, and with it
    whether the quotients are z_k / z_l or their inverses (the lower median of the inverses is the inverse of the upper
    median, so such a record is held to the restatement on the two lists in the new order, not to the old record)"""
    s, ref = scenes[name]
    perm = np.random.default_rng(5).permutation(len(s["pairs"]))
    got = capi.WedgeScales(**permuted(s["call"], perm)).records
    want = {(v, k, l): (n, q) for v, k, l, n, q in ref["records"]}
    assert len(got) == len(want)
    kept = swapped = 0
    for v, k, l, n, q in got.tolist():
        a, b = int(perm[k]), int(perm[l])
        n0, q0 = want[(v, min(a, b), max(a, b))]
        assert n == n0
        if a < b:
            assert np.float64(q).view(np.uint64) == np.float64(q0).view(np.uint64)
            kept += 1
        else:
            pairs = s["pairs"].tolist()
            q1 = tw.wedge_ratio(*ref["lists"][(a, int(pairs[a][1] == v))], *ref["lists"][(b, int(pairs[b][1] == v))])[1]
            assert np.float64(q).view(np.uint64) == np.float64(q1).view(np.uint64)
            swapped += 1
    assert kept > 10 and swapped > 10
    if name == "corridor":
        c = permuted(s["call"], perm)
        same_bits(capi.WedgeScales(**c).records, as_records(tw.wedge_scales(**c)["records"]))


def test_options_and_pairs_left_out(scenes):
    s, ref = scenes["corridor"]
    c = s["call"]
    use = np.ones(len(s["pairs"]), np.uint8)
    use[[0, 7, s["wrong_pair"]]] = 0
    w = capi.WedgeScales(**c, use_pair=use)
    want = [r for r in ref["records"] if use[r[1]] and use[r[2]]]
    same_bits(w.records, as_records(want))
    assert w.report.n_pairs_used == len(use) - 3 and w.report.n_candidates == len(want) < ref["n_candidates"]
    # a cap inside the lists and a higher floor: another median of other quotients
    for opt in (dict(min_shared=40, max_shared=16), dict(min_shared=1, max_shared=1), dict(min_shared=2048)):
        w = capi.WedgeScales(**c, **opt)
        want = tw.wedge_scales(**c, **{**tw.OPTIONS, **opt})["records"]
        same_bits(w.records, as_records(want))
        assert len(want) < len(ref["records"]) or opt.get("max_shared") == 1
    assert any(a[4] != b[4] for a, b in zip(tw.wedge_scales(**c, max_shared=16)["records"], ref["records"]))


def test_empty_calls(scenes):
    s, _ = scenes["triplet"]
    c = s["call"]
    none = dict(c, pairs=np.zeros((0, 2), np.uint32), offsets=np.zeros(1, np.uint64), match_i=[], match_j=[],
                rel_R=np.zeros((0, 3, 3)), rel_t=np.zeros((0, 3)), inl_off=np.zeros(1, np.uint64), inl_idx=[])
    w = capi.WedgeScales(**none)
    assert len(w.records) == 0 and (w.report.n_pairs, w.report.n_wedges, w.report.launches) == (0, 0, 0)
    # pairs without inliers: candidates, no depths, no records
    w = capi.WedgeScales(**dict(c, inl_off=np.zeros(4, np.uint64), inl_idx=[]))
    assert len(w.records) == 0 and (w.report.n_candidates, w.report.n_depths, w.report.launches) == (3, 0, 0)
    # one pair alone: no candidate
    w = capi.WedgeScales(**c, use_pair=[0, 1, 0])
    assert len(w.records) == 0 and (w.report.n_pairs_used, w.report.n_candidates) == (1, 0)
    # inliers in one pair of a wedge only
    w = capi.WedgeScales(**dict(c, inl_off=np.array([0, 40, 40, 40], np.uint64), inl_idx=c["inl_idx"][:40]))
    assert len(w.records) == 0 and (w.report.n_inliers, w.report.n_depths, w.report.n_candidates) == (40, 40, 3)


def test_both_relpose_programs_write_the_calls_pair_scales(tmp_path):
    """relpose -s on the file scene of the global poses (six views, every pair, about 150 matches each): the two programs
    write the same bytes, and the file holds what the two calls give on the same arrays"""
    written = {}
    for name, prog in PROGRAMS:
        folder = str(tmp_path / name)
        os.makedirs(folder)
        s = gs.scene_files(folder)
        r = subprocess.run(prog + ["-i", s["path"], "-m", folder, "-s", "pair_scales.json"], capture_output=True, text=True,
                           cwd=ROOT, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Pair scales: " in r.stdout
        written[name] = [open(os.path.join(folder, f), "rb").read()
                         for f in ("matches.e.txt", "relative_poses.json", "pair_scales.json")]
    assert written["cpp"] == written["py"]
    args = gs.relpose_call(s)
    rp = capi.RelPoses(**args)
    wargs = {k: v for k, v in args.items() if k != "view_wh"}
    use = relpose.scale_pairs(rp.results)
    w = capi.WedgeScales(**wargs, rel_R=rp.results["R"], rel_t=rp.results["t"], inl_off=rp.inl_off, inl_idx=rp.inl_idx,
                         use_pair=use)
    rec, lo, hi = fileio.read_pair_scales(os.path.join(folder, "pair_scales.json"))
    assert (lo, hi) == (8, 2048) and rec == relpose.scale_entries(gs.E2E_VIEW_ID, args["pairs"], w.records)
    assert use.sum() >= 10 and len(rec) >= 20
    # the ratios are those of the planted baselines, to the relative poses' accuracy: a pose is a minimal-sample model
    # that fits its inliers to precision_px = 2.5 px, 0.0036 rad at f = 700, in its rotation and in its direction; the
    # views stand 60 degrees and more apart around the cloud, a parallax of 0.5 rad at the least: 0.7 % on a pair's depths
    # from either, and a ratio has two pairs: 4 x 0.7 %
    index = {v: k for k, v in enumerate(gs.E2E_VIEW_ID)}
    err = [abs(np.log(q * np.linalg.norm(s["C_true"][index[k[0]]] - s["C_true"][index[k[1]]]) /
                      np.linalg.norm(s["C_true"][index[l[0]]] - s["C_true"][index[l[1]]]))) for _, k, l, _, q in rec]
    print("pair scales of the file scene: log error of the ratios, median %.5f, largest %.5f" % (np.median(err), max(err)))
    assert max(err) < 0.03
    # without the switch nothing of it is written
    folder = str(tmp_path / "plain")
    os.makedirs(folder)
    s = gs.scene_files(folder)
    assert relpose.main(["-i", s["path"], "-m", folder]) == 0 and not os.path.exists(os.path.join(folder, "pair_scales.json"))
    assert open(os.path.join(folder, "relative_poses.json"), "rb").read() == written["py"][1]


def test_timing_tool_on_a_short_corridor(tmp_path):
    """tools/pairscales_time.py at 40 views: the record's fields, and ratios that are the planted baselines' to the
    noise of the relative poses (0.005 rad of direction against a parallax of 0.5 d / 9 and more: a tenth per depth)"""
    import json
    out = str(tmp_path / "time.json")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pairscales_time.py"), "--views", "40", "--repeats", "1",
                        "--out", out, "--commit", "test"], capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    with open(out) as fh:
        doc = json.load(fh)
    assert (doc["views"], doc["pairs"], doc["commit"], len(doc["runs"])) == (40, 185, "test", 1)
    run = doc["runs"][0]
    assert run["n_pairs_used"] == 185 and run["n_inliers"] == doc["matches"] and run["n_depths"] > 0.99 * doc["matches"]
    assert 1000 < run["n_wedges"] <= run["n_candidates"] and run["device_ms"] > 0.0     # (pairs five steps either way share nothing)
    assert run["ratio_log_error"]["median"] < 0.1
    assert doc["global_poses_same_run"]["n_translation_pairs"] > 0
    scaled = doc["global_poses_scaled_same_run"]
    assert scaled["scale"]["n_scaled_pairs"] == scaled["n_translation_pairs"] > 0 and scaled["scale"]["scale_ms"] > 0.0
    assert scaled["n_component_views"] == 40 and scaled["centre_error"] is not None      # (recorded, not asserted)


# ---- sfmloc_global_poses_scaled ("Scaled global poses") -------------------------------------------------------------------
# The integers against the restatement; the doubles within four times what the restatement's two solvers leave between
# them, with the floor of 16 eps (tests/golden/pairscales_parity.json, the rule of test_gpu_globalposes.py).

sys.path.insert(0, os.path.join(HERE, "golden"))
from make_globalposes_fixtures import bound as bound_of  # noqa: E402
from make_pairscales_fixtures import INTS, wedges_for  # noqa: E402
from sfmlocalization_amd import globalposes, globalsfm  # noqa: E402


@pytest.fixture(scope="module")
def parity():
    import json
    with open(os.path.join(HERE, "golden", "pairscales_parity.json")) as fh:
        return json.load(fh)


@pytest.fixture(scope="module")
def scaled(scenes):
    """name -> (scene, kl, ratio, the restatement's scaled result, the device's); computed once per scene"""
    cache = {}

    def get(name):
        if name not in cache:
            s, ref = scenes[name]
            kl, ratio = wedges_for(name, s, ref)
            n = len(s["R_true"])
            twin = tw.global_poses_scaled(n, s["pairs"], s["rel_R"], s["rel_t"], kl, ratio)
            cache[name] = (s, kl, ratio, twin, capi.GlobalPoses(n, s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl, ratio)))
        return cache[name]
    return get


def scaled_ints(g):
    r, sr = g.report, g.scale_report
    return dict(n_component_views=r.n_component_views, root=r.root, n_translation_pairs=r.n_translation_pairs,
                scale_n_wedges_used=sr.n_wedges_used, scale_n_scaled_pairs=sr.n_scaled_pairs,
                scale_n_scaled_views=sr.n_scaled_views, scale_first_pair=sr.first_pair, scale_steps_tried=sr.steps_tried,
                scale_steps_accepted=sr.steps_accepted, scale_stop=sr.stop, trans_steps_tried=r.trans_steps_tried,
                trans_steps_accepted=r.trans_steps_accepted, trans_stop=r.trans_stop)


@pytest.mark.parametrize("name", list(MAKERS))
def test_scaled_call_against_the_restatement(scaled, parity, name):
    s, kl, ratio, twin, g = scaled(name)
    got = scaled_ints(g)
    assert got == {k: int(twin[k]) for k in INTS} == {k: parity[name][k] for k in INTS}
    assert np.array_equal(g.in_component, twin["in_component"]) and np.array_equal(g.pairs["used_t"] != 0, twin["used_t"])
    assert g.scale_report.n_wedges == len(kl) and g.scale_report.launches > 0 and g.scale_report.scale_ms > 0.0
    assert g.scale_report.centre_ms == g.report.translation_ms > 0.0
    bd = bound_of(dict(b=parity[name]["twin_baseline"], C=parity[name]["twin_centre"]))
    db, dC = np.max(np.abs(g.baselines - twin["baselines"])), np.max(np.abs(g.C - twin["C"]))
    print("scaled", name, "baselines", db, "of", bd["b"], "centres", dC, "of", bd["C"])
    assert db <= bd["b"] and dC <= bd["C"]
    assert np.max(np.abs(g.wedge_weights - twin["wedge_weights"])) <= 1e3 * bd["b"]    # (weights: delta / |r|, |r| >= 0.1)
    assert not g.R[~g.in_component].any() and not g.C[~g.in_component].any() and not g.baselines[g.pairs["used_t"] == 0].any()
    if name == "boundaries":      # the planted star's centre is a node of more than 64 wedges: the wave's gather; groups drop out
        deg = np.bincount(kl.reshape(-1), minlength=len(s["pairs"]))
        assert deg.max() > 64 and g.scale_report.n_wedges_used < len(kl) and g.report.n_translation_pairs < len(s["pairs"])


def test_scaled_call_twice_gives_the_same_bits(scaled):
    s, kl, ratio, _, g = scaled("boundaries")
    h = capi.GlobalPoses(len(s["R_true"]), s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl, ratio))
    assert h.C.tobytes() == g.C.tobytes() and h.baselines.tobytes() == g.baselines.tobytes()
    assert h.wedge_weights.tobytes() == g.wedge_weights.tobytes()


def test_the_corridor_keeps_its_spacing(scaled, parity):
    """The test that carries the feature: scene (b), 14 views on a line with uneven steps and one wrong direction.  The
    restatement at the committed seed (tests/golden/pairscales_parity.json): scaled 0.0158 of the extent, unscaled 0.0826,
    ratio 0.19."""
    s, kl, ratio, twin, g = scaled("corridor")
    u = capi.GlobalPoses(14, s["pairs"], s["rel_R"], s["rel_t"])
    assert u.in_component.all() and g.in_component.all()
    e_scaled = gs.errors(s, g.in_component, int(u.report.root), g.R, g.C)[1]
    e_plain = gs.errors(s, u.in_component, int(u.report.root), u.R, u.C)[1]
    print("corridor: centre error scaled", e_scaled, "unscaled", e_plain, "ratio", e_scaled / e_plain, "; restatement",
          parity["corridor"]["centre_error_scaled"], parity["corridor"]["centre_error_unscaled"])
    assert e_scaled <= 0.03
    assert e_scaled <= e_plain / 3.0
    assert e_plain > 0.05
    assert np.array_equal(g.R, u.R)                       # the rotations are the unscaled call's


def test_the_wrong_pair_is_weighed_down(scaled, parity):
    s, kl, ratio, twin, g = scaled("corridor")
    wp = s["wrong_pair"]
    rel = np.abs(g.baselines / (s["b_true"] / tw.lower_median(s["b_true"])) - 1.0)
    mine = (kl[:, 0] == wp) | (kl[:, 1] == wp)
    print("wrong pair: baseline error", rel[wp], "weights", g.wedge_weights[mine], "others at most", np.delete(rel, wp).max())
    assert rel[wp] > parity["corridor"]["other_baseline_error"]              # off: its depths come from a wrong direction
    down = g.wedge_weights < 1.0                           # weighed down: wedges of the wrong pair, and only such
    assert np.array_equal(down, twin["wedge_weights"] < 1.0) and down.sum() >= 2 and mine[down].all()
    assert (g.wedge_weights > 0.0).all()
    assert np.delete(rel, wp).max() <= parity["corridor"]["other_baseline_error"] * (1.0 + 1e-6)
    assert abs(rel[wp] - parity["corridor"]["wrong_pair_baseline_error"]) < 1e-6


def test_scaled_call_without_wedges_and_empty(scaled):
    s, kl, ratio, _, _ = scaled("corridor")
    n, none = 14, (np.zeros((0, 2), np.uint32), np.zeros(0))
    for wedges in (none, (kl, np.full(len(kl), np.nan)), (kl[:1], -ratio[:1])):      # no wedge, none usable
        g = capi.GlobalPoses(n, s["pairs"], s["rel_R"], s["rel_t"], wedges=wedges)
        assert not g.in_component.any() and not g.R.any() and not g.C.any() and not g.baselines.any()
        assert not g.pairs["used_t"].any() and g.pairs["kept"].all()
        assert (g.report.n_component_views, g.report.n_translation_pairs, g.report.n_rotation_pairs) == (0, 0, 36)
        assert (g.scale_report.n_wedges, g.scale_report.n_wedges_used, g.scale_report.n_scaled_pairs) == (len(wedges[1]), 0, 0)
        assert g.report.rot_steps_tried > 0
    g = capi.GlobalPoses(5, np.zeros((0, 2)), np.zeros((0, 3, 3)), np.zeros((0, 3)), wedges=none)
    assert not g.in_component.any() and len(g.baselines) == 0 and g.report.launches == 0 and g.scale_report.n_wedges == 0
    # a wedge list that leaves pairs out: they drop out of the translations, and a view only they reach with them
    keep = ~((kl[:, 0] == 0) | (kl[:, 1] == 0) | (kl[:, 0] == 1) | (kl[:, 1] == 1))          # pairs (0, 1) and (0, 2)
    g = capi.GlobalPoses(n, s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl[keep], ratio[keep]))
    assert s["pairs"][:3].tolist() == [[0, 1], [0, 2], [0, 3]]
    assert g.pairs["used_t"][:3].tolist() == [0, 0, 1] and g.report.n_translation_pairs == 34 and g.in_component.all()
    keep = ~np.isin(kl, [0, 1, 2]).any(1)
    g = capi.GlobalPoses(n, s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl[keep], ratio[keep]))
    assert not g.in_component[0] and g.in_component[1:].all() and (g.report.root, g.scale_report.n_scaled_views) == (1, 13)
    assert not g.R[0].any() and g.scale_report.first_pair == 3


def test_scaled_call_refusals_come_before_any_launch(scaled):
    s, kl, ratio, _, _ = scaled("corridor")
    P = len(s["pairs"])

    def refused(kl, ratio, text, **kw):
        with pytest.raises(capi.SfmlocError) as e:
            capi.GlobalPoses(14, s["pairs"], s["rel_R"], s["rel_t"], wedges=(kl, ratio), **kw)
        assert text in e.value.message, e.value.message
    refused([[0, P]], [1.0], "out of range")
    refused([[1, 0]], [1.0], "k must be below l")
    refused([[2, 2]], [1.0], "k must be below l")
    refused([[0, 1], [1, 2], [0, 1]], [1.0, 1.0, 2.0], "listed twice")
    far = int(np.nonzero((s["pairs"][:, 0] > 5))[0][0])
    refused([[0, far]], [1.0], "share no view")
    refused(kl, ratio, "scale_delta", scale=dict(scale_delta=0.0))
    refused(kl, ratio, "max_pcg", scale=dict(max_pcg=0))
    bad = s["rel_R"].copy()
    bad[3, 0, 0] = np.nan
    with pytest.raises(capi.SfmlocError):                                      # the unscaled call's refusals still hold
        capi.GlobalPoses(14, s["pairs"], bad, s["rel_t"], wedges=(kl, ratio))


GP_PROGRAMS = [("cpp", [os.path.join(ROOT, "sfmlocalization_amd", "bin", globalposes.NAME)]),
               ("py", [sys.executable, "-m", "sfmlocalization_amd.globalposes"])]


def test_both_globalposes_programs_write_the_same_bytes_with_scales(tmp_path):
    import json
    folder = str(tmp_path)
    s = gs.scene_files(folder)
    assert relpose.main(["-i", s["path"], "-m", folder, "-s", "pair_scales.json"]) == 0
    written = {}
    for name, prog in GP_PROGRAMS:
        out, rep = str(tmp_path / f"{name}.json"), str(tmp_path / f"{name}_report.json")
        r = subprocess.run(prog + ["-i", s["path"], "-p", os.path.join(folder, "relative_poses.json"), "-o", out, "-r", rep,
                                   "-s", os.path.join(folder, "pair_scales.json")], capture_output=True, text=True, cwd=ROOT,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        assert "Pair scales: " in r.stdout
        doc = json.load(open(rep))
        written[name] = (open(out, "rb").read(), doc)
    assert written["cpp"][0] == written["py"][0]
    a, b = written["cpp"][1], written["py"][1]
    assert list(a) == list(b) == list(globalposes.REPORT_FIELDS) + ["scale", "baselines"]
    assert list(a["scale"]) == list(b["scale"]) == list(globalposes.SCALE_REPORT_FIELDS)
    timed = {"graph_ms", "rotation_ms", "translation_ms", "device_ms"}
    assert {k: v for k, v in a.items() if k not in timed | {"scale"}} == {k: v for k, v in b.items() if k not in timed | {"scale"}}
    assert {k: v for k, v in a["scale"].items() if not k.endswith("_ms")} == {k: v for k, v in b["scale"].items() if not k.endswith("_ms")}
    assert a["scale"]["n_scaled_views"] == 6 and a["scale"]["n_wedges_used"] >= 20 and len(a["baselines"]) == 15
    # the baselines are the planted ones in the median's unit, to the ratios' accuracy (see the relpose test above: 3 %)
    entries = json.load(open(os.path.join(folder, "relative_poses.json")))["relative_poses"]
    index = {v: k for k, v in enumerate(gs.E2E_VIEW_ID)}
    bt = np.array([np.linalg.norm(s["C_true"][index[e["I"]]] - s["C_true"][index[e["J"]]]) for e in entries])
    used = np.array(a["baselines"]) > 0
    rel = np.abs(np.array(a["baselines"])[used] / (bt[used] / tw.lower_median(bt[used])) - 1.0)
    print("file scene: baseline errors", rel.max())
    assert used.sum() >= 10 and rel.max() < 0.03
    # an unknown pair in the scales file: both refuse
    rec, lo, hi = fileio.read_pair_scales(os.path.join(folder, "pair_scales.json"))
    fileio.write_pair_scales(str(tmp_path / "bad.json"), [(rec[0][0], (98, 99), rec[0][2], rec[0][3], rec[0][4])], lo, hi)
    for name, prog in GP_PROGRAMS:
        r = subprocess.run(prog + ["-i", s["path"], "-p", os.path.join(folder, "relative_poses.json"), "-o",
                                   str(tmp_path / "x.json"), "-s", str(tmp_path / "bad.json")], capture_output=True, text=True,
                           cwd=ROOT, timeout=300)
        assert r.returncode == 1 and "Invalid pair scales file." in r.stderr


def test_globalsfm_with_pair_scales_end_to_end(tmp_path):
    """globalsfm --pair-scales on the planted six views, inside the bound of
    test_gpu_globalposes.py::test_end_to_end_from_features_and_matches"""
    import json
    with open(os.path.join(HERE, "golden", "globalposes", "expected.json")) as fh:
        chain = json.load(fh)["chain"]
    s = gs.scene_files(str(tmp_path))
    lines = []
    assert globalsfm.run(s["path"], str(tmp_path), str(tmp_path / "out"), log=lines.append, pair_scales=True) == 0
    assert os.path.exists(tmp_path / "out" / "pair_scales.json") and any(l.startswith("Pair scales: ") for l in lines)
    out = json.loads((tmp_path / "out" / "sfm_data.json").read_text())
    assert [e["key"] for e in out["extrinsics"]] == gs.E2E_VIEW_ID and len(out["structure"]) > 100
    R = np.array([e["value"]["rotation"] for e in out["extrinsics"]])
    C = np.array([e["value"]["center"] for e in out["extrinsics"]])
    rot, cen = gs.errors(s, np.ones(6, bool), 0, R @ R[0].T, C)
    print("end to end with pair scales: rotation", rot, "deg, centre", cen, "of the extent; the CPU chain's:", chain)
    assert cen <= chain["centre"] + bound_of(chain["parity"])["C"]
