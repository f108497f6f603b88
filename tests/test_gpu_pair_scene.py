"""GPU: the three two-view calls and the tracks on ONE small scene built so that a swapped or stale pointer of the
scene they share (csrc/pair_scene.h, PairDev of csrc/twoview_device.h) lands somewhere else: three views of 50, 70 and
90 features (a wrong view_off row is another view's), view 1 on a radial intrinsic and the others on a pinhole of another
focal length, the pairs listed as (2, 0), (0, 1), (1, 2) -- the first with I > J -- with 40 planted matches each whose
two feature indices always differ.  RelPoses, then RelRefine on its results, then WedgeScales on the refined poses, and
Tracks, each against its NumPy restatement bit for bit; RelRefine and WedgeScales once more with use_pair = [1, 0, 1].
(Neither of the two takes a view_wh: every call of theirs here is one without it.)"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import pairscales_np  # noqa: E402
import relpose_np  # noqa: E402
import relrefine_cases as cases  # noqa: E402
import relrefine_np  # noqa: E402
import structure_np  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu

N_FEAT = (50, 70, 90)
SHIFT = (0, 7, 13)                      # view v keeps point p at feature (p + SHIFT[v]) % N_FEAT[v]
PAIRS = ((2, 0), (0, 1), (1, 2))
W, H = 640, 480
INTRINSICS = np.array([[520.0, 322.0, 238.0, 0.0, 0.0, 0.0], [610.0, 316.0, 243.0, -0.12, 0.03, 0.0]])
ITER = 64                               # AC-RANSAC iterations: every match is planted, the first rounds find the pose


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).reshape(-1).view(np.uint64)


def make_call(seed=7):
    """-> the keyword arguments of capi.RelPoses / relpose_np.relative_poses"""
    rng = np.random.default_rng(seed)
    X = rng.uniform([-2.0, -1.5, 5.0], [2.0, 1.5, 9.0], (max(N_FEAT), 3))
    C = np.array([[0.0, 0.0, 0.0], [1.0, 0.1, 0.0], [-0.9, -0.1, 0.2]])
    view_intrinsic = np.array([0, 1, 0], np.uint32)
    feats = []
    for v, n in enumerate(N_FEAT):
        f, ppx, ppy, k1, k2, k3 = INTRINSICS[view_intrinsic[v]]
        Xc = X[:n] - C[v]                                   # (every camera looks down +z)
        p = Xc[:, :2] / Xc[:, 2:]
        r2 = (p * p).sum(1, keepdims=True)
        px = f * p * (1.0 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3) + np.array([ppx, ppy]) + rng.normal(size=(n, 2)) * 0.2
        at = (np.arange(n) + SHIFT[v]) % n
        feat = np.zeros((n, 2), np.float32)
        feat[at] = px
        feats.append(feat)
    mi, mj, offsets = [], [], [0]
    for a, b in PAIRS:
        pts = rng.permutation(min(N_FEAT[a], N_FEAT[b]))[:40]
        mi += ((pts + SHIFT[a]) % N_FEAT[a]).tolist()
        mj += ((pts + SHIFT[b]) % N_FEAT[b]).tolist()
        offsets.append(len(mi))
    assert all(i != j for i, j in zip(mi, mj))
    return dict(view_off=np.concatenate([[0], np.cumsum(N_FEAT)]).astype(np.uint64), kpt_xy=np.concatenate(feats),
                view_wh=np.tile(np.array([W, H], np.uint32), (3, 1)), view_intrinsic=view_intrinsic, intrinsics=INTRINSICS,
                intrinsic_type=np.array([0, 3], np.uint32), pairs=np.array(PAIRS, np.uint32),
                offsets=np.array(offsets, np.uint64), match_i=np.array(mi, np.uint32), match_j=np.array(mj, np.uint32))


def refined_call(call, results):
    """the wedge scales' call: the refinement's pose where there is one (results: records or the twin's list)"""
    R, t = np.array(call["rel_R"], np.float64).reshape(-1, 9), np.array(call["rel_t"], np.float64).reshape(-1, 3)
    for k, r in enumerate(results):
        if int(r["status"]) in (1, 3):
            R[k], t[k] = np.asarray(r["R"], np.float64).reshape(9), np.asarray(r["t"], np.float64).reshape(3)
    return dict(call, rel_R=R, rel_t=t)


def wscale_records(ref):
    rec = np.zeros(len(ref), capi.WSCALE)
    for i, r in enumerate(ref):
        rec[i] = r
    return rec


@pytest.fixture(scope="module")
def twin():
    """the restatements' chain on the scene, for every pair and for use_pair = [1, 0, 1]: computed once, left unchanged"""
    args = make_call()
    poses = relpose_np.relative_poses(**args, max_iteration=ITER)
    call = cases.call_from_twin(args, poses)
    out = {"args": args, "poses": poses, "call": call}
    for tag, use in (("all", call["use_pair"]), ("101", np.array([1, 0, 1], np.uint8))):
        c = dict(call, use_pair=use)
        fine = relrefine_np.refine_relative_poses(**c)
        out[tag] = {"call": c, "fine": fine, "wedges": pairscales_np.wedge_scales(**refined_call(c, fine))}
    return out


def test_relative_poses_are_the_twins_bits(twin):
    got = capi.RelPoses(**twin["args"], max_iteration=ITER)
    for k, want in enumerate(twin["poses"]):
        for f in ("ok", "n_matches", "n_inliers", "sample", "front", "choice"):
            assert np.array_equal(np.asarray(got.results[k][f], np.int64).ravel(), np.asarray(want[f], np.int64).ravel()), (k, f)
        for f in ("E", "R", "t", "error_max_px", "nfa"):
            assert np.array_equal(bits(got.results[k][f]), bits(want[f])), (k, f)
        assert np.array_equal(got.inliers(k).astype(np.int64), want["inliers"]), k
    assert got.results["ok"].tolist() == [1, 1, 1] and got.results["n_matches"].tolist() == [40, 40, 40]
    # the next calls are fed from the device's results: they are the twin's, array for array
    call = cases.call_from_device(twin["args"], got)
    for f in ("rel_R", "rel_t", "inl_off", "inl_idx", "use_pair"):
        assert np.asarray(call[f]).tobytes() == np.asarray(twin["call"][f]).tobytes(), f


@pytest.mark.parametrize("tag", ["all", "101"])
def test_refinement_and_wedge_scales_are_the_twins_bits(twin, tag):
    t = twin[tag]
    fine = capi.RelRefine(**t["call"])
    assert cases.same_bits(fine.results, t["fine"]) == []
    want_status = [int(r["status"]) for r in t["fine"]]
    assert all(s in (1, 3) for s in want_status) if tag == "all" else want_status[1] == 0 and want_status[0] in (1, 3)
    w = capi.WedgeScales(**refined_call(t["call"], fine.results))
    want = wscale_records(t["wedges"]["records"])
    assert len(w.records) == len(want) == (3 if tag == "all" else 1)
    for f in ("view", "k", "l", "n_shared"):
        assert np.array_equal(w.records[f], want[f]), f
    assert np.array_equal(bits(w.records["ratio"]), bits(want["ratio"]))
    rep = w.report
    assert (rep.n_pairs, rep.n_pairs_used) == (3, 3 if tag == "all" else 2)
    assert (rep.n_depths, rep.n_candidates) == (t["wedges"]["n_depths"], t["wedges"]["n_candidates"])


def test_tracks_equal_the_twin(twin):
    a = twin["args"]
    pl = (a["pairs"], a["offsets"], a["match_i"], a["match_j"])
    use = np.array([1, 1, 1], np.uint8)
    for view_use in (None, use):
        got, want = capi.Tracks(a["view_off"], *pl, view_use=view_use), structure_np.tracks(a["view_off"], *pl, view_use=view_use)
        assert got.counts == want["counts"] and got.n_tracks > 40
        for f in ("off", "view", "feat"):
            np.testing.assert_array_equal(getattr(got, f), want[f])
