"""The resident sfm_data as every map-side stage sees it through one struct built from the handle at each use
(csrc/sfm_data.h: SfmDev, sfm_dev): the per-view lists after the transpose's sort left them in either buffer, the keep
masks null and then set on one handle, and one handle taken through every stage in turn.  References are the numpy
twins, or this library on other handles: bits are compared, there is no tolerance."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import adjust_ba_scene as BS  # noqa: E402
import adjust_scene as AS  # noqa: E402
import colorize_np as CN  # noqa: E402
import register_scene as RS  # noqa: E402
from sfmlocalization_amd import adjust  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402
from test_gpu_register import bits, compare_all, twin_of  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oc():
    from oracle import oracle_c
    oracle_c.build()
    return oracle_c


@pytest.mark.parametrize("n_views,key_bits", [(256, 8), (257, 9)])
def test_lists_after_the_sorts_swap(oc, n_views, key_bits):
    """one radix pass leaves the sorted lists in the sort's scratch buffer (the handle swaps the two), two passes in the
    buffer they started in: the colouring plan and the growth step read vlist and view_off in both cases"""
    a = AS.sparse_views_case(n_views)
    assert AS.radix_key_bits(n_views - 1) == key_bits
    h = S.Sfm(**a)
    try:
        ran, ok = h.resect()
        assert ran >= 3 and ok >= 3 and h.resect_read()[n_views - 1].ok
        order, lm_iter, lm_obs = h.color_plan()
        e_order, e_iter, e_obs = CN.plan(n_views, a["obs_off"], a["obs_view"])
        np.testing.assert_array_equal(order, e_order)
        np.testing.assert_array_equal(lm_iter, e_iter)
        np.testing.assert_array_equal(lm_obs, e_obs)
    finally:
        h.close()
    # the last view (index 256 is the one the second pass's bit parts from the rest) without its pose
    b = dict(a)
    b["pose_valid"] = a["pose_valid"].copy()
    b["pose_valid"][a["view_pose"][n_views - 1]] = 0
    t, tw = twin_of(b, oc)
    # (256 views: two views with many observations are left, 10 landmarks are kept and the view is not tried -- its
    # compacted list is counted all the same; 257: 176 kept landmarks, 91 correspondences, the view registers)
    assert tw["report"]["views_unposed_in"] == 1 and tw["report"]["views_registered"] == (n_views == 257)
    h = S.Sfm(**b)
    try:
        h.triangulate()
        compare_all(h, h.register(), tw)
    finally:
        h.close()


def test_masks_null_then_set_on_one_handle():
    """before any cleanup every observation enters (the masks are null) and LM_DROPPED, 150 px off, moves; after the
    first cleanup dropped it the same call leaves it where it is"""
    a = adjust.sfm_arrays(BS.make_doc()[0])[0]
    h = S.Sfm(**a)
    try:
        rep0 = h.adjust(8)
        X0 = h.read_structure().copy()
        assert rep0.n_blocks == len(a["landmark_id"])
        assert (X0[BS.LM_DROPPED] != a["landmark_X"][BS.LM_DROPPED]).any()
        h.clean(*BS.FIRST_CLEAN, False)
        assert not h.read()["landmark_keep"][BS.LM_DROPPED]
        rep1 = h.adjust(8)
        X1 = h.read_structure()
        assert rep1.n_blocks == len(a["landmark_id"]) - 1
        np.testing.assert_array_equal(bits(X1[BS.LM_DROPPED]), bits(X0[BS.LM_DROPPED]))
        p = h.read(masks=False)                                 # the poses keep their bits
        np.testing.assert_array_equal(bits(p["pose_R"].reshape(-1, 9)), bits(a["pose_R"]))
        np.testing.assert_array_equal(bits(p["pose_C"]), bits(a["pose_C"]))
    finally:
        h.close()


STAGES = (("triangulate", lambda h: h.triangulate()),
          ("clean", lambda h: h.clean(4.0, 2.0, False)),
          ("adjust structure", lambda h: h.adjust(S.BA_STRUCTURE)),
          ("adjust joint rst", lambda h: h.adjust_joint(S.BA_ROTATION | S.BA_TRANSLATION | S.BA_STRUCTURE)),
          ("register", lambda h: h.register()),
          ("colour plan", lambda h: h.color_plan()))


def state(h):
    p = h.read(masks=True)
    return [p["pose_valid"], bits(p["pose_R"]), bits(p["pose_C"]), p["obs_keep"], p["landmark_keep"],
            bits(h.read_structure()), bits(h.read_intrinsics())]


def report(r):
    if isinstance(r, (list, tuple)):
        return [np.asarray(x) for x in r]
    return [np.array([getattr(r, f) for f, _ in r._fields_ if f != "device_ms"])]


def test_one_handle_through_every_stage():
    """triangulate, clean, adjust structure, adjust joint, register and the colouring plan on one handle give what each
    stage gives on a handle of its own.  The C ABI takes no keep masks, so a stage's own handle cannot be made from the
    previous stage's read-back alone: it is a fresh handle that is first brought to that read-back (the earlier stages,
    checked against it array for array) and then runs the stage."""
    a = RS.make_scene_a()["arrays"]
    one = S.Sfm(**a)
    try:
        for k, (name, stage) in enumerate(STAGES):
            before = state(one) if k else None
            got = report(stage(one)) + state(one)
            own = S.Sfm(**a)
            try:
                for _, earlier in STAGES[:k]:
                    earlier(own)
                if k:
                    for x, y in zip(state(own), before):
                        np.testing.assert_array_equal(x, y, err_msg="before " + name)
                want = report(stage(own)) + state(own)
            finally:
                own.close()
            assert len(got) == len(want)
            for x, y in zip(got, want):
                np.testing.assert_array_equal(x, y, err_msg=name)
        res, rnd = one.register_read()
        assert (rnd[8:12] >= 0).all() and all(res[v].ok for v in range(8, 12))    # the growth step did register views
    finally:
        one.close()
