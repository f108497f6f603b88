"""GPU: K9 AKAZE + M-LDB at the sizes and octave settings where csrc/akaze.hip changes form or fills a table
(akaze_cases.py; test_akaze_cases_cpu.py asserts that each case is on its side of its boundary): always the CPU
restatement's scale space, keypoints and descriptors, bit for bit."""
import numpy as np
import pytest

import akaze_cases as A
import sfmlocalization_amd as S
from akaze_compare import assert_extraction_matches_oracle, assert_outputs_equal, bits32
from sfmlocalization_amd import capi

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.name)
def test_case_matches_oracle(oracle_c, c):
    g = c.image()
    ak = S.Akaze(c.w, c.h, n_octaves=c.n_octaves, n_sublevels=c.n_sublevels, threshold=c.threshold)
    try:
        assert len(ak.levels) == c.levels
        kp, _ = assert_extraction_matches_oracle(oracle_c, ak, g, c.threshold, c.n_octaves, c.n_sublevels, what=c.name)
        assert c.kp[0] <= len(kp) <= c.kp[1]
        if c.kp == A.NONE:
            assert ak.suppress_stats()["keypoints"] == 0
        if c.name in ("constant", "thres10"):
            assert ak.suppress_stats()["candidates"] == 0
    finally:
        ak.close()


@pytest.mark.parametrize("name", ["80x4096", "16384x64"])
def test_largest_frames_decided_by_band_scans(oracle_c, name, monkeypatch):
    """k_suppress reads its row-start tables (4 097 entries: rows 0 .. h of the tallest frame) only for a candidate whose
    neighbour lists spilled, which no frame does by itself: every candidate of the tallest and of the widest frame spilled
    (SFMLOC_AKAZE_SUPPRESS, read when the extractor is made) -- the same keypoints"""
    monkeypatch.setenv("SFMLOC_AKAZE_SUPPRESS", "spill")
    c = A.BY_NAME[name]
    ak = S.Akaze(c.w, c.h)
    try:
        kp, _ = assert_extraction_matches_oracle(oracle_c, ak, c.image(), what=name + " spilled")
        st = ak.suppress_stats()
        assert st["spilled_ap"] == st["spilled_n"] == st["candidates"] >= len(kp) > 500
    finally:
        ak.close()


@pytest.mark.parametrize("name", ["128x100", "160x80"])
def test_batches_of_small_frames_equal_one_at_a_time(name):
    """three frames per call at the sizes whose octaves are evolved in LDS (k_octave_resident in its gang form: octave 0 at
    128 x 100, octaves 0 and 1 at 160 x 80): keypoints, descriptors and scale space as from separate calls; the resident
    outputs' counts as the downloaded ones"""
    c = A.BY_NAME[name]
    assert all(r for _, r in c.resident)
    imgs = [A.blocks(50 + k, c.w, c.h, 4 + k) for k in range(3)]
    one = S.Akaze(c.w, c.h)
    exs = [S.Akaze(c.w, c.h) for _ in range(3)]
    try:
        ref, ref_levels = [], []
        for g in imgs:
            ref.append(one.detect_and_compute(g))
            ref_levels.append(one.read_levels())
        assert sum(len(kp) for kp, _ in ref) > 30
        got = S.Akaze.detect_and_compute_batch(exs, imgs)
        for e, (kp, d), (rkp, rd), (rldet, rlt) in zip(exs, got, ref, ref_levels):
            assert len(kp) == len(rkp)
            np.testing.assert_array_equal(bits32(kp), bits32(rkp))
            np.testing.assert_array_equal(d, rd)
            ldet, lt = e.read_levels()
            np.testing.assert_array_equal(bits32(lt), bits32(rlt))
            np.testing.assert_array_equal(bits32(ldet), bits32(rldet))
        ns = S.Akaze.detect_resident_batch(exs, imgs[::-1])
        assert list(ns) == [len(kp) for kp, _ in ref[::-1]]
    finally:
        for e in exs + [one]:
            e.close()


def test_output_paths_of_one_extractor(oracle_c):
    """sfmloc_akaze_detect_and_compute serves a call out of the speculative download (n <= spec_n, which follows the last
    count between 256 and 4 096) or with a second copy: one extractor through no keypoint, a few, more than spec_n, more
    than spec_n can become, a few again (test_akaze_cases_cpu.py asserts those counts) -- every call the restatement's
    outputs; then a caller buffer below the count (ECAP), and the same frame with room again"""
    p = A.PATH_PARAMS
    ak = S.Akaze(A.PATH_W, A.PATH_H, **p)
    try:
        counts = []
        for name, image, (lo, hi) in A.PATH_SEQUENCE:
            kp, _ = assert_extraction_matches_oracle(oracle_c, ak, image(), p["threshold"], p["n_octaves"], p["n_sublevels"],
                                                     what=name)
            assert lo <= len(kp) <= hi, name
            counts.append(len(kp))
        assert counts[1] == counts[4] and counts[0] == 0
        g = A.PATH_SEQUENCE[2][1]()
        ekp, edesc = oracle_c.akaze_detect_and_compute(g, p["threshold"], p["n_octaves"], p["n_sublevels"], cap=65536)
        for cap in (len(ekp) - 1, 200, 1):  # just below the count; below the speculative size too; one row
            with pytest.raises(S.SfmlocError) as ei:
                ak.detect_and_compute(g, cap=cap)
            assert ei.value.code == capi.ECAP and f"{len(ekp)} keypoints" in ei.value.message
        kp, desc = ak.detect_and_compute(g, cap=len(ekp))  # exactly enough room
        assert_outputs_equal(kp, desc, ekp, edesc, "cap == n")
        kp, desc = ak.detect_and_compute(g)
        assert_outputs_equal(kp, desc, ekp, edesc, "after ECAP")
    finally:
        ak.close()


def test_dense_compute_with_other_octave_settings(oracle_c):
    """the description-only path (sfmloc_akaze_compute) on a plan of two octaves of two sub-levels: a grid of keypoints on
    every level, angles and descriptors the restatement's"""
    g = A.blocks(8, 300, 300, 6)
    ak = S.Akaze(300, 300, n_octaves=2, n_sublevels=2)
    try:
        kin = A.dense_keypoints(ak.levels, 300, 300)
        assert sorted(set(kin[:, 3].astype(int))) == [0, 1, 2, 3] == list(range(len(ak.levels)))
        desc, ang = ak.compute(g, kin)
        edesc, eang = oracle_c.akaze_compute(g, kin, omax=2, nsub=2)
        np.testing.assert_array_equal(bits32(ang), bits32(eang))
        np.testing.assert_array_equal(desc[:, :61], edesc)
        assert (desc[:, 61:] == 0).all() and len(np.unique(ang)) > 100
        # only the lowest level asked for: nothing above it is built, the same bits
        low = kin[kin[:, 3] == 0]
        desc0, ang0 = ak.compute(g, low)
        np.testing.assert_array_equal(bits32(ang0), bits32(eang[kin[:, 3] == 0]))
        np.testing.assert_array_equal(desc0[:, :61], edesc[kin[:, 3] == 0])
    finally:
        ak.close()


@pytest.mark.parametrize("n", A.NEED_CASES, ids=lambda n: n.name)
def test_dense_compute_cut_short_and_whole(oracle_c, n):
    """a description-only call builds no level above its keypoints' highest, and an octave's run cut short can change form
    (test_akaze_cases_cpu.py::test_need_cases_change_the_run: a resident run of 2 instead of 4; a resident run of 8
    instead of nine levels by the per-level kernels): one extractor, first cut short, then whole -- the restatement's
    angles and descriptors both times"""
    g = A.blocks(9, n.w, n.h, 5)
    ak = S.Akaze(n.w, n.h, n_octaves=n.n_octaves, n_sublevels=n.n_sublevels)
    try:
        kin = A.dense_keypoints(ak.levels, n.w, n.h)
        edesc, eang = oracle_c.akaze_compute(g, kin, omax=n.n_octaves, nsub=n.n_sublevels)
        assert n.need < len(ak.levels) and len(np.unique(eang)) > 100
        for top in (n.need, len(ak.levels)):
            sel = kin[:, 3] < top
            assert sorted(set(kin[sel, 3].astype(int))) == list(range(top))
            desc, ang = ak.compute(g, kin[sel])
            np.testing.assert_array_equal(bits32(ang), bits32(eang[sel]), err_msg=f"levels 0 .. {top - 1}")
            np.testing.assert_array_equal(desc[:, :61], edesc[sel], err_msg=f"levels 0 .. {top - 1}")
            assert (desc[:, 61:] == 0).all()
    finally:
        ak.close()


def test_long_fed_schedule_is_refused():
    """a level whose FED cycle has more than 64 steps does not fit the plan's tables (nor the device's): refused at
    creation, with the level and its step count in the text; 57 steps are fine"""
    with pytest.raises(S.SfmlocError) as ei:
        S.Akaze(2560, 1280, n_octaves=6)
    assert ei.value.code == capi.EINVAL
    assert "68 diffusion steps at level 20" in ei.value.message
    with pytest.raises(S.SfmlocError) as ei:
        S.Akaze(2560, 1280, n_octaves=6, n_sublevels=1)
    assert ei.value.code == capi.EINVAL and "109 diffusion steps at level 5" in ei.value.message
    ak = S.Akaze(2560, 1280, n_octaves=5)
    assert len(ak.levels) == 20
    ak.close()


def test_candidate_overflow_is_reported_and_survived(oracle_c):
    """More extrema than the candidate workspace (65 536) holds: ECAP, nothing written past an array (every consumer of the
    count clamps: DESIGN.md), and the extractor then gives the restatement's bits on an ordinary frame.  The restatement
    finds 73 871 KEYPOINTS on the overflow frame (A.OVERFLOW_KEYPOINTS; 14 s on a CPU core, not recomputed here), and
    keypoints are a subset of the candidates."""
    p = A.OVERFLOW_PARAMS
    ak = S.Akaze(A.OVERFLOW_W, A.OVERFLOW_H, **p)
    try:
        g = A.overflow_image()
        with pytest.raises(S.SfmlocError) as ei:
            ak.detect_and_compute(g)
        assert ei.value.code == capi.ECAP and "candidates exceed the workspace" in ei.value.message
        assert ak.suppress_stats()["candidates"] > A.OVERFLOW_KEYPOINTS > A.CAND_CAP
        with pytest.raises(S.SfmlocError) as ei:
            ak.detect_resident(g)
        assert ei.value.code == capi.ECAP
        assert_extraction_matches_oracle(oracle_c, ak, A.overflow_ordinary_image(), p["threshold"], p["n_octaves"],
                                         p["n_sublevels"], what="after the overflow")
    finally:
        ak.close()
