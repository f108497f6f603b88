"""CPU: every case of akaze_cases.py is what it says it is -- the number of levels, which octaves are evolved in LDS and
in runs of what length, the side of the segment scan's one-launch limit, the side of the output paths' keypoint counts,
keypoints at the far edge -- by the CPU restatement alone (oracle_c.akaze_levels / akaze_detect_and_compute).  These are
conditions on the inputs, not measurements of the library: test_gpu_akaze_shapes.py runs the same cases on the device,
and a case that drifted off its boundary would leave a kernel form untested with everything green."""
import numpy as np
import pytest

import akaze_cases as A


def detect(oracle_c, c):
    return oracle_c.akaze_detect_and_compute(c.image(), c.threshold, c.n_octaves, c.n_sublevels, cap=A.CAND_CAP)[0]


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.name)
def test_case_is_what_it_is_for(oracle_c, c):
    g = c.image()
    assert g.shape == (c.h, c.w) and g.dtype == np.uint8
    assert 16 <= c.w <= 16384 and 16 <= c.h <= 4096 and 1 <= c.n_octaves <= 8 and c.n_octaves * c.n_sublevels <= 32
    levels = oracle_c.akaze_levels(c.w, c.h, c.n_octaves, c.n_sublevels)
    assert len(levels) == c.levels, c.what
    assert A.resident_plan(levels) == c.resident, c.what
    n_seg = A.n_seg(levels, c.w)
    assert {"<": n_seg < A.SCAN_ONE_LAUNCH, "==": n_seg == A.SCAN_ONE_LAUNCH, ">": n_seg > A.SCAN_ONE_LAUNCH}[c.seg], n_seg
    kp = detect(oracle_c, c)
    assert c.kp[0] <= len(kp) <= c.kp[1], (len(kp), c.what)
    if c.edge == "rows":
        assert (kp[:, 1] >= c.h - 64).any(), float(kp[:, 1].max())
    if c.edge == "cols":
        assert (kp[:, 0] >= c.w - 64).any(), float(kp[:, 0].max())
    if len(kp):  # every level the plan has is a level a keypoint can name
        assert 0 <= kp[:, 5].min() and kp[:, 5].max() < c.levels


def test_table_covers_the_boundaries():
    """each boundary has a case on either side of it"""
    by = A.BY_NAME
    res = {n: [r for _, r in by[n].resident] for n in by}
    runs = {n: [r for r, _ in by[n].resident] for n in by}
    # octave 0 in LDS: the last size that is, the first that is not; its longest run and one more
    assert 3 * 128 * 100 * 4 == A.LDS_BYTES and res["128x100"] == [True] and res["129x100"] == [False]
    assert (runs["o1s9"], res["o1s9"]) == ([A.RUN_MAX], [True]) and (runs["o1s10"], res["o1s10"]) == ([A.RUN_MAX + 1], [False])
    # a later octave of exactly that size: its longest run and one more
    assert (runs["o2s8_lds"][1], res["o2s8_lds"][1]) == (A.RUN_MAX, True)
    assert (runs["o2s9_lds"][1], res["o2s9_lds"][1]) == (A.RUN_MAX + 1, False)
    # the level table: one level, and all of them (in one octave, and in two)
    assert by["o1s1"].levels == 1 and by["o1s32"].levels == by["o2s16"].levels == A.MAX_LEVELS
    assert by["o2s1"].n_sublevels == by["o3s1"].n_sublevels == 1
    # the octave cut
    assert by["160x80"].levels == 8 and by["159x80"].levels == by["160x79"].levels == 4
    assert by["o8_small"].n_octaves == 8 and by["o8_small"].levels == 2 * by["o8_small"].n_sublevels
    # the size limits, the scan boundary
    assert {by["16x4096"].h, by["80x4096"].h, by["160x4096"].h} == {4096} and by["16384x64"].w == 16384
    assert [by[n].seg for n in ("16384x64", "16384x65", "1024x544", "1024x548")] == ["==", ">", "<", ">"]
    # nothing found, and nothing even proposed
    assert by["thres10"].kp == by["constant"].kp == by["16x16"].kp == (0, 0)


def test_output_path_sequence_counts(oracle_c):
    """one extractor across the output paths: none, a few, more than the first speculative size, more than its cap, a few"""
    want = [(0, 0), (1, 256), (513, A.SPEC_MAX), (A.SPEC_MAX + 1, A.CAND_CAP), (1, 256)]
    assert [r for _, _, r in A.PATH_SEQUENCE] == want
    p = A.PATH_PARAMS
    for name, image, (lo, hi) in A.PATH_SEQUENCE:
        g = image()
        assert g.shape == (A.PATH_H, A.PATH_W)
        n = len(oracle_c.akaze_detect_and_compute(g, p["threshold"], p["n_octaves"], p["n_sublevels"], cap=A.CAND_CAP)[0])
        assert lo <= n <= hi, (name, n)


def test_overflow_frame_and_its_ordinary_twin(oracle_c):
    """the frame of the candidate overflow is counted by hand (A.OVERFLOW_KEYPOINTS: 14 s here); its ordinary twin, which the
    same extractor takes afterwards, fits every buffer"""
    assert A.OVERFLOW_KEYPOINTS > A.CAND_CAP
    assert A.overflow_image().shape == A.overflow_ordinary_image().shape == (A.OVERFLOW_H, A.OVERFLOW_W)
    p = A.OVERFLOW_PARAMS
    n = len(oracle_c.akaze_detect_and_compute(A.overflow_ordinary_image(), p["threshold"], p["n_octaves"], p["n_sublevels"],
                                              cap=A.CAND_CAP)[0])
    assert A.SPEC_MAX < n < A.CAND_CAP // 4, n


def test_dense_keypoints_span_every_level(oracle_c):
    levels = oracle_c.akaze_levels(300, 300, 2, 2)
    kin = A.dense_keypoints(levels, 300, 300)
    assert sorted(set(kin[:, 3].astype(int))) == list(range(len(levels))) and len(levels) == 4
