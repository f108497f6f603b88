"""CPU: every case of akaze_cases.py is what it says it is -- the number of levels, which octaves are evolved in LDS and
in runs of what length, the side of the segment scan's one-launch limit, the side of the output paths' keypoint counts,
keypoints at the far edge -- by the CPU restatement alone (oracle_c.akaze_levels / akaze_detect_and_compute).  These are
conditions on the inputs, not measurements of the library: test_gpu_akaze_shapes.py runs the same cases on the device,
and a case that drifted off its boundary would leave a kernel form untested with everything green.  The conditions are
restated in akaze_cases.py; the library's own are in csrc/akaze_plan.h, and a host program over that header
(akaze_header.py) says here that both put every case on the same side, with the same constants."""
import numpy as np
import pytest

import akaze_cases as A
import akaze_header as H


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


@pytest.fixture(scope="module")
def header(tmp_path_factory):
    """-> (the constants of csrc/akaze_plan.h, {request: its plan and launch schedule by that header})"""
    reqs = [(c.w, c.h, c.n_octaves, c.n_sublevels) for c in A.CASES + A.NEED_CASES]
    return H.run(H.build(tmp_path_factory.mktemp("akaze_schedule")), list(dict.fromkeys(reqs)))


def header_resident_plan(plan, need):
    """the header's evolution steps of a call that builds `need` levels -> per octave (run, resident), as
    A.resident_plan gives it; on the way: the steps cover the loop's levels 1 .. need - 1 once and in order, a run stays in
    its octave, and a single level's launches never run in place and end in the level's Lt"""
    built, steps = plan.evo[need]
    assert built == need
    octave = [ints[2] for ints, _ in plan.levels[:need]]
    out = [[0, False] for _ in range(octave[-1] + 1)]
    nxt = 1
    for s in steps:
        assert s.first == nxt and s.last >= s.first and len(set(octave[s.first:s.last + 1])) == 1
        nxt = s.last + 1
        assert s.halfsample == (octave[s.first] > octave[s.first - 1])
        o = out[octave[s.first]]
        o[0] += s.last - s.first + 1
        w, nsteps = plan.levels[s.first][0][0], plan.levels[s.first][0][5]
        if s.resident:
            assert o[0] == s.last - s.first + 1 and s.source == ("scratch" if s.halfsample else "prev")
            o[1] = True
        else:
            assert s.first == s.last and not o[1]
            assert s.fuse == (A.STEPS_SMALL if w <= A.SMALL_WIDTH else A.STEPS_LARGE)
            assert s.n_launch == -(-nsteps // s.fuse) >= 1
            assert (s.source == "prev") == (not s.halfsample)
            cur = s.source
            for j in range(s.n_launch):  # build_scale_space: launch j writes Lt when an even number of launches follow
                dst = "own" if (s.n_launch - 1 - j) % 2 == 0 else "scratch"
                assert dst != cur
                cur = dst
            assert cur == "own"
    assert nxt == need
    return [tuple(o) for o in out]


@pytest.mark.parametrize("c", A.CASES, ids=lambda c: c.name)
def test_header_schedules_what_the_case_promises(header, c):
    """the launch schedule the LIBRARY goes by (csrc/akaze_plan.h) puts the case where akaze_cases.py's restatement of it
    does: resident runs per octave, the side of the segment scan, the fixed grids"""
    constants, plans = header
    plan = plans[(c.w, c.h, c.n_octaves, c.n_sublevels)]
    assert plan.kind == "plan" and len(plan.levels) == c.levels
    assert header_resident_plan(plan, c.levels) == c.resident, c.what
    d = plan.detect
    assert d.n_seg == A.n_seg([ints[:2] for ints, _ in plan.levels], c.w) == d.rows * d.segs_per_row
    assert {"<": d.n_seg < constants["kSegScanOneLaunch"], "==": d.n_seg == constants["kSegScanOneLaunch"],
            ">": d.n_seg > constants["kSegScanOneLaunch"]}[c.seg], d.n_seg
    assert d.scan_two_launches == (c.seg == ">") and d.seg_chunks * constants["kSegChunk"] >= d.n_seg
    assert d.seg_chunks <= constants["kSegChunksMax"]
    assert (d.nbr_grid, d.desc_grid) == (A.fixed_grid(c.w, c.h, A.NBR_GRID), A.fixed_grid(c.w, c.h, A.DESC_GRID))
    assert (d.cand_cap, d.spec_start, d.spec_max) == (A.CAND_CAP, A.SPEC_START, A.SPEC_MAX)
    assert 1 <= d.hist_grid_y <= d.grad_grid_y == -(-c.h // constants["kGradRows"])
    assert d.hist_grid_y == 1 or d.hist_grid_x * d.hist_grid_y <= constants["kHistGridMax"]


def test_constants_equal_the_headers(header):
    """akaze_cases.py restates the thresholds by hand; csrc/akaze_plan.h is where the library has them"""
    constants = header[0]
    assert {k: constants[k] for k in A.HEADER_NAMES} == A.HEADER_NAMES


@pytest.mark.parametrize("n", A.NEED_CASES, ids=lambda n: n.name)
def test_need_cases_change_the_run(oracle_c, header, n):
    """a description-only call that stops below the plan's top level: the last octave's run is shorter, and at 128 x 100
    with ten sub-levels that moves it from the per-level kernels into LDS -- by the restatement and by the header"""
    levels = oracle_c.akaze_levels(n.w, n.h, n.n_octaves, n.n_sublevels)
    plan = header[1][(n.w, n.h, n.n_octaves, n.n_sublevels)]
    assert n.need < len(levels) == len(plan.levels) and n.cut != n.whole
    assert A.resident_plan(levels, n.need) == header_resident_plan(plan, n.need) == n.cut
    assert A.resident_plan(levels) == header_resident_plan(plan, len(levels)) == n.whole
    kin = A.dense_keypoints(levels, n.w, n.h)
    per_level = np.bincount(kin[:, 3].astype(int))
    assert len(per_level) == len(levels) and 100 <= per_level.min() and per_level.max() <= 1000


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
