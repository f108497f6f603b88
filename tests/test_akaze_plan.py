"""CPU: the plan sfmloc_akaze_create makes on the host (sfmlocalization_amd/csrc/akaze_plan.h: the evolution levels and
every level's FED cycle) against the CPU restatement's plan (oracle/sfm_oracle_akaze.c), over a grid of requests -- level
sizes, octave, sub-level, sigma_size, nsteps and the bits of every step time.  A host program
(tests/cpp/akaze_plan.cpp) that includes the header the library includes prints the plans.

A FED cycle of more than 64 steps does not fit the plan's tables (nor the device's): both sides refuse such a request
and name the level.  A cycle of ONE step (sub-level counts from about 11 up) has nothing to reorder: both sides take the
step as it is (OpenCV's reordering reads in front of its array there)."""
import numpy as np
import pytest

import akaze_cases as A
import akaze_header as H

REFUSED = [(2560, 1280, 6, 4), (2560, 1280, 6, 1), (5120, 2560, 7, 4)]
ACCEPTED = (
    [(c.w, c.h, c.n_octaves, c.n_sublevels) for c in A.CASES]
    + [(A.PATH_W, A.PATH_H, A.PATH_PARAMS["n_octaves"], A.PATH_PARAMS["n_sublevels"]),
       (A.OVERFLOW_W, A.OVERFLOW_H, A.OVERFLOW_PARAMS["n_octaves"], A.OVERFLOW_PARAMS["n_sublevels"]),
       (300, 300, 2, 2)]
    + [(160, 80, 4, 4), (159, 80, 4, 4), (160, 79, 4, 4), (161, 81, 8, 4), (320, 160, 8, 4), (319, 160, 8, 4)]  # the cut
    + [(320, 240, 2, 16), (128, 96, 1, 32), (640, 480, 4, 8), (1280, 640, 5, 6), (2560, 1280, 5, 6), (640, 320, 8, 4)]  # 32
    + [(640, 480, 4, 4), (1920, 1080, 4, 4), (2560, 1280, 5, 4), (2560, 1280, 5, 2), (2560, 1280, 5, 3),  # (5, 2): 63 steps
       (16384, 4096, 5, 4), (16384, 4096, 5, 1), (16384, 4096, 4, 8), (16, 16, 8, 4), (16, 4096, 8, 4), (16384, 16, 8, 4)]
    + [(w, h, o, s) for (w, h) in ((641, 479), (333, 177)) for o in (1, 2, 3, 5) for s in (1, 2, 3, 5, 6, 7, 10, 11, 12)
       if o * s <= 32]
)
GRID = list(dict.fromkeys(ACCEPTED + REFUSED))


@pytest.fixture(scope="module")
def header_plans(tmp_path_factory):
    """-> {(w, h, n_octaves, n_sublevels): akaze_header.Plan or akaze_header.Refused}"""
    return H.run(H.build(tmp_path_factory.mktemp("akaze_plan")), GRID)[1]


@pytest.mark.parametrize("req", ACCEPTED, ids=lambda q: "%dx%d-o%d-s%d" % q)
def test_plan_equals_the_restatements(oracle_c, header_plans, req):
    w, h, omax, nsub = req
    lev, ts = oracle_c.akaze_plan(w, h, omax, nsub)
    kind, total, levels = header_plans[req][:3]
    assert kind == "plan"
    assert len(levels) == len(lev) <= A.MAX_LEVELS
    off = 0
    for i, (ints, bits) in enumerate(levels):
        assert ints[:6] == [int(v) for v in lev[i]], f"level {i}: w, h, octave, sublevel, sigma_size, nsteps"
        assert ints[6] == off, f"level {i}: offset in the stacks"
        off += ints[0] * ints[1]
        n = ints[5]
        assert 0 <= n <= 64 and (n >= 1) == (i >= 1) and len(bits) == n
        np.testing.assert_array_equal(bits, ts[i, :n].view(np.uint32), err_msg=f"level {i}: FED step times (bits)")
        assert np.isfinite(ts[i, :n]).all() and (ts[i, :n] > 0).all()
        # the cycle covers the level's evolution time (etime = esigma^2 / 2, esigma = 1.6 * 2^(octave + sublevel / nsub)),
        # whatever its order.  float32: the longest step is d / cos^2 of an angle up to pi / 2 - pi / (4 n + 2), whose
        # rounding (1.5e-7 absolute against a cosine of 0.012 at n = 64) is 2.5e-5 of that step, and the step is less than
        # half the sum: 1e-4 relative holds with room and still catches a missing, doubled or foreign step
        def etime(r):
            return 0.5 * 1.6 ** 2 * 4.0 ** (r[2] + r[3] / nsub)
        t = etime(lev[i]) - etime(lev[i - 1]) if i else 0.0
        assert abs(float(ts[i, :n].astype(np.float64).sum()) - t) <= 1e-4 * max(t, 1.0)
    assert total == off
    assert [tuple(r[:2]) for r in lev] == [tuple(x) for x in oracle_c.akaze_levels(w, h, omax, nsub)]


def test_level_table_is_bounded_at_32_levels(oracle_c):
    """the restatement's own bound (its plan used to have none): 32 levels asked for and 32 planned, none beyond"""
    assert len(oracle_c.akaze_plan(320, 240, 2, 16)[0]) == 32
    assert len(oracle_c.akaze_plan(128, 96, 1, 32)[0]) == 32
    assert len(oracle_c.akaze_plan(640, 320, 8, 4)[0]) == 16          # (the cut, far below the request)


@pytest.mark.parametrize("req", REFUSED, ids=lambda q: "%dx%d-o%d-s%d" % q)
def test_long_fed_cycles_are_refused_by_both(oracle_c, header_plans, req):
    kind, level, steps = header_plans[req]
    assert kind == "refused" and steps > 64 and 1 <= level < 32
    with pytest.raises(ValueError) as e:
        oracle_c.akaze_plan(*req)
    assert f"{steps} diffusion steps at level {level}" in str(e.value)
    with pytest.raises(ValueError):
        oracle_c.akaze_levels(*req)
    with pytest.raises(ValueError):
        oracle_c.akaze_detect_and_compute(np.zeros((req[1], req[0]), np.uint8), omax=req[2], nsub=req[3], cap=16)
    with pytest.raises(ValueError):
        oracle_c.akaze_compute(np.zeros((req[1], req[0]), np.uint8), np.zeros((1, 4), np.float32), omax=req[2], nsub=req[3])


def test_57_steps_are_accepted(oracle_c, header_plans):
    kind, _, levels = header_plans[(2560, 1280, 5, 4)][:3]
    assert kind == "plan" and max(ints[5] for ints, _ in levels) == 57
    assert int(oracle_c.akaze_plan(2560, 1280, 5, 4)[0][:, 5].max()) == 57


@pytest.mark.parametrize("req", REFUSED, ids=lambda q: "%dx%d-o%d-s%d" % q)
def test_library_refuses_before_it_looks_for_a_device(header_plans, req):
    """sfmloc_akaze_create plans on the host first: the refusal is EINVAL with or without a GPU, and names what the header
    named"""
    import sfmlocalization_amd as S
    from sfmlocalization_amd import capi
    _, level, steps = header_plans[req]
    with pytest.raises(S.SfmlocError) as ei:
        S.Akaze(req[0], req[1], n_octaves=req[2], n_sublevels=req[3])
    assert ei.value.code == capi.EINVAL
    assert f"needs {steps} diffusion steps at level {level} (at most 64 per level)" in ei.value.message
