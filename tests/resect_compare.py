"""sfmloc_sfm_resect against the oracle's resection of every view (adjust_scene.oracle_resect), field for field and bit
for bit: shared by test_gpu_adjust.py and tests/tools/k5_forms_cases.py."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def compare_view(h, k, r, e):
    """view k of handle h: its sfmloc_sfm_view_result r and its inlier list against the oracle's record e"""
    assert bool(r.ran) == e["ran"] and r.n_obs == e["n_obs"], k
    if not e["ran"]:
        assert len(h.resect_inliers(k)) == 0
        return
    # every view that ran, failed or not: iterations, NFA, the best model's P, its inliers
    assert bool(r.ok) == (e["n"] >= 8), k
    assert r.iterations == e["iters"] and r.nfa == e["nfa"], k
    np.testing.assert_array_equal(bits(np.array(r.P)), bits(e["P"].ravel()), err_msg=str(k))
    inl = h.resect_inliers(k)
    assert len(inl) == r.n_inliers, k
    if e["n"] > 0:                  # Localize's gate passed: the wrapper's count and list
        assert r.n_inliers == e["n"], k
        np.testing.assert_array_equal(inl, e["inliers"])
    else:                           # below the gate the oracle's count is not reported: its list's prefix
        assert 0 <= r.n_inliers <= 7, k
        np.testing.assert_array_equal(inl, e["inl_raw"][:r.n_inliers])
        assert (r.n_inliers == 0) == (not np.any(e["P"])), k
    if r.n_inliers > 0:             # errmax is the n_inliers-th smallest residual: pins the count as well
        assert r.error_max == e["errmax"], k
    if e["ok"]:
        np.testing.assert_array_equal(bits(np.array(r.R)), bits(e["R"].ravel()))
        np.testing.assert_array_equal(bits(np.array(r.center)), bits(e["center"]))
    else:                           # sfmloc.h: R and centre only on success
        assert not np.any(np.array(r.R)) and not np.any(np.array(r.center)), k


def resect_and_compare(h, exp):
    """h.resect() against the oracle's resection of every view (adjust_scene.oracle_resect) -> resect_read()"""
    ran, ok = h.resect()
    res = h.resect_read()
    assert ran == sum(e["ran"] for e in exp) and ok == sum(e["ok"] for e in exp)
    for k, (r, e) in enumerate(zip(res, exp)):
        compare_view(h, k, r, e)
    return res
