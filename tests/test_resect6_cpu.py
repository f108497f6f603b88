"""CPU: the NumPy twin of the uncalibrated query's resection (tests/resect6_np.py) on hand-made cases, its building
blocks against the C oracle, the margins of the GPU tests' scenes (tests/resect6_cases.py), the declarations of the new
symbols and the tools' -u switch."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import resect6_cases as RC  # noqa: E402
import resect6_np as R6  # noqa: E402
from oracle import oracle_c  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

CLI_BIN = os.path.join(ROOT, "sfmlocalization_amd", "bin", "OpenMVGLocalization_AKAZE")


def test_building_blocks_equal_the_c_oracle():
    xs = np.concatenate([10.0 ** np.random.default_rng(0).uniform(-300, 300, 500),
                         [0.0, 1.0, 2.0, 1e-310, 5e-324, np.inf, 3.0, 1.4142135623730951]])
    a = R6.det_log10(xs)
    b = np.array([oracle_c.det_log10(float(v)) for v in xs])
    assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    for n in (7, 11, 65, 300):
        a, b = R6.logcombi_tables(6, n), oracle_c.logcombi_tables(6, n)
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), n
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32)), n
    seed = 0x5f3759df12345678
    for n in (7, 50):
        s = R6.sample(6, n, seed, R6.STAGE_RESECT6, 0, np.arange(40))
        for it in range(40):
            assert np.array_equal(s[it], oracle_c.ac_sample(6, np.arange(n), seed, R6.STAGE_RESECT6, 0, it)), (n, it)


def test_six_exact_points_give_the_planted_p():
    rng = np.random.default_rng(3)
    K = np.array([[1040.0, 0, 640], [0, 1040.0, 480], [0, 0, 1]])
    Rm, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    Rm *= np.sign(np.linalg.det(Rm))
    X = rng.uniform(-2, 2, (6, 3)) + np.array([0, 0, 8.0])
    t = rng.uniform(-0.5, 0.5, 3)
    P = K @ np.concatenate([Rm, t[:, None]], 1)
    Xw = (X - t) @ Rm                                    # camera frame X = R Xw + t
    x = (P @ np.concatenate([Xw, np.ones((6, 1))], 1).T).T
    x = x[:, :2] / x[:, 2:]
    xn, f, ppx, ppy = R6.normalize(x, 1280, 960)
    nm, M = R6.solve(xn[None], Xw[None])
    assert nm[0] == 1
    N1inv = np.array([[f, 0, ppx], [0, f, ppy], [0, 0, 1]])
    Pg = N1inv @ M[0].reshape(3, 4)
    Pg, Pt = Pg / np.linalg.norm(Pg), P / np.linalg.norm(P)
    assert np.abs(Pg - Pt).max() < 1e-8                  # up to scale, and the sign puts the points in front
    assert ((Pg[2] @ np.concatenate([Xw, np.ones((6, 1))], 1).T) > 0).all()


def test_rank_deficient_samples_give_no_model():
    rows = np.stack([RC.solver_batch(1, 1)[0], RC.solver_batch(1, 2)[0]])        # coplanar; a repeated point
    nm, M = R6.solve(rows[:, :12].reshape(-1, 6, 2), rows[:, 12:].reshape(-1, 6, 3))
    assert list(nm) == [0, 0]
    x, X, C, res, _ = RC.twin(64, 0.0, coplanar=True)
    assert res["ok"] == 0 and res["n_inliers"] == 0 and np.isfinite(res["P"]).all() and res["iterations"] == 4096


@pytest.mark.parametrize("n,outliers", RC.CASES)
def test_gpu_scene_margins(n, outliers):
    """What the GPU tests compare must not hang on a coin toss: on every scene that can be localised (more than
    2.5 * 6 correspondences can be inliers) the twin alone localises with at least 2 x min_inliers inliers, and the best
    NFA is not shared by a second model.  n = 7 stops at the min_resection_points gate and n = 11 can
    have at most 11 <= 15 inliers: not localised, by rule."""
    x, X, C, res, trace = RC.twin(n, outliers)
    nfas = np.array([v for _, v, _ in trace])
    if len(nfas):      # the best NFA belongs to ONE model (the same sample drawn again is the same model, not a tie)
        assert len({smp for _, v, smp in trace if v == nfas.min()}) == 1, "two models tie for the best NFA"
    if n == 24 and outliers:
        return                                   # 17 true matches: may or may not pass the 15-inlier gate, no margin
    if n in RC.LOCALISABLE:
        assert res["ok"] == 1 and res["n_inliers"] >= 2 * RC.MIN_INLIERS
        f_err, c_err = RC.planted_errors(res, C)
        assert f_err < 0.01 and c_err < 0.05
    else:
        assert res["ok"] == 0
        assert (res["iterations"] == 0) == (n <= 8)


def test_new_symbols_are_declared():
    assert "sfmloc_query_set_uncalibrated" in capi.SYMBOLS and "sfmloc_debug_resect6" in capi.SYMBOLS
    L = capi._L()
    assert L.sfmloc_query_set_uncalibrated.argtypes == [C.c_void_p, C.c_int]
    assert len(L.sfmloc_debug_resect6.argtypes) == 9
    assert L.sfmloc_abi_version() == 2
    assert hasattr(capi.Query, "set_uncalibrated")
    assert L.sfmloc_query_set_uncalibrated(None, 1) == -1            # SFMLOC_EINVAL, no device needed
    header = open(os.path.join(ROOT, "include", "sfmloc.h")).read()
    assert "int sfmloc_query_set_uncalibrated(sfmloc_query *q, int on);" in header
    assert "RESTATED, UNVERIFIED AGAINST OpenMVG" in header


def test_both_tools_accept_u(capsys):
    from sfmlocalization_amd import engine
    assert engine.main([]) == 1
    assert "[-u|--uncalibrated]" in capsys.readouterr().out
    pos, o = engine.parse_cv_args(["a", "b", "c", "d", "-u"], engine.KEYS)
    assert o["uncalibrated"] is True and engine.parse_cv_args(["a"], engine.KEYS)[1]["uncalibrated"] is False
    assert engine.parse_cv_args(["--uncalibrated"], engine.KEYS)[1]["uncalibrated"] is True
    r = subprocess.run([CLI_BIN], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and "[-u|--uncalibrated]" in r.stdout
