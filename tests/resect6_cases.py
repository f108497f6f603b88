"""The synthetic 2D-3D sets of the uncalibrated-resection tests (test_resect6_cpu.py checks their margins with the twin
alone, test_gpu_resect6.py runs them on the device) and the twin's results on them, computed once per process."""
import functools

import numpy as np

import resect6_np as R6

WIDTH, HEIGHT = 1280, 960
MAP_FOCAL = 800.0
FOCAL = 1.3 * MAP_FOCAL       # the query camera's: P3P with the map's K would be wrong by 30 %
SIZES = (7, 11, 24, 64, 65, 300, 2000)
OUTLIERS = (0.0, 0.3)
# 7 <= min_resection_points (8): ends at the gate, as a calibrated query would.  11 runs AC-RANSAC but cannot have more
# than 2.5 * 6 = 15 inliers: not localised.  Both are compared with the twin field by field all the same.  24 without
# outliers is the smallest set here that can have 2 x min_inliers = 20 inliers: the localising case just above the gates
# (with 30 % outliers it has 17 true matches: above the 15-inlier gate, no margin asked of it).
LOCALISABLE = (24, 64, 65, 300, 2000)
MIN_INLIERS = 10              # sfmloc_default_params


def scene(n, outlier_frac, seed, coplanar=False):
    """-> (pt2d [n, 2] pixels, X [n, 3] world, camera centre)"""
    rng = np.random.default_rng(seed)
    K = np.array([[FOCAL, 0, WIDTH / 2], [0, FOCAL, HEIGHT / 2], [0, 0, 1.0]])
    a = rng.uniform(-0.3, 0.3, 3)
    cx, sx, cy, sy, cz, sz = np.cos(a[0]), np.sin(a[0]), np.cos(a[1]), np.sin(a[1]), np.cos(a[2]), np.sin(a[2])
    Rm = (np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]]) @ np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
          @ np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]]))
    C = rng.uniform(-1, 1, 3)
    Xc = np.stack([rng.uniform(-3, 3, n), rng.uniform(-2.2, 2.2, n), rng.uniform(5, 12, n)], 1)
    if coplanar:
        Xc[:, 2] = 8.0
    X = Xc @ Rm + C                      # X = R^T Xc + C
    x = (K @ Xc.T).T
    x = x[:, :2] / x[:, 2:]
    x += rng.normal(0, 0.3, x.shape)
    n_out = int(round(outlier_frac * n))
    idx = rng.permutation(n)[:n_out]
    x[idx] = np.stack([rng.uniform(0, WIDTH, n_out), rng.uniform(0, HEIGHT, n_out)], 1)
    return np.ascontiguousarray(x), np.ascontiguousarray(X), C


def seed_of(n, outlier_frac):
    return 100 + n + (7 if outlier_frac else 0)


CASES = [(n, o) for n in SIZES for o in OUTLIERS]


@functools.lru_cache(maxsize=None)
def twin(n, outlier_frac, coplanar=False):
    """-> (pt2d, X, centre, the twin's result, trace of (iteration, model NFA, sample))"""
    x, X, C = scene(n, outlier_frac, 5 if coplanar else seed_of(n, outlier_frac), coplanar)
    trace = []
    res = R6.localize(x, X, WIDTH, HEIGHT, min_inliers=MIN_INLIERS, trace=trace)
    return x, X, C, res, trace


def planted_errors(res, C):
    """(relative focal error, centre error) of a localised result against the scene"""
    f_err = max(abs(res["K"][0] - FOCAL), abs(res["K"][4] - FOCAL)) / FOCAL
    return f_err, float(np.abs(np.asarray(res["center"]) - C).max())


def solver_batch(count, seed):
    """`count` six-point samples [count, 30] (x[12], X[18]); the last one rank deficient (a repeated point, or all six
    coplanar for odd seeds)"""
    rows = np.zeros((count, 30))
    for i in range(count):
        x, X, _ = scene(6, 0.0, seed * 1000 + i, coplanar=(i == count - 1 and seed % 2 == 1))
        xn, _, _, _ = R6.normalize(x, WIDTH, HEIGHT)
        if i == count - 1 and seed % 2 == 0:
            xn[3], X[3] = xn[1], X[1]
        rows[i, :12] = xn.ravel()
        rows[i, 12:] = X.ravel()
    return rows
