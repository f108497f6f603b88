"""A second, independent two-view refinement for tests/golden/make_relrefine_fixtures.py: scipy.optimize.least_squares on
the cost of include/sfmloc.h "Two-view refinement" -- four residuals per inlier in undistorted pixels, no loss -- under
another parametrisation (a rotation vector on the left of the starting rotation, a free translation renormalised inside
the residual, the points) and with nothing eliminated by hand.  It shares no code with tests/relrefine_np.py: the points
start from numpy.linalg.svd on the four DLT rows, the derivatives are SciPy's complex steps."""
import numpy as np
from scipy.optimize import least_squares
from scipy.sparse import lil_matrix

DENSE_MAX_POINTS = 100      # above this the Jacobian is kept sparse and the trust-region steps come from LSMR


def rodrigues(w):
    """exp([w]x), also for a complex w (the complex step of the derivative)"""
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if abs(th2) < 1e-16:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        th = np.sqrt(th2)
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    K = np.array([[0 * w[0], -w[2], w[1]], [w[2], 0 * w[0], -w[0]], [-w[1], w[0], 0 * w[0]]])
    return np.eye(3) + a * K + b * (K @ K)


def triangulate(R, t, b):
    """-> (X [n, 3] in the first view's frame, depths [n, 2]) of the matches with bearings b [n, 4]"""
    P1 = np.hstack([np.eye(3), np.zeros((3, 1))])
    P2 = np.hstack([np.asarray(R, float).reshape(3, 3), np.asarray(t, float).reshape(3, 1)])
    X, z = np.zeros((len(b), 3)), np.zeros((len(b), 2))
    for n, (a0, a1, u, v) in enumerate(b):
        A = np.stack([a0 * P1[2] - P1[0], a1 * P1[2] - P1[1], u * P2[2] - P2[0], v * P2[2] - P2[1]])
        h = np.linalg.svd(A)[2][-1]
        X[n] = h[:3] / h[3]
        z[n] = X[n, 2], (P2 @ np.append(X[n], 1.0))[2]
    return X, z


def residuals(x, R0, b, fi, fj):
    R = rodrigues(x[0:3]) @ R0
    t = x[3:6] / np.sqrt(x[3] * x[3] + x[4] * x[4] + x[5] * x[5])
    X = x[6:].reshape(-1, 3)
    Y = X @ R.T + t
    return np.concatenate([fi * (X[:, :2] / X[:, 2:] - b[:, :2]), fj * (Y[:, :2] / Y[:, 2:] - b[:, 2:])], 1).ravel()


def refine(R0, t0, b, fi, fj, tol=1e-14, max_nfev=2000):
    """R0 [3, 3], t0 [3], b [n, 4] bearings (a, b, u, v), the two focal lengths -> dict(R, t, cost, cost_initial, n_used,
    nfev, status): the inliers whose starting point has positive depth in both views are the ones used"""
    R0, t0, b = np.asarray(R0, float).reshape(3, 3), np.asarray(t0, float).reshape(3), np.asarray(b, float).reshape(-1, 4)
    X0, z = triangulate(R0, t0, b)
    used = np.isfinite(X0).all(1) & np.isfinite(z).all(1) & (z > 0.0).all(1)
    b, X0 = b[used], X0[used]
    n = len(b)
    x0 = np.concatenate([np.zeros(3), t0, X0.ravel()])
    kw = {}
    if n > DENSE_MAX_POINTS:
        S = lil_matrix((4 * n, 6 + 3 * n), dtype=int)
        for k in range(n):
            S[4 * k:4 * k + 4, 6 + 3 * k:9 + 3 * k] = 1
            S[4 * k + 2:4 * k + 4, 0:6] = 1
        # (LSMR needs the columns scaled and its own tolerances tight: left at their defaults it is still descending
        # when max_nfev ends the run)
        kw = dict(jac_sparsity=S, tr_solver="lsmr", tr_options=dict(atol=1e-15, btol=1e-15), x_scale="jac")
    sol = least_squares(residuals, x0, jac="cs", method="trf", ftol=tol, xtol=tol, gtol=tol, max_nfev=max_nfev,
                        args=(R0, b, float(fi), float(fj)), **kw)
    t = sol.x[3:6] / np.linalg.norm(sol.x[3:6])
    r0 = residuals(x0, R0, b, float(fi), float(fj))
    return dict(R=rodrigues(sol.x[0:3]) @ R0, t=t, cost=float(sol.cost), cost_initial=float(0.5 * np.dot(r0, r0)),
                n_used=int(n), nfev=int(sol.nfev), status=int(sol.status))
