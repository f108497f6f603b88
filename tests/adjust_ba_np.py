"""CPU twin of sfmloc_sfm_adjust (include/sfmloc.h, "blocks" .. "stopping"): the residual, the Huber loss and the
per-block problems of the separable commands (structure alone; rotations, translations or both alone) in NumPy, and two
independent solvers over them: scipy.optimize.least_squares (trust-region reflective, its tolerances at their floor)
and a plain Levenberg-Marquardt written from the solver rules of the header.  Arrays as adjust.sfm_arrays returns them.

A pose block is [angle-axis of R (3), t (3)], t = -R C.  The two solvers step in the angle-axis itself (analytic
Jacobian through the left Jacobian of SO(3)); the device steps in the tangent space at the current rotation.  The
robust cost has one minimum in the basin the scene starts in, and that minimum is what is compared."""
import numpy as np
from scipy.optimize import least_squares

HUBER_A = 16.0                    # HuberLoss(Square(4.0)): the squared 4.0 is the reference's quirk
ROTATION, TRANSLATION, INTRINSICS, STRUCTURE = 1, 2, 4, 8
EPS = float(np.finfo(np.float64).eps)


# ---- loss ------------------------------------------------------------------------------------------------------------
def rho(s):
    """Ceres HuberLoss(a) on s = |r|^2 -> (rho, rho')"""
    s = np.asarray(s, np.float64)
    out = s.copy()
    d = np.ones_like(s)
    big = s > HUBER_A * HUBER_A
    rt = np.sqrt(s[big])
    out[big] = 2.0 * HUBER_A * rt - HUBER_A * HUBER_A
    d[big] = HUBER_A / rt
    return out, d


def robust_cost(r):
    """1/2 sum rho(|r_k|^2) of residuals r [n, 2]"""
    r = np.asarray(r, np.float64).reshape(-1, 2)
    return 0.5 * float(rho((r * r).sum(1))[0].sum())


def paired_huber(z):
    """least_squares' callable loss for residuals that come in pairs (x, y of one observation): z = f^2 per component,
    the loss acts on the pair's sum s.  Row 0 shares rho(s) between the two components in proportion to z (their sum is
    rho(s), so the solver's cost is 1/2 sum rho), row 1 is rho'(s) for both (the exact gradient J^T rho' f), row 2 is 0:
    the first-order reweighting, no second-order correction."""
    s = z.reshape(-1, 2).sum(1)
    r0, r1 = rho(s)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(s[:, None] > 0.0, z.reshape(-1, 2) / s[:, None], 0.5)
    out = np.empty((3, z.size))
    out[0] = (share * r0[:, None]).ravel()
    out[1] = np.repeat(r1, 2)
    out[2] = 0.0
    return out


# ---- rotations -------------------------------------------------------------------------------------------------------
def hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def rodrigues(w):
    w = np.asarray(w, np.float64)
    th = float(np.sqrt(w @ w))
    K = hat(w)
    if th < 1e-8:
        return np.eye(3) + K + 0.5 * (K @ K)
    return np.eye(3) + (np.sin(th) / th) * K + ((1.0 - np.cos(th)) / (th * th)) * (K @ K)


def left_jacobian(w):
    w = np.asarray(w, np.float64)
    th = float(np.sqrt(w @ w))
    K = hat(w)
    if th < 1e-5:
        return np.eye(3) + 0.5 * K + (K @ K) / 6.0
    return np.eye(3) + ((1.0 - np.cos(th)) / (th * th)) * K + ((th - np.sin(th)) / (th ** 3)) * (K @ K)


def angle_axis(R):
    """rotation matrix -> angle-axis (through the quaternion, as Ceres' RotationMatrixToAngleAxis does)"""
    R = np.asarray(R, np.float64).reshape(3, 3)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr >= 0.0:
        t = np.sqrt(tr + 1.0)
        q = np.array([0.5 * t, (R[2, 1] - R[1, 2]) * (0.5 / t), (R[0, 2] - R[2, 0]) * (0.5 / t),
                      (R[1, 0] - R[0, 1]) * (0.5 / t)])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = np.zeros(4)
        q[i + 1] = 0.5 * t
        q[0] = (R[k, j] - R[j, k]) * (0.5 / t)
        q[j + 1] = (R[j, i] + R[i, j]) * (0.5 / t)
        q[k + 1] = (R[k, i] + R[i, k]) * (0.5 / t)
    sn = float(np.sqrt(q[1:] @ q[1:]))
    if sn < 1e-300:
        return 2.0 * q[1:]
    th = 2.0 * (np.arctan2(sn, q[0]) if q[0] >= 0.0 else np.arctan2(-sn, -q[0]))
    return q[1:] * (th / sn)


def nearest_angle_axis(w, near):
    """the angle-axis of the same rotation as w that lies closest to `near` (w + 2 pi k along its axis: near an angle of
    pi two solvers may name one rotation on either side)"""
    w = np.asarray(w, np.float64)
    th = float(np.sqrt(w @ w))
    if th == 0.0:
        return w
    cands = [w * (1.0 + 2.0 * np.pi * k / th) for k in (-1, 0, 1)]
    return min(cands, key=lambda c: float(np.abs(c - near).max()))


def t_of(R, C):
    """t = -R C, row by row as the header states it"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    C = np.asarray(C, np.float64).reshape(-1, 3)
    return -np.stack([(R[:, 3 * i] * C[:, 0] + R[:, 3 * i + 1] * C[:, 1]) + R[:, 3 * i + 2] * C[:, 2] for i in range(3)], 1)


def c_of(R, t):
    """C = -R^T t"""
    R = np.asarray(R, np.float64).reshape(-1, 9)
    t = np.asarray(t, np.float64).reshape(-1, 3)
    return -np.stack([(R[:, i] * t[:, 0] + R[:, 3 + i] * t[:, 1]) + R[:, 6 + i] * t[:, 2] for i in range(3)], 1)


# ---- residual --------------------------------------------------------------------------------------------------------
def obs_landmark(a):
    off = a["obs_off"].astype(np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def entering(a, obs_keep=None, landmark_keep=None):
    """the observations that enter: kept observations of kept landmarks (all before the first cleanup)"""
    e = np.ones(len(a["obs_view"]), bool)
    if obs_keep is not None:
        e &= np.asarray(obs_keep, bool)
    if landmark_keep is not None:
        e &= np.asarray(landmark_keep, bool)[obs_landmark(a)]
    return e


def terms(a, idx, R, t, X, want_jac=True):
    """observations idx with rotations R [n, 3, 3], translations t [n, 3] and points X [n, 3] ->
    (r [n, 2] = proj - obs.x, d r / d Xc [n, 2, 3], R X [n, 3])"""
    v = a["obs_view"][idx].astype(np.int64)
    ii = a["view_intrinsic"][v].astype(np.int64)
    K = a["intrinsic"][ii]
    radial = a["intrinsic_type"][ii] == 3
    f, ppx, ppy = K[:, 0], K[:, 1], K[:, 2]
    Y = np.stack([(R[:, i, 0] * X[:, 0] + R[:, i, 1] * X[:, 1]) + R[:, i, 2] * X[:, 2] for i in range(3)], 1)
    Xc = Y + t
    iz = 1.0 / Xc[:, 2]
    p0, p1 = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = p0 * p0 + p1 * p1
    r4 = r2 * r2
    r6 = r4 * r2
    rc = np.where(radial, ((1.0 + K[:, 3] * r2) + K[:, 4] * r4) + K[:, 5] * r6, 1.0)
    r = np.stack([(f * (p0 * rc) + ppx) - a["obs_x"][idx, 0], (f * (p1 * rc) + ppy) - a["obs_x"][idx, 1]], 1)
    if not want_jac:
        return r, None, Y
    drc = np.where(radial, K[:, 3] + 2.0 * K[:, 4] * r2 + 3.0 * K[:, 5] * r4, 0.0)    # d rc / d r2
    # d q / d p, q = p rc(r2)
    q00 = rc + 2.0 * drc * p0 * p0
    q01 = 2.0 * drc * p0 * p1
    q11 = rc + 2.0 * drc * p1 * p1
    # d p / d Xc = [[iz, 0, -p0 iz], [0, iz, -p1 iz]]
    J = np.empty((len(idx), 2, 3))
    J[:, 0, 0] = f * q00 * iz
    J[:, 0, 1] = f * q01 * iz
    J[:, 0, 2] = -f * (q00 * p0 + q01 * p1) * iz
    J[:, 1, 0] = f * q01 * iz
    J[:, 1, 1] = f * q11 * iz
    J[:, 1, 2] = -f * (q01 * p0 + q11 * p1) * iz
    return r, J, Y


class Problem:
    """one block: x0, fun(x) -> raw residuals [2 n] (no loss applied), jac(x) [2 n, k], n observations"""

    def __init__(self, x0, fun, jac, n):
        self.x0, self.fun, self.jac, self.n = np.asarray(x0, np.float64), fun, jac, n

    def cost(self, x):
        return robust_cost(self.fun(x))


def structure_problem(a, l, enter, pose_R, pose_t, X):
    off = a["obs_off"].astype(np.int64)
    idx = np.arange(off[l], off[l + 1])[enter[off[l]:off[l + 1]]]
    pi = a["view_pose"][a["obs_view"][idx].astype(np.int64)].astype(np.int64)
    R = np.asarray(pose_R, np.float64).reshape(-1, 3, 3)[pi]
    t = np.asarray(pose_t, np.float64).reshape(-1, 3)[pi]

    def fun(x):
        return terms(a, idx, R, t, np.broadcast_to(x, (len(idx), 3)), False)[0].ravel()

    def jac(x):
        _, J, _ = terms(a, idx, R, t, np.broadcast_to(x, (len(idx), 3)))
        return np.einsum("nij,njk->nik", J, R).reshape(-1, 3)
    return Problem(X[l], fun, jac, len(idx))


def pose_observations(a, p, enter):
    """the entering observations of pose p: its views in ascending view index, each view's list in ascending landmark"""
    out = []
    for v in np.nonzero(a["view_pose"] == p)[0]:
        out.append(np.nonzero((a["obs_view"] == v) & enter)[0])
    return np.concatenate(out) if out else np.zeros(0, np.int64)


def pose_problem(a, p, what, enter, aa, t, X, idx=None):
    """what: ROTATION, TRANSLATION or both.  x = the free part of [angle-axis, t]."""
    if idx is None:
        idx = pose_observations(a, p, enter)
    Xo = np.asarray(X, np.float64)[obs_landmark(a)[idx]]
    w0, t0 = np.array(aa[p], np.float64), np.array(t[p], np.float64)
    rot, trn = bool(what & ROTATION), bool(what & TRANSLATION)

    def split(x):
        return (x[:3] if rot else w0), (x[3:] if rot and trn else x if trn else t0)

    def fun(x):
        w, tt = split(x)
        R = rodrigues(w)
        return terms(a, idx, np.broadcast_to(R, (len(idx), 3, 3)), np.broadcast_to(tt, (len(idx), 3)), Xo, False)[0].ravel()

    def jac(x):
        w, tt = split(x)
        R = rodrigues(w)
        _, J, Y = terms(a, idx, np.broadcast_to(R, (len(idx), 3, 3)), np.broadcast_to(tt, (len(idx), 3)), Xo)
        cols = []
        if rot:
            Jl = left_jacobian(w)
            # d (exp(w) X) / d w = -[R X]x Jl(w)
            Yx = np.zeros((len(idx), 3, 3))
            Yx[:, 0, 1], Yx[:, 0, 2] = -Y[:, 2], Y[:, 1]
            Yx[:, 1, 0], Yx[:, 1, 2] = Y[:, 2], -Y[:, 0]
            Yx[:, 2, 0], Yx[:, 2, 1] = -Y[:, 1], Y[:, 0]
            cols.append(np.einsum("nij,njk->nik", J, -Yx @ Jl))
        if trn:
            cols.append(J)
        return np.concatenate(cols, 2).reshape(2 * len(idx), -1)
    x0 = np.concatenate(([w0] if rot else []) + ([t0] if trn else []))
    return Problem(x0, fun, jac, len(idx))


# ---- the two solvers --------------------------------------------------------------------------------------------------
def solve_scipy(prob):
    """-> (x, cost before, cost after, function evaluations).  A result above the input cost is never taken."""
    c0 = prob.cost(prob.x0)
    if prob.n == 0:
        return prob.x0.copy(), 0.0, 0.0, 0
    res = least_squares(prob.fun, prob.x0, jac=prob.jac, method="trf", loss=paired_huber, f_scale=1.0, x_scale="jac",
                        ftol=EPS, xtol=EPS, gtol=EPS, max_nfev=2000)
    c1 = prob.cost(res.x)
    if not (np.all(np.isfinite(res.x)) and c1 < c0):
        return prob.x0.copy(), c0, c0, res.nfev
    return res.x, c0, c1, res.nfev


FTOL = 1e-14
MAX_STEPS = 500


def _normal(prob, x):
    r = prob.fun(x).reshape(-1, 2)
    J = prob.jac(x).reshape(len(r), 2, -1)
    r0, r1 = rho((r * r).sum(1))
    w = np.sqrt(r1)
    Jw = (J * w[:, None, None]).reshape(2 * len(r), -1)
    rw = (r * w[:, None]).ravel()
    return Jw.T @ Jw, Jw.T @ rw, 0.5 * float(r0.sum())


def solve_lm(prob):
    """Levenberg-Marquardt from the header's solver rules -> (x, cost before, cost after, steps tried, at the cap)"""
    x = prob.x0.copy()
    if prob.n == 0:
        return x, 0.0, 0.0, 0, False
    A, g, c = _normal(prob, x)
    c0 = c
    lam, nu = 1e-4, 2.0
    steps = 0
    capped = True
    while steps < MAX_STEPS:
        steps += 1
        D = np.clip(np.diag(A), 1e-6, 1e32)
        try:
            with np.errstate(all="ignore"):
                d = -np.linalg.solve(A + lam * np.diag(D), g)
        except np.linalg.LinAlgError:
            d = np.full_like(g, np.nan)
        model = -(g @ d + 0.5 * (d @ (A @ d)))
        ok = bool(np.all(np.isfinite(d))) and model > 0.0
        if ok:
            xn = x + d
            with np.errstate(all="ignore"):
                An, gn, cn = _normal(prob, xn)
            ok = bool(np.isfinite(cn)) and bool(np.all(np.isfinite(An))) and bool(np.all(np.isfinite(gn)))
        if ok and cn < c and (c - cn) / model > 1e-3:
            q = (c - cn) / model
            done = (c - cn) <= FTOL * c
            x, A, g, c = xn, An, gn, cn
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3), 1e-32)
            nu = 2.0
            if done:
                capped = False
                break
        else:
            if np.isfinite(model) and model <= FTOL * c:
                capped = False
                break
            lam *= nu
            nu *= 2.0
            if not lam < 1e32:
                capped = False
                break
    return x, c0, c, steps, capped


# ---- a whole adjustment ----------------------------------------------------------------------------------------------
def adjust(a, what, pose_R, pose_C, X, solver="scipy", obs_keep=None, landmark_keep=None):
    """what = STRUCTURE, ROTATION, TRANSLATION or ROTATION | TRANSLATION on the scene (a, poses, X) ->
    dict(pose_R [n, 9], pose_C, aa, t, X, blocks (block indices that had observations), x (their solutions),
    cost0, cost1 (per block), steps)"""
    assert what in (0, 1, 2, 3, 8)
    solve = {"scipy": solve_scipy, "lm": solve_lm}[solver]
    pose_R = np.array(pose_R, np.float64).reshape(-1, 9)
    pose_C = np.array(pose_C, np.float64).reshape(-1, 3)
    X = np.array(X, np.float64).reshape(-1, 3)
    enter = entering(a, obs_keep, landmark_keep)
    t = t_of(pose_R, pose_C)
    aa = np.array([angle_axis(R) for R in pose_R])
    out = {"blocks": [], "x": [], "cost0": [], "cost1": [], "steps": []}
    if what == STRUCTURE:
        for l in range(len(X)):
            prob = structure_problem(a, l, enter, pose_R, t, X)
            if prob.n == 0:
                continue
            sol = solve(prob)
            out["blocks"].append(l)
            out["x"].append(sol[0])
            out["cost0"].append(sol[1])
            out["cost1"].append(sol[2])
            out["steps"].append(sol[3])
        Xn = X.copy()
        for l, x in zip(out["blocks"], out["x"]):
            Xn[l] = x
        X = Xn
    elif what:
        aa_n, t_n, R_n, C_n = aa.copy(), t.copy(), pose_R.copy(), pose_C.copy()
        for p in range(len(pose_R)):
            prob = pose_problem(a, p, what, enter, aa, t, X)
            if prob.n == 0:
                continue
            sol = solve(prob)
            x = sol[0]
            out["blocks"].append(p)
            out["x"].append(x)
            out["cost0"].append(sol[1])
            out["cost1"].append(sol[2])
            out["steps"].append(sol[3])
            if sol[2] < sol[1]:
                if what & ROTATION:
                    aa_n[p] = x[:3]
                    R_n[p] = rodrigues(x[:3]).reshape(9)
                if what & TRANSLATION:
                    t_n[p] = x[3:] if what & ROTATION else x
                C_n[p] = c_of(R_n[p], t_n[p])[0]
        aa, t, pose_R, pose_C = aa_n, t_n, R_n, C_n
    out.update(pose_R=pose_R, pose_C=pose_C, aa=aa, t=t, X=X)
    for k in ("cost0", "cost1"):
        out[k] = np.array(out[k], np.float64)
    return out


def block_costs(a, what, pose_R, pose_C, X, obs_keep=None, landmark_keep=None, t=None):
    """the robust cost of every block of `what` at (poses, X) -> {block index: cost}.  t: the translations where the
    caller knows their bits (a rotation-only adjustment holds them), else -R C"""
    pose_R = np.asarray(pose_R, np.float64).reshape(-1, 9)
    X = np.asarray(X, np.float64).reshape(-1, 3)
    enter = entering(a, obs_keep, landmark_keep)
    idx = np.nonzero(enter)[0]
    v = a["obs_view"][idx].astype(np.int64)
    pi = a["view_pose"][v].astype(np.int64)
    lm = obs_landmark(a)[idx]
    t = t_of(pose_R, pose_C) if t is None else np.asarray(t, np.float64).reshape(-1, 3)
    r, _, _ = terms(a, idx, pose_R.reshape(-1, 3, 3)[pi], t[pi], X[lm], False)
    c = 0.5 * rho((r * r).sum(1))[0]
    key = lm if what == STRUCTURE else pi
    return {int(k): float(c[key == k].sum()) for k in np.unique(key)}
