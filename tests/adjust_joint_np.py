"""CPU twin of sfmloc_sfm_adjust_joint (include/sfmloc.h, "parameters" .. "after"): poses, intrinsics and structure as
one robust least-squares problem, and two independent solvers over it.  The residual, the loss, the angle-axis code and
the entering rule are adjust_ba_np's.

  lm      the header's algorithm in NumPy: one Levenberg-Marquardt loop with one lambda, D = diag(J^T J) clamped, steps
          in the tangent space of the rotations.  At the test scenes' size the damped normal equations are solved
          exactly (a sparse direct factorisation), so no PCG is needed.
  scipy   scipy.optimize.least_squares (trust-region reflective over a sparse Jacobian, LSMR inside) on the same
          residuals with the paired Huber loss of adjust_ba_np; it steps in the angle-axis itself.

Both run to a tight stop; what is compared between them (and with the device) is gauge invariant: the residual vectors
at the solution and the total cost."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.optimize import least_squares

import adjust_ba_np as BN

ROTATION, TRANSLATION, INTRINSICS, STRUCTURE = 1, 2, 4, 8
FTOL = 1e-14
MAX_STEPS = 400


class Joint:
    """the problem of command `what` on scene a from (pose_R, pose_C, K, X); entering as adjust_ba_np.entering"""

    def __init__(self, a, what, pose_R, pose_C, K, X, obs_keep=None, landmark_keep=None):
        self.a, self.what = a, int(what)
        self.R0 = np.array(pose_R, np.float64).reshape(-1, 3, 3)
        self.t0 = BN.t_of(self.R0.reshape(-1, 9), pose_C)
        self.C0 = np.array(pose_C, np.float64).reshape(-1, 3)
        self.K0 = np.array(K, np.float64).reshape(-1, 6)
        self.X0 = np.array(X, np.float64).reshape(-1, 3)
        self.idx = np.nonzero(BN.entering(a, obs_keep, landmark_keep))[0]
        v = a["obs_view"][self.idx].astype(np.int64)
        self.pi = a["view_pose"][v].astype(np.int64)
        self.ii = a["view_intrinsic"][v].astype(np.int64)
        self.li = BN.obs_landmark(a)[self.idx]
        self.radial = np.asarray(a["intrinsic_type"]) == 3
        n = len(self.idx)
        # free columns of the tangent step [poses 6 | intrinsics 6 | landmarks 3]
        np_, ni, nl = len(self.R0), len(self.K0), len(self.X0)
        free = np.zeros(6 * np_ + 6 * ni + 3 * nl, bool)
        pose_in = np.zeros(np_, bool)
        intr_in = np.zeros(ni, bool)
        lm_in = np.zeros(nl, bool)
        if what & (ROTATION | TRANSLATION):
            pose_in[self.pi] = True
        if what & INTRINSICS:
            intr_in[self.ii] = True
        if what & STRUCTURE:
            lm_in[self.li] = True
        fp = free[:6 * np_].reshape(-1, 6)
        if what & ROTATION:
            fp[pose_in, :3] = True
        if what & TRANSLATION:
            fp[pose_in, 3:] = True
        fi = free[6 * np_:6 * np_ + 6 * ni].reshape(-1, 6)
        fi[intr_in, :3] = True
        fi[intr_in & self.radial, 3:] = True
        free[6 * np_ + 6 * ni:].reshape(-1, 3)[lm_in] = True
        self.free = np.nonzero(free)[0]
        self.pose_in, self.intr_in, self.lm_in = pose_in, intr_in, lm_in
        self.n_pose, self.n_intr, self.n_lm, self.n = np_, ni, nl, n
        rows = 2 * np.arange(n)
        self._rows = rows
        self._cols = (6 * self.pi, 6 * np_ + 6 * self.ii, 6 * np_ + 6 * ni + 3 * self.li)

    # ---- residual and Jacobian ----------------------------------------------------------------------------------
    def residual(self, R, t, K, X, want_jac=False):
        """raw residuals [n, 2]; with want_jac also (J d r / d Xc [n, 2, 3], Y = R X [n, 3], Ji [n, 2, 6])"""
        b = dict(self.a)
        b["intrinsic"] = K
        r, J, Y = BN.terms(b, self.idx, R[self.pi], t[self.pi], X[self.li], want_jac)
        if not want_jac:
            return r
        return r, J, Y, intrinsic_jacobian(K[self.ii], self.radial[self.ii], Y + t[self.pi])

    def cost(self, R, t, K, X):
        return BN.robust_cost(self.residual(R, t, K, X))

    def tangent_jacobian(self, R, t, K, X):
        """-> (raw r [n, 2], J [2 n, all columns] sparse: rotations step as R <- exp([w]x) R)"""
        r, J, Y, Ji = self.residual(R, t, K, X, True)
        Jc = np.concatenate([np.cross(Y[:, None, :], J), J], 2)        # J (-[Y]x) = Y x J row by row
        Jx = np.einsum("nij,njk->nik", J, R[self.pi])
        return r, self._assemble(Jc, Ji, Jx)

    def _assemble(self, Jc, Ji, Jx):
        blocks = []
        for Jb, col, w in ((Jc, self._cols[0], 6), (Ji, self._cols[1], 6), (Jx, self._cols[2], 3)):
            rr = (self._rows[:, None, None] + np.arange(2)[None, :, None]) + np.zeros((1, 1, w), np.int64)
            cc = (col[:, None, None] + np.arange(w)[None, None, :]) + np.zeros((1, 2, 1), np.int64)
            blocks.append((Jb.ravel(), rr.ravel(), cc.ravel()))
        val = np.concatenate([b[0] for b in blocks])
        row = np.concatenate([b[1] for b in blocks])
        col = np.concatenate([b[2] for b in blocks])
        ncol = 6 * self.n_pose + 6 * self.n_intr + 3 * self.n_lm
        return sp.csr_matrix((val, (row, col)), shape=(2 * self.n, ncol))

    def step(self, R, t, K, X, d_free):
        """the state moved by a tangent step over the free columns"""
        d = np.zeros(6 * self.n_pose + 6 * self.n_intr + 3 * self.n_lm)
        d[self.free] = d_free
        dp = d[:6 * self.n_pose].reshape(-1, 6)
        moved = d != 0.0                                    # (x + 0 would turn a -0 into +0: what is held keeps its bits)
        Rn, tn = R.copy(), np.where(moved[:6 * self.n_pose].reshape(-1, 6)[:, 3:], t + dp[:, 3:], t)
        if self.what & ROTATION:
            for p in np.nonzero(self.pose_in)[0]:
                Rn[p] = BN.rodrigues(dp[p, :3]) @ R[p]
        dk, mk = (v[6 * self.n_pose:6 * self.n_pose + 6 * self.n_intr].reshape(-1, 6) for v in (d, moved))
        dx, mx = (v[6 * self.n_pose + 6 * self.n_intr:].reshape(-1, 3) for v in (d, moved))
        Kn, Xn = np.where(mk, K + dk, K), np.where(mx, X + dx, X)
        return Rn, tn, Kn, Xn

    def result(self, R, t, K, X, steps):
        Rf = R.reshape(-1, 9)
        C = self.C0.copy()
        if self.what & (ROTATION | TRANSLATION):
            C[self.pose_in] = BN.c_of(Rf[self.pose_in], t[self.pose_in])
        r = self.residual(R, t, K, X)
        return dict(pose_R=Rf, pose_C=C, t=t, K=K, X=X, residual=r, cost0=self.cost(self.R0, self.t0, self.K0, self.X0),
                    cost1=BN.robust_cost(r), steps=steps)


def intrinsic_jacobian(K, radial, Xc):
    """d (raw residual) / d (f, ppx, ppy, k1, k2, k3) [n, 2, 6]; the k columns are 0 for a pinhole"""
    p0, p1 = Xc[:, 0] / Xc[:, 2], Xc[:, 1] / Xc[:, 2]
    r2 = np.where(radial, p0 * p0 + p1 * p1, 0.0)
    r4 = r2 * r2
    r6 = r4 * r2
    rc = np.where(radial, ((1.0 + K[:, 3] * r2) + K[:, 4] * r4) + K[:, 5] * r6, 1.0)
    f = K[:, 0]
    one, zero = np.ones_like(p0), np.zeros_like(p0)
    return np.stack([np.stack([p0 * rc, one, zero, f * (p0 * r2), f * (p0 * r4), f * (p0 * r6)], 1),
                     np.stack([p1 * rc, zero, one, f * (p1 * r2), f * (p1 * r4), f * (p1 * r6)], 1)], 1)


def _weighted(r, J):
    """first-order reweighting: residual and Jacobian rows times sqrt(rho')"""
    r0, r1 = BN.rho((r * r).sum(1))
    w = np.repeat(np.sqrt(r1), 2)
    return r.ravel() * w, sp.diags(w) @ J, 0.5 * float(r0.sum())


def solve_lm(pr, ftol=FTOL, max_steps=MAX_STEPS):
    """Levenberg-Marquardt by the header's rules; every damped system is solved exactly"""
    R, t, K, X = pr.R0.copy(), pr.t0.copy(), pr.K0.copy(), pr.X0.copy()

    def normal(R, t, K, X):
        r, J = pr.tangent_jacobian(R, t, K, X)
        rw, Jw, c = _weighted(r, J)
        Jf = Jw[:, pr.free].tocsc()
        return (Jf.T @ Jf).tocsc(), Jf.T @ rw, c, Jf
    A, g, c, Jf = normal(R, t, K, X)
    lam, nu, steps = 1e-4, 2.0, 0
    while steps < max_steps:
        steps += 1
        D = np.clip(A.diagonal(), 1e-6, 1e32)
        try:
            with np.errstate(all="ignore"):
                d = -spla.splu((A + lam * sp.diags(D)).tocsc()).solve(g)       # (a sparse direct factorisation: exact)
        except (RuntimeError, ValueError):
            d = np.full_like(g, np.nan)
        Jd = Jf @ d
        model = -(g @ d) - 0.5 * (Jd @ Jd)
        ok = bool(np.all(np.isfinite(d))) and model > 0.0
        if ok:
            with np.errstate(all="ignore"):
                Rn, tn, Kn, Xn = pr.step(R, t, K, X, d)
                cn = pr.cost(Rn, tn, Kn, Xn)
            ok = bool(np.isfinite(cn)) and cn < c and (c - cn) / model > 1e-3
        if ok:
            q = (c - cn) / model
            done = (c - cn) <= ftol * c
            R, t, K, X = Rn, tn, Kn, Xn
            A, g, c, Jf = normal(R, t, K, X)
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3), 1e-32)
            nu = 2.0
            if done:
                break
        else:
            if np.isfinite(model) and 0.0 < model <= ftol * c:
                break
            lam *= nu
            nu *= 2.0
            if not lam < 1e32:
                break
    return pr.result(R, t, K, X, steps)


def solve_scipy(pr, max_nfev=400):
    """least_squares over x = [angle-axis, t per pose | K | X], the free ones; a result above the input cost is not taken"""
    aa0 = np.array([BN.angle_axis(Rp) for Rp in pr.R0])
    full0 = np.concatenate([np.concatenate([aa0, pr.t0], 1).ravel(), pr.K0.ravel(), pr.X0.ravel()])

    def unpack(x):
        full = full0.copy()
        full[pr.free] = x
        pt = full[:6 * pr.n_pose].reshape(-1, 6)
        R = pr.R0.copy()
        if pr.what & ROTATION:
            for p in np.nonzero(pr.pose_in)[0]:
                R[p] = BN.rodrigues(pt[p, :3])
        K = full[6 * pr.n_pose:6 * pr.n_pose + 6 * pr.n_intr].reshape(-1, 6)
        return R, pt[:, 3:].copy(), K, full[6 * pr.n_pose + 6 * pr.n_intr:].reshape(-1, 3), pt[:, :3]

    def fun(x):
        R, t, K, X, _ = unpack(x)
        return pr.residual(R, t, K, X).ravel()

    def jac(x):
        R, t, K, X, aa = unpack(x)
        _, J, Y, Ji = pr.residual(R, t, K, X, True)
        Jl = np.array([BN.left_jacobian(w) for w in aa])
        Jrot = np.einsum("nij,njk->nik", np.cross(Y[:, None, :], J), Jl[pr.pi])      # J (-[Y]x) Jl(w)
        Jx = np.einsum("nij,njk->nik", J, R[pr.pi])
        return pr._assemble(np.concatenate([Jrot, J], 2), Ji, Jx)[:, pr.free].tocsr()
    res = least_squares(fun, full0[pr.free], jac=jac, method="trf", tr_solver="lsmr", loss=BN.paired_huber, f_scale=1.0,
                        x_scale="jac", ftol=BN.EPS, xtol=BN.EPS, gtol=BN.EPS, max_nfev=max_nfev,
                        tr_options={"atol": 1e-14, "btol": 1e-14})
    R, t, K, X, _ = unpack(res.x)
    out = pr.result(R, t, K, X, res.nfev)
    if not (np.all(np.isfinite(res.x)) and out["cost1"] < out["cost0"]):
        return pr.result(pr.R0, pr.t0, pr.K0, pr.X0, res.nfev)
    return out


def adjust(a, what, pose_R, pose_C, K, X, solver="lm", obs_keep=None, landmark_keep=None):
    pr = Joint(a, what, pose_R, pose_C, K, X, obs_keep, landmark_keep)
    return {"lm": solve_lm, "scipy": solve_scipy}[solver](pr)


def total_cost(a, pose_R, pose_C, K, X, obs_keep=None, landmark_keep=None, t=None):
    """the robust cost over the entering observations at (poses, K, X); t where the caller knows its bits"""
    pr = Joint(a, 15, pose_R, pose_C, K, X, obs_keep, landmark_keep)
    return pr.cost(pr.R0, pr.t0 if t is None else np.asarray(t, np.float64).reshape(-1, 3), pr.K0, pr.X0)


def residuals(a, pose_R, pose_C, K, X, obs_keep=None, landmark_keep=None, t=None):
    pr = Joint(a, 15, pose_R, pose_C, K, X, obs_keep, landmark_keep)
    return pr.residual(pr.R0, pr.t0 if t is None else np.asarray(t, np.float64).reshape(-1, 3), pr.K0, pr.X0)
