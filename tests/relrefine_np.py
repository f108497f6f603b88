"""NumPy restatement of sfmloc_refine_relative_poses (include/sfmloc.h "Two-view refinement", csrc/relrefine.hip): the
bearings of the inlier matches, their two-view points, and the Levenberg-Marquardt loop over the pose and the points
with the points eliminated.  Only + - * / sqrt in f64, elementwise and in the stated order (NumPy does not fuse), the
sums in the kernel's order -- lane l of 256 adds its points l, l + 256, ... from 0, the wave's butterfly over xor 32 .. 1,
the four waves in order -- so the records are the device's bits.  refine_relative_poses has the calling convention of
capi.RelRefine."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from merge_np import jacobi_fixed  # noqa: E402
from relpose_np import bearings  # noqa: E402

OPTIONS = dict(max_steps=100, min_points=13)
THREADS = 256
FTOL = 1e-14                 # kBaFtol (csrc/ba_device.h)
LANE = np.arange(64)


def two_view_point(R, t, b1, b2):
    """two_view_point (csrc/twoview_device.h): bearings b1, b2 [n, 2] under [I | 0] and [R | t] (R [9], t [3]) ->
    (X [n, 3], z_J [n], exists [n])"""
    n = len(b1)
    P1 = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0])
    P2 = np.array([R[0], R[1], R[2], t[0], R[3], R[4], R[5], t[1], R[6], R[7], R[8], t[2]])
    with np.errstate(all="ignore"):
        G = np.zeros((n, 4, 4))
        for P, bb in ((P1, b1), (P2, b2)):
            a = bb[:, 0:1] * P[None, 8:12] - P[None, 0:4]
            b = bb[:, 1:2] * P[None, 8:12] - P[None, 4:8]
            G = G + a[:, :, None] * a[:, None, :]
            G = G + b[:, :, None] * b[:, None, :]
        d, V = jacobi_fixed([[G[:, min(i, j), max(i, j)] for j in range(4)] for i in range(4)])
        best = d[0]
        x = [V[k][0] for k in range(4)]
        for i in range(1, 4):
            take = d[i] < best
            best = np.where(take, d[i], best)
            x = [np.where(take, V[k][i], x[k]) for k in range(4)]
        X = np.stack([x[0] / x[3], x[1] / x[3], x[2] / x[3]], 1)
        ok = (x[3] != 0.0) & np.isfinite(x[3]) & np.isfinite(X).all(1)
        zj = ((R[6] * X[:, 0] + R[7] * X[:, 1]) + R[8] * X[:, 2]) + t[2]
    return X, zj, ok


def block_sum(terms, used):
    """sfmloc.h "reduction": terms [n] (or [n, q]) of the points in the order of the inlier list, used [n] -> the
    workgroup's sum(s)"""
    terms = np.asarray(terms, np.float64)
    flat = terms.ndim == 1
    if flat:
        terms = terms[:, None]
    n, q = terms.shape
    rows = max(1, -(-n // THREADS))
    pad = np.zeros((rows * THREADS, q))
    pad[:n] = terms
    msk = np.zeros(rows * THREADS, bool)
    msk[:n] = used
    pad, msk = pad.reshape(rows, THREADS, q), msk.reshape(rows, THREADS)
    acc = np.zeros((THREADS, q))
    with np.errstate(all="ignore"):
        for j in range(rows):                                   # lane l: its points l, l + 256, ... ascending
            acc = np.where(msk[j][:, None], acc + pad[j], acc)
        w = acc.reshape(4, 64, q)
        for m in (32, 16, 8, 4, 2, 1):                           # ba_group_sum<64>
            w = w + w[:, LANE ^ m]
        s = ((w[0, 0] + w[1, 0]) + w[2, 0]) + w[3, 0]
    return float(s[0]) if flat else s


def basis(t):
    """the tangent basis of the unit sphere at t -> B [3, 2]"""
    a = [abs(float(v)) for v in t]
    k, m = 0, a[0]
    if a[1] < m:
        k, m = 1, a[1]
    if a[2] < m:
        k = 2
    t0, t1, t2 = (np.float64(v) for v in t)
    z = np.float64(0.0)
    c = [(z, t2, -t1), (-t2, z, t0), (t1, -t0, z)][k]
    with np.errstate(all="ignore"):
        n = np.sqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2])
        b = [c[0] / n, c[1] / n, c[2] / n]
    B = np.zeros((3, 2))
    B[:, 0] = b
    B[0, 1] = t1 * b[2] - t2 * b[1]
    B[1, 1] = t2 * b[0] - t0 * b[2]
    B[2, 1] = t0 * b[1] - t1 * b[0]
    return B


def rotate(w, R):
    """C(w) R, R [9] -> [9]"""
    w = [np.float64(v) for v in w]
    xx = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    f = np.float64(2.0) / (np.float64(1.0) + xx)
    z = np.float64(0.0)
    K = [z, -w[2], w[1], w[2], z, -w[0], -w[1], w[0], z]
    M = [(1.0 if i == j else 0.0) + f * (K[3 * i + j] + (w[i] * w[j] - (xx if i == j else 0.0)))
         for i in range(3) for j in range(3)]
    return np.array([(M[3 * i] * R[j] + M[3 * i + 1] * R[3 + j]) + M[3 * i + 2] * R[6 + j]
                     for i in range(3) for j in range(3)])


def translate(t, B, d0, d1):
    v = [np.float64(t[i]) + (B[i, 0] * d0 + B[i, 1] * d1) for i in range(3)]
    n = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    return np.array([v[0] / n, v[1] / n, v[2] / n])


def essential(R, t):
    """[t]x R over its Frobenius norm; zeros where that is zero"""
    E = np.zeros(9)
    for j in range(3):
        E[j] = t[1] * R[6 + j] - t[2] * R[3 + j]
        E[3 + j] = t[2] * R[j] - t[0] * R[6 + j]
        E[6 + j] = t[0] * R[3 + j] - t[1] * R[j]
    s = np.float64(0.0)
    for i in range(9):
        s = s + E[i] * E[i]
    n = np.sqrt(s)
    return E / n if n > 0.0 else np.zeros(9)


def residual(R, t, fi, fj, X, b):
    """-> (r [n, 4], Z [n, 3], Y [n, 3], every depth finite and positive [n])"""
    with np.errstate(all="ignore"):
        Z = np.stack([(R[3 * i] * X[:, 0] + R[3 * i + 1] * X[:, 1]) + R[3 * i + 2] * X[:, 2] for i in range(3)], 1)
        Y = Z + np.asarray(t)[None]
        r = np.stack([fi * (X[:, 0] / X[:, 2] - b[:, 0]), fi * (X[:, 1] / X[:, 2] - b[:, 1]),
                      fj * (Y[:, 0] / Y[:, 2] - b[:, 2]), fj * (Y[:, 1] / Y[:, 2] - b[:, 3])], 1)
        good = (X[:, 2] > 0.0) & np.isfinite(X[:, 2]) & (Y[:, 2] > 0.0) & np.isfinite(Y[:, 2])
    return r, Z, Y, good


def squares(r):
    return ((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]) + r[:, 3] * r[:, 3]


def inv3(A):
    """rr_inv3: A [n, 3, 3] symmetric -> its inverse by Cholesky; NaN where a pivot is not positive"""
    n = len(A)
    L = np.zeros((n, 3, 3))
    for i in range(3):
        for j in range(i + 1):
            s = A[:, i, j].copy()
            for k in range(j):
                s = s - L[:, i, k] * L[:, j, k]
            if i == j:
                L[:, i, i] = np.sqrt(np.where(s > 0.0, s, -1.0))
            else:
                L[:, i, j] = s / L[:, j, j]
    Ai = np.zeros((n, 3, 3))
    for c in range(3):
        y, d = [None] * 3, [None] * 3
        for i in range(3):
            s = np.full(n, 1.0 if i == c else 0.0)
            for k in range(i):
                s = s - L[:, i, k] * y[k]
            y[i] = s / L[:, i, i]
        for i in (2, 1, 0):
            s = y[i]
            for k in range(i + 1, 3):
                s = s - L[:, k, i] * d[k]
            d[i] = s / L[:, i, i]
        for i in range(3):
            Ai[:, i, c] = d[i]
    return Ai


def clamp(a):
    """fmin(fmax(a, 1e-6), 1e32) with C's rule for NaN"""
    a = np.where(a > 1e-6, a, 1e-6)
    return np.where(a < 1e32, a, 1e32)


def point_terms(R, t, B, fi, fj, lam, X, b):
    """rr_point over all points -> (Vi [n, 3, 3], W [n, 5, 3], gx [n, 3], Ap [n, 15], gp [n, 5], r^2 [n])"""
    with np.errstate(all="ignore"):
        r, Z, Y, _ = residual(R, t, fi, fj, X, b)
        sq = squares(r)
        n = len(X)
        ix, iy = 1.0 / X[:, 2], 1.0 / Y[:, 2]
        d, e0, e1 = fi * ix, -(fi * (X[:, 0] / X[:, 2])) * ix, -(fi * (X[:, 1] / X[:, 2])) * ix
        a, c0, c1 = fj * iy, -(fj * (Y[:, 0] / Y[:, 2])) * iy, -(fj * (Y[:, 1] / Y[:, 2])) * iy
        zero = np.zeros(n)
        Jx = [[d, zero, e0], [zero, d, e1], [a * R[k] + c0 * R[6 + k] for k in range(3)],
              [a * R[3 + k] + c1 * R[6 + k] for k in range(3)]]
        P0 = [2.0 * (c0 * Z[:, 1]), 2.0 * (a * Z[:, 2] - c0 * Z[:, 0]), -2.0 * (a * Z[:, 1])]
        P1 = [2.0 * (c1 * Z[:, 1] - a * Z[:, 2]), -2.0 * (c1 * Z[:, 0]), 2.0 * (a * Z[:, 0])]
        for m in range(2):
            P0.append(a * B[0, m] + c0 * B[2, m])
            P1.append(a * B[1, m] + c1 * B[2, m])
        V = np.zeros((n, 3, 3))
        gx = np.zeros((n, 3))
        for i in range(3):
            for j in range(i, 3):
                V[:, i, j] = ((Jx[0][i] * Jx[0][j] + Jx[1][i] * Jx[1][j]) + Jx[2][i] * Jx[2][j]) + Jx[3][i] * Jx[3][j]
                V[:, j, i] = V[:, i, j]
            gx[:, i] = ((Jx[0][i] * r[:, 0] + Jx[1][i] * r[:, 1]) + Jx[2][i] * r[:, 2]) + Jx[3][i] * r[:, 3]
        for i in range(3):
            V[:, i, i] = V[:, i, i] + lam * clamp(V[:, i, i])
        Vi = inv3(V)
        W, F, gp = np.zeros((n, 5, 3)), np.zeros((n, 5, 3)), np.zeros((n, 5))
        for q in range(5):
            for i in range(3):
                W[:, q, i] = P0[q] * Jx[2][i] + P1[q] * Jx[3][i]
            for i in range(3):
                F[:, q, i] = (W[:, q, 0] * Vi[:, 0, i] + W[:, q, 1] * Vi[:, 1, i]) + W[:, q, 2] * Vi[:, 2, i]
            gp[:, q] = (P0[q] * r[:, 2] + P1[q] * r[:, 3]) - ((F[:, q, 0] * gx[:, 0] + F[:, q, 1] * gx[:, 1])
                                                              + F[:, q, 2] * gx[:, 2])
        Ap = np.zeros((n, 15))
        k = 0
        for q in range(5):
            for p in range(q, 5):
                Ap[:, k] = (P0[q] * P0[p] + P1[q] * P1[p]) - ((F[:, q, 0] * W[:, p, 0] + F[:, q, 1] * W[:, p, 1])
                                                              + F[:, q, 2] * W[:, p, 2])
                k += 1
    return Vi, W, gx, Ap, gp, sq


def solve5(A, g, lam):
    """ba_solve<5> (csrc/ba_device.h) -> (ok, d [5], model)"""
    N = 5
    A = [[np.float64(A[i][j]) for j in range(N)] for i in range(N)]
    g = [np.float64(v) for v in g]
    lam = np.float64(lam)
    L = [[np.float64(0.0)] * N for _ in range(N)]
    ok = True
    with np.errstate(all="ignore"):
        for i in range(N):
            for j in range(i + 1):
                s = A[i][j]
                if i == j:
                    s = s + lam * np.float64(clamp(A[i][i]))
                for k in range(j):
                    s = s - L[i][k] * L[j][k]
                if i == j:
                    ok = ok and bool(s > 0.0)
                    L[i][i] = np.sqrt(s)
                else:
                    L[i][j] = s / L[j][j]
        y, d = [None] * N, [None] * N
        for i in range(N):
            s = -g[i]
            for k in range(i):
                s = s - L[i][k] * y[k]
            y[i] = s / L[i][i]
        for i in range(N - 1, -1, -1):
            s = y[i]
            for k in range(i + 1, N):
                s = s - L[k][i] * d[k]
            d[i] = s / L[i][i]
        gd, dAd = np.float64(0.0), np.float64(0.0)
        for i in range(N):
            gd = gd + g[i] * d[i]
            s = np.float64(0.0)
            for j in range(N):
                s = s + A[i][j] * d[j]
            dAd = dAd + d[i] * s
            ok = ok and bool(np.isfinite(d[i]))
        model = -(gd + 0.5 * dAd)
    return ok and bool(model > 0.0), d, model


class Lm:
    """BaLm (csrc/ba_device.h)"""

    def __init__(self):
        self.lam, self.nu = np.float64(1e-4), np.float64(2.0)

    def accepted(self, c, cn, model):
        q = (c - cn) / model
        e = 2.0 * q - 1.0
        f = 1.0 - e * e * e
        third = np.float64(1.0) / np.float64(3.0)
        f = f if f > third else third                       # fmax(1 / 3, .)
        lam = self.lam * f
        self.lam = lam if lam > 1e-32 else np.float64(1e-32)
        self.nu = np.float64(2.0)
        return bool((c - cn) <= FTOL * c)

    def rejected(self, c, model):
        if np.isfinite(model) and model <= FTOL * c:
            return True
        self.lam = self.lam * self.nu
        self.nu = self.nu * 2.0
        return not bool(self.lam < 1e32)


def refine_pair(R, t, b, fi, fj, use=True, max_steps=100, min_points=13):
    """one pair: R [9], t [3], b [n, 4] the inliers' bearings (a, b, u, v) -> the fields of sfmloc_relrefine_result"""
    R, t = np.array(R, np.float64).reshape(9), np.array(t, np.float64).reshape(3)
    fi, fj = np.float64(fi), np.float64(fj)
    out = dict(status=0, n_used=0, steps=0, cost_initial=0.0, cost=0.0)
    if use:
        b = np.asarray(b, np.float64).reshape(-1, 4)
        X, zj, ok = two_view_point(R, t, b[:, :2], b[:, 2:])
        with np.errstate(all="ignore"):
            used = ok & np.isfinite(zj) & (X[:, 2] > 0.0) & (zj > 0.0)
        X = np.where(used[:, None], X, 0.0)
        out["n_used"] = int(used.sum())
        if out["n_used"] < min_points:
            out["status"] = 2
        else:
            Xu, bu = X[used], b[used]                          # (the sums skip the others; their places stay)
            lm = Lm()
            stop = moved = False
            finite0 = True
            steps = 0
            c = c0 = np.float64(0.0)
            B = basis(t)
            while not stop and steps < max_steps:
                steps += 1
                Vi, W, gx, Ap, gp, sq = point_terms(R, t, B, fi, fj, lm.lam, Xu, bu)
                full = np.zeros((len(X), 21))
                full[used] = np.concatenate([Ap, gp, sq[:, None]], 1)
                acc = block_sum(full, used)
                if steps == 1:
                    finite0 = bool(np.isfinite(acc).all())
                    if not finite0:
                        break
                    c = c0 = 0.5 * acc[20]
                A = np.zeros((5, 5))
                k = 0
                for i in range(5):
                    for j in range(i, 5):
                        A[i, j] = A[j, i] = acc[k]
                        k += 1
                ok, x, model = solve5(A, acc[15:20], lm.lam)
                cn = np.float64(0.0)
                if ok:
                    Rn, tn = rotate(x[:3], R), translate(t, B, x[3], x[4])
                    with np.errstate(all="ignore"):
                        h = np.stack([gx[:, i] + ((((W[:, 0, i] * x[0] + W[:, 1, i] * x[1]) + W[:, 2, i] * x[2])
                                                   + W[:, 3, i] * x[3]) + W[:, 4, i] * x[4]) for i in range(3)], 1)
                        Xn = np.stack([Xu[:, i] - ((Vi[:, i, 0] * h[:, 0] + Vi[:, i, 1] * h[:, 1]) + Vi[:, i, 2] * h[:, 2])
                                       for i in range(3)], 1)
                        rn, _, _, good = residual(Rn, tn, fi, fj, Xn, bu)
                        full = np.zeros(len(X))
                        full[used] = squares(rn)
                        cn = 0.5 * block_sum(full, used)
                        ok = bool(good.all()) and bool(np.isfinite(cn)) and bool(cn < c) and bool((c - cn) / model > 1e-3)
                if ok:
                    stop = lm.accepted(c, cn, model)
                    c, moved, R, t, Xu = cn, True, Rn, tn, Xn
                    B = basis(t)
                else:
                    stop = lm.rejected(c, model)
            out["status"] = 4 if not moved else 1 if stop else 3
            if not finite0:
                c = c0 = np.float64(0.0)
            out.update(steps=steps, cost_initial=float(c0), cost=float(c))
    out.update(R=R, t=t, E=essential(R, t))
    return out


def refine_relative_poses(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j,
                          rel_R, rel_t, inl_off, inl_idx, use_pair=None, **options):
    """The whole call, capi.RelRefine's arguments -> list of refine_pair() results in the order of `pairs`"""
    o = dict(OPTIONS, **options)
    view_off = np.asarray(view_off, np.int64)
    kpt_xy = np.asarray(kpt_xy, np.float32).reshape(-1, 2)
    intrinsics = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    rel_R, rel_t = np.asarray(rel_R, np.float64).reshape(-1, 9), np.asarray(rel_t, np.float64).reshape(-1, 3)
    out = []
    for k, (vi, vj) in enumerate(pairs):
        use = use_pair is None or bool(use_pair[k])
        b = np.zeros((0, 4))
        ii, ij = int(view_intrinsic[vi]), int(view_intrinsic[vj])
        if use:
            pos = int(offsets[k]) + np.asarray(inl_idx[int(inl_off[k]):int(inl_off[k + 1])], np.int64)
            ri = int(view_off[vi]) + np.asarray(match_i, np.int64)[pos]
            rj = int(view_off[vj]) + np.asarray(match_j, np.int64)[pos]
            b = np.concatenate([bearings(kpt_xy[ri], intrinsics[ii], intrinsic_type[ii]),
                                bearings(kpt_xy[rj], intrinsics[ij], intrinsic_type[ij])], 1)
        out.append(refine_pair(rel_R[k], rel_t[k], b, intrinsics[ii, 0], intrinsics[ij, 0], use, o["max_steps"],
                               o["min_points"]))
    return out
