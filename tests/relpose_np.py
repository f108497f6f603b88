"""NumPy restatement of sfmloc_relative_poses (include/sfmloc.h "Relative poses", csrc/relpose.hip,
csrc/essential_device.h): the bearings, the sampler, the five-point solver (null space by the fixed-sweep Jacobi, the ten
cubic constraints, Gauss-Jordan, the 3 x 3 polynomial matrix in z, the Sturm chain, bisection and Newton), the residual,
AC-RANSAC's acceptance rule with its NFA, the decomposition and the cheirality count.  Only + - * / sqrt in f64, elementwise
and in the stated order (NumPy does not fuse), vectorised over hypotheses: the results are the device's bits."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from adjust_np import ud_pixel_k3  # noqa: E402
from merge_np import jacobi_fixed, philox4x32_10  # noqa: E402
from resect6_np import FLT_EPSILON, det_log10, logcombi_tables  # noqa: E402

STAGE_RELPOSE = 6
S = 5                       # sample size
MAX_MODELS = 10
RANK_TOL = 1e-12            # no model when the fifth smallest eigenvalue of G <= this * the largest
PIVOT_FLOOR = 1e-13         # no model when a Gauss-Jordan pivot is not larger in magnitude
BISECT = 48
NEWTON = 3
POLISH = 2
SEED = 0x5F3759DF12345678
MAX_LDS_M = 2048            # matches the LDS form holds (forms.h kFMaxM)

VAR = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]
QUAD = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (1, 0, 0), (0, 2, 0), (0, 1, 1), (0, 1, 0), (0, 0, 2), (0, 0, 1), (0, 0, 0)]
CUBE = [(3, 0, 0), (0, 3, 0), (2, 1, 0), (1, 2, 0), (2, 0, 1), (2, 0, 0), (0, 2, 1), (0, 2, 0), (1, 1, 1), (1, 1, 0),
        (1, 0, 2), (1, 0, 1), (1, 0, 0), (0, 1, 2), (0, 1, 1), (0, 1, 0), (0, 0, 3), (0, 0, 2), (0, 0, 1), (0, 0, 0)]


def _add(a, b):
    return tuple(x + y for x, y in zip(a, b))


IDX2 = [[QUAD.index(_add(VAR[p], VAR[q])) for q in range(4)] for p in range(4)]
IDX3 = [[CUBE.index(_add(QUAD[m], VAR[p])) for p in range(4)] for m in range(10)]


def sample5(n, seed, view_i, view_j, iters):
    """rp_sample5 (csrc/relpose.hip): five distinct sorted positions in [0, n) per iteration; the Philox counter is
    (iteration, I, J, STAGE_RELPOSE | (draw >> 2) << 8), the key the seed's two halves -> int64 [len(iters), 5]"""
    iters = np.asarray(iters, np.uint64)
    z = np.zeros_like(iters)
    blocks = [philox4x32_10((iters, z + np.uint64(view_i), z + np.uint64(view_j), z + np.uint64(STAGE_RELPOSE | (b << 8))),
                            seed & 0xFFFFFFFF, seed >> 32) for b in range(2)]
    s = np.zeros((len(iters), S), np.int64)
    for i in range(S):
        r = (blocks[i >> 2][i & 3] % np.uint64(n - i)).astype(np.int64)
        j = np.zeros(len(iters), np.int64)
        for k in range(i):
            go = (j == k) & (r >= s[:, k])
            r = r + go
            j = j + go
        for k in range(i, 0, -1):
            s[:, k] = np.where(k > j, s[:, k - 1], s[:, k])
        for k in range(i + 1):
            s[:, k] = np.where(j == k, r, s[:, k])
    return s


# ---- the five-point solver ---------------------------------------------------------------------------------------------

def _mul11(q, a, b):
    """q [B, 10] += the product of two linear forms a, b [B, 4] (x, y, z, 1), terms added in the order p, q"""
    q = q.copy()
    for p in range(4):
        for r in range(4):
            q[:, IDX2[p][r]] = q[:, IDX2[p][r]] + a[:, p] * b[:, r]
    return q


def _mul21(c, q, a):
    """c [B, 20] += a quadratic q [B, 10] times a linear form a [B, 4], terms added in the order m, p"""
    c = c.copy()
    for m in range(10):
        for p in range(4):
            c[:, IDX3[m][p]] = c[:, IDX3[m][p]] + q[:, m] * a[:, p]
    return c


def _pm(a, b):
    """the product of two polynomials in z (coefficient i = z^i), terms added in the order i, j from 0.0"""
    c = np.zeros((a.shape[0], a.shape[1] + b.shape[1] - 1))
    for i in range(a.shape[1]):
        for j in range(b.shape[1]):
            c[:, i + j] = c[:, i + j] + a[:, i] * b[:, j]
    return c


def _horner(p, deg, x):
    """p [..., >= deg + 1] at x, from the leading coefficient down"""
    v = p[..., deg]
    for i in range(deg - 1, -1, -1):
        v = v * x + p[..., i]
    return v


def null_space(x1, x2):
    """x1, x2 [B, 5, 2] bearings of views I and J -> (N [B, 4, 9]: X, Y, Z, W, rank_ok [B])"""
    B = x1.shape[0]
    a, b, u, v = x1[:, :, 0], x1[:, :, 1], x2[:, :, 0], x2[:, :, 1]
    one = np.ones_like(a)
    D = np.stack([u * a, u * b, u, v * a, v * b, v, a, b, one], 2)          # [B, 5, 9]
    G = D[:, 0, :, None] * D[:, 0, None, :]
    for r in range(1, 5):
        G = G + D[:, r, :, None] * D[:, r, None, :]
    d, V = jacobi_fixed([[G[:, i, j] for j in range(9)] for i in range(9)])
    d = np.stack(d, 1)
    V = np.stack([np.stack(row, 1) for row in V], 1)                        # [B, 9 (component), 9 (column)]
    taken = np.zeros((B, 9), bool)
    N = np.zeros((B, 4, 9))
    dsel = None
    for t in range(5):                                                      # the smallest untaken diagonal, first on ties
        best = np.full(B, np.inf)
        ib = np.full(B, -1, np.int64)
        for i in range(9):
            take = ~taken[:, i] & ((ib < 0) | (d[:, i] < best))
            best = np.where(take, d[:, i], best)
            ib = np.where(take, i, ib)
        taken[np.arange(B), ib] = True
        if t < 4:
            N[:, t, :] = V[np.arange(B), :, ib]
        else:
            dsel = best
    dmax = d[:, 0]
    for i in range(1, 9):
        dmax = np.where(d[:, i] > dmax, d[:, i], dmax)
    return N, dsel > RANK_TOL * dmax


def constraints(N):
    """N [B, 4, 9] -> M [B, 10, 20]: row 0 det E, row 1 + 3 i + j the (i, j) entry of (E E^T - tr(E E^T) / 2) E"""
    B = N.shape[0]
    E = [[np.stack([N[:, t, 3 * i + j] for t in range(4)], 1) for j in range(3)] for i in range(3)]
    z10, z20 = np.zeros((B, 10)), np.zeros((B, 20))
    M = np.zeros((B, 10, 20))
    q1 = _mul11(z10, E[1][1], E[2][2]) - _mul11(z10, E[1][2], E[2][1])
    q2 = _mul11(z10, E[1][0], E[2][2]) - _mul11(z10, E[1][2], E[2][0])
    q3 = _mul11(z10, E[1][0], E[2][1]) - _mul11(z10, E[1][1], E[2][0])
    M[:, 0, :] = (_mul21(z20, q1, E[0][0]) - _mul21(z20, q2, E[0][1])) + _mul21(z20, q3, E[0][2])
    EEt = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            q = z10
            for k in range(3):
                q = _mul11(q, E[i][k], E[j][k])
            EEt[i][j] = q
    half = 0.5 * ((EEt[0][0] + EEt[1][1]) + EEt[2][2])
    for i in range(3):
        for j in range(3):
            c = z20
            for k in range(3):
                c = _mul21(c, EEt[i][k] - half if i == k else EEt[i][k], E[k][j])
            M[:, 1 + 3 * i + j, :] = c
    return M


def gauss_jordan(M):
    """M [B, 10, 20] -> (reduced M, ok): partial pivoting, the largest magnitude (the first on ties)"""
    M = M.copy()
    B = M.shape[0]
    ok = np.ones(B, bool)
    ar = np.arange(B)
    with np.errstate(all="ignore"):
        for c in range(10):
            pr = np.full(B, c, np.int64)
            pa = np.abs(M[:, c, c])
            for r in range(c + 1, 10):
                av = np.abs(M[:, r, c])
                take = av > pa
                pa = np.where(take, av, pa)
                pr = np.where(take, r, pr)
            ok &= pa > PIVOT_FLOOR
            rc, rp = M[ar, c, :].copy(), M[ar, pr, :].copy()
            M[ar, pr, :] = rc
            M[ar, c, :] = rp
            piv = M[:, c, c].copy()
            M[:, c, :] = M[:, c, :] / piv[:, None]
            for r in range(10):
                if r != c:
                    f = M[:, r, c].copy()
                    M[:, r, :] = M[:, r, :] - f[:, None] * M[:, c, :]
    return M, ok


def _brow(M, a, b):
    """rows a (leading x^2 z, y^2 z or x y z) and b (x^2, y^2, x y) -> a - z b as (x part [B, 4], y part [B, 4], 1 part [B, 5])"""
    ea, eb = M[:, a, :], M[:, b, :]
    out = []
    for o in (10, 13):
        out.append(np.stack([ea[:, o + 2], ea[:, o + 1] - eb[:, o + 2], ea[:, o] - eb[:, o + 1], -eb[:, o]], 1))
    out.append(np.stack([ea[:, 19], ea[:, 18] - eb[:, 19], ea[:, 17] - eb[:, 18], ea[:, 16] - eb[:, 17], -eb[:, 16]], 1))
    return out


def _sign_changes(chain, x):
    """chain [B, 11, 11], x [B, R] -> the number of sign changes of the chain at x, zeros (and NaN) skipped"""
    cnt = np.zeros(x.shape, np.int64)
    last = np.zeros(x.shape, np.int64)
    for i in range(11):
        v = _horner(chain[:, i, None, :], 10 - i, x)
        s = np.where(v > 0.0, 1, np.where(v < 0.0, -1, 0))
        cnt = cnt + ((s != 0) & (last != 0) & (s != last))
        last = np.where(s != 0, s, last)
    return cnt


def _maxabs(p):
    m = np.abs(p[:, 0])
    for i in range(1, p.shape[1]):
        a = np.abs(p[:, i])
        m = np.where(a > m, a, m)
    return m


def five_point(x1, x2, trace=None):
    """x1, x2 [B, 5, 2] -> (nm [B], E [B, 10, 9]): the models in ascending order of the root z, unit Frobenius norm"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    B = x1.shape[0]
    with np.errstate(all="ignore"):
        N, ok = null_space(x1, x2)
        M, ok2 = gauss_jordan(constraints(N))
        ok = ok & ok2
        k, l, m = _brow(M, 4, 5), _brow(M, 6, 7), _brow(M, 8, 9)
        t1 = _pm(l[1], m[2]) - _pm(l[2], m[1])
        t2 = _pm(l[0], m[2]) - _pm(l[2], m[0])
        t3 = _pm(l[0], m[1]) - _pm(l[1], m[0])
        p = (_pm(k[0], t1) - _pm(k[1], t2)) + _pm(k[2], t3)                 # [B, 11]
        # the Sturm chain, every member divided by its largest magnitude
        chain = np.zeros((B, 11, 11))
        chain[:, 0, :] = p / _maxabs(p)[:, None]
        dp = np.stack([float(i + 1) * chain[:, 0, i + 1] for i in range(10)], 1)
        chain[:, 1, :10] = dp / _maxabs(dp)[:, None]
        for i in range(1, 10):
            n = 11 - i                                                       # deg chain[i - 1] = n, deg chain[i] = n - 1
            a, b = chain[:, i - 1, :n + 1], chain[:, i, :n]
            q1 = a[:, n] / b[:, n - 1]
            a1 = a[:, :n].copy()
            a1[:, 1:] = a1[:, 1:] - q1[:, None] * b[:, :n - 1]
            q0 = a1[:, n - 1] / b[:, n - 1]
            r = -(a1[:, :n - 1] - q0[:, None] * b[:, :n - 1])
            chain[:, i + 1, :n - 1] = r / _maxabs(r)[:, None]
        p0 = chain[:, 0, :]
        if trace is not None:
            trace['chain'] = chain.copy()
        bound = np.abs(p0[:, 0] / p0[:, 10])
        for i in range(1, 10):
            a = np.abs(p0[:, i] / p0[:, 10])
            bound = np.where(a > bound, a, bound)
        bound = 1.0 + bound
        vlo = _sign_changes(chain, -bound[:, None])[:, 0]
        nr = vlo - _sign_changes(chain, bound[:, None])[:, 0]
        kk = np.arange(10)[None, :]
        lo = np.repeat(-bound[:, None], 10, 1)
        hi = np.repeat(bound[:, None], 10, 1)
        for _ in range(BISECT):
            mid = 0.5 * (lo + hi)
            c = vlo[:, None] - _sign_changes(chain, mid)
            up = c >= kk + 1
            hi = np.where(up, mid, hi)
            lo = np.where(up, lo, mid)
        z = 0.5 * (lo + hi)
        for _ in range(NEWTON):
            f = _horner(p0[:, None, :], 10, z)
            df = _horner(dp[:, None, :], 9, z)
            zn = z - f / df
            z = np.where((zn >= lo) & (zn <= hi), zn, z)
        if trace is not None:
            trace['z_newton'] = z.copy()
        # two more Newton steps on det B(z) taken from the matrix itself (the expanded coefficients of p have lost digits
        # to cancellation; the matrix has not), each kept when it moves z by at most 1e-6 (1 + |z|)
        def at(z):
            return [[_horner(r[0][:, None, :], 3, z), _horner(r[1][:, None, :], 3, z), _horner(r[2][:, None, :], 4, z)]
                    for r in (k, l, m)]

        def det3(a, b, c):
            return (a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0])) \
                + a[2] * (b[0] * c[1] - b[1] * c[0])
        dk = [[np.stack([float(i + 1) * q[:, i + 1] for i in range(q.shape[1] - 1)], 1) for q in r] for r in (k, l, m)]
        for _ in range(POLISH):
            rows = at(z)
            drows = [[_horner(r[0][:, None, :], 2, z), _horner(r[1][:, None, :], 2, z), _horner(r[2][:, None, :], 3, z)]
                     for r in dk]
            f = det3(rows[0], rows[1], rows[2])
            df = (det3(drows[0], rows[1], rows[2]) + det3(rows[0], drows[1], rows[2])) + det3(rows[0], rows[1], drows[2])
            zn = z - f / df
            z = np.where(np.abs(zn - z) <= 1e-6 * (1.0 + np.abs(z)), zn, z)
        if trace is not None:
            trace['z'] = z.copy()
        # x and y from the null vector of the polynomial matrix at z: the cross product with the largest third entry
        rows = at(z)
        best = None
        for ra, rb in ((0, 1), (0, 2), (1, 2)):
            A_, B_ = rows[ra], rows[rb]
            n0 = A_[1] * B_[2] - A_[2] * B_[1]
            n1 = A_[2] * B_[0] - A_[0] * B_[2]
            n2 = A_[0] * B_[1] - A_[1] * B_[0]
            if best is None:
                best = [n0, n1, n2]
            else:
                take = np.abs(n2) > np.abs(best[2])
                best = [np.where(take, n0, best[0]), np.where(take, n1, best[1]), np.where(take, n2, best[2])]
        x, y = best[0] / best[2], best[1] / best[2]
        E = ((x[:, :, None] * N[:, None, 0, :] + y[:, :, None] * N[:, None, 1, :]) + z[:, :, None] * N[:, None, 2, :]) \
            + N[:, None, 3, :]
        ss = E[:, :, 0] * E[:, :, 0]
        for i in range(1, 9):
            ss = ss + E[:, :, i] * E[:, :, i]
        E = E / np.sqrt(ss)[:, :, None]
        valid = ok[:, None] & (kk < nr[:, None]) & np.isfinite(E).all(2)
    nm = valid.sum(1)
    out = np.zeros((B, 10, 9))
    for b in range(B):
        out[b, :nm[b]] = E[b, valid[b]]
    return nm, out


# ---- the stage ---------------------------------------------------------------------------------------------------------

def bearings(kpt_xy, K, ktype):
    """pixels [n, 2] (float32) of one view -> bearings [n, 2]: ud_pixel_k3 for type 3, then ((x - ppx) / f, (y - ppy) / f)"""
    xy = np.asarray(kpt_xy, np.float32).astype(np.float64).reshape(-1, 2)
    ud = xy.copy()
    if int(ktype) == 3:
        for o in range(len(xy)):
            ud[o] = ud_pixel_k3(*[float(t) for t in K], float(xy[o, 0]), float(xy[o, 1]))
    return np.stack([(ud[:, 0] - K[1]) / K[0], (ud[:, 1] - K[2]) / K[0]], 1)


def residuals(E, b1, b2, fj):
    """err_fmatrix of one model over all matches on bearings, times f_J^2 (NaN -> inf)"""
    with np.errstate(all="ignore"):
        x, y, u, v = b1[:, 0], b1[:, 1], b2[:, 0], b2[:, 1]
        l0 = (E[0] * x + E[1] * y) + E[2]
        l1 = (E[3] * x + E[4] * y) + E[5]
        l2 = (E[6] * x + E[7] * y) + E[8]
        num = (l0 * u + l1 * v) + l2
        e = (num * num) / (l0 * l0 + l1 * l1)
        e = np.where(np.isnan(e), np.inf, e)
        return e * (fj * fj)


def decompose(E):
    """E [9] -> (R [4, 9], t [4, 3]): the four candidates (Ra, +t), (Ra, -t), (Rb, +t), (Rb, -t)"""
    E = np.asarray(E, np.float64)
    with np.errstate(all="ignore"):
        A = [[(E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j] for j in range(3)] for i in range(3)]
        d, V = jacobi_fixed([[np.array([A[i][j]]) for j in range(3)] for i in range(3)])
        d = [float(t[0]) for t in d]
        V = np.array([[float(V[i][j][0]) for j in range(3)] for i in range(3)])
        i1 = 0
        for i in (1, 2):
            if d[i] > d[i1]:
                i1 = i
        i2 = -1
        for i in range(3):
            if i != i1 and (i2 < 0 or d[i] > d[i2]):
                i2 = i
        v1, v2 = V[:, i1], V[:, i2]
        s1, s2 = np.sqrt(np.float64(d[i1])), np.sqrt(np.float64(d[i2]))
        u1 = np.array([((E[3 * i] * v1[0] + E[3 * i + 1] * v1[1]) + E[3 * i + 2] * v1[2]) / s1 for i in range(3)])
        u2 = np.array([((E[3 * i] * v2[0] + E[3 * i + 1] * v2[1]) + E[3 * i + 2] * v2[2]) / s2 for i in range(3)])

        def cross(a, b):
            return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])
        v3 = cross(v1, v2)
        u3 = cross(u1, u2)
        u3 = u3 / np.sqrt((u3[0] * u3[0] + u3[1] * u3[1]) + u3[2] * u3[2])
        Ra = np.array([(u2[i] * v1[j] - u1[i] * v2[j]) + u3[i] * v3[j] for i in range(3) for j in range(3)])
        Rb = np.array([(u1[i] * v2[j] - u2[i] * v1[j]) + u3[i] * v3[j] for i in range(3) for j in range(3)])
    return np.stack([Ra, Ra, Rb, Rb]), np.stack([u3, -u3, u3, -u3])


def front_count(R, t, b1, b2):
    """the matches whose two-view point (csrc/triangulate.hip's hypothesis from [I | 0] and [R | t] on bearings) has
    positive depth in both views -> (count, mask)"""
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
        mask = ok & (X[:, 2] > 0.0) & (zj > 0.0)
    return int(mask.sum()), mask


def pair(b1, b2, wh_j, fj, view_i, view_j, max_iteration=256, precision_px=2.5, seed=SEED):
    """One pair on its matches' bearings b1, b2 [m, 2] -> dict with the fields of sfmloc_relpose_result and `inliers`"""
    m = len(b1)
    res = dict(ok=0, n_matches=m, n_inliers=0, sample=np.zeros(5, np.int64), front=np.zeros(4, np.int64), choice=0,
               E=np.zeros(9), R=np.zeros(9), t=np.zeros(3), error_max_px=0.0, nfa=0.0, inliers=np.zeros(0, np.int64),
               rounds=0)
    if m <= S:
        return res
    w, h = float(wh_j[0]), float(wh_j[1])
    Dg = np.sqrt(np.float64(w * w + h * h))
    logalpha0 = float(det_log10(np.array([2.0 * Dg / (w * h)]))[0])
    loge0 = float(det_log10(np.array([10.0 * float(m - S)]))[0])
    with np.errstate(all="ignore"):
        max_thr = np.float64(precision_px) * np.float64(precision_px)
    logc_n, logc_k = logcombi_tables(S, m)
    tail = logc_n[S + 1:].astype(np.float64), logc_k[S + 1:].astype(np.float64)
    kk = np.arange(S + 1, m + 1)
    kms = (kk - S).astype(np.float64)
    vec_index = np.arange(m)
    n_index = m
    min_nfa, errmax, n_in = np.inf, np.inf, 0
    inl = np.zeros(0, np.int64)
    model, smp_best = np.zeros(9), np.zeros(5, np.int64)
    n_iter = int(max_iteration)
    n_reserve = n_iter // 10
    n_iter -= n_reserve
    it = 0
    batch_it0, batch_nm = 0, None
    while it < n_iter:
        if batch_nm is None or it >= batch_it0 + len(batch_nm):
            cnt = min(64, n_iter - it)
            smp = vec_index[sample5(n_index, seed, view_i, view_j, np.arange(it, it + cnt))]
            batch_nm, batch_E = five_point(b1[smp], b2[smp])
            batch_smp, batch_it0 = smp, it
        b = it - batch_it0
        better = False
        for k in range(batch_nm[b]):
            E = batch_E[b, k]
            e = residuals(E, b1, b2, fj)
            order = np.argsort(e, kind="stable")
            es = e[order]
            with np.errstate(all="ignore"):
                logalpha = logalpha0 + 0.5 * det_log10(es[S:] + FLT_EPSILON)
                nfa = ((loge0 + logalpha * kms) + tail[0]) + tail[1]
                nfa = np.where(es[S:] <= max_thr, nfa, np.inf)
            j = int(np.argmin(nfa))
            if nfa[j] < min_nfa:
                better = True
                min_nfa = float(nfa[j])
                n_in = int(kk[j])
                inl = order[:n_in].copy()
                errmax = float(es[n_in - 1])
                model, smp_best = E.copy(), batch_smp[b].copy()
        if (better and min_nfa < 0.0) or (it + 1 == n_iter and n_reserve):
            if n_in == 0:
                n_iter += 1
                n_reserve -= 1
            else:
                vec_index = inl.copy()
                n_index = n_in
                batch_nm = None
                if n_reserve:
                    n_iter = it + 1 + n_reserve
                    n_reserve = 0
        it += 1
    res["rounds"] = it
    res["nfa"] = min_nfa
    if not min_nfa < 0.0:
        return res
    R4, t4 = decompose(model)
    front = np.array([front_count(R4[c], t4[c], b1[inl], b2[inl])[0] for c in range(4)], np.int64)
    choice = 0
    for c in range(1, 4):
        if front[c] > front[choice]:
            choice = c
    res.update(n_inliers=n_in, inliers=inl, sample=smp_best, E=model, front=front, choice=choice, R=R4[choice],
               t=t4[choice], error_max_px=float(np.sqrt(np.float64(errmax))),
               ok=int(float(n_in) > 2.5 * S and front[choice] > 0))
    return res


def relative_poses(view_off, kpt_xy, view_wh, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i,
                   match_j, max_iteration=256, precision_px=2.5, seed=SEED):
    """The whole call -> list of pair() results, in the order of `pairs`"""
    view_off = np.asarray(view_off, np.int64)
    kpt_xy = np.asarray(kpt_xy, np.float32).reshape(-1, 2)
    intrinsics = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    cache = {}

    def view_bearings(v):
        if v not in cache:
            ii = int(view_intrinsic[v])
            cache[v] = bearings(kpt_xy[view_off[v]:view_off[v + 1]], intrinsics[ii], intrinsic_type[ii])
        return cache[v]
    out = []
    for k, (vi, vj) in enumerate(pairs):
        s = slice(int(offsets[k]), int(offsets[k + 1]))
        b1 = view_bearings(int(vi))[np.asarray(match_i[s], np.int64)]
        b2 = view_bearings(int(vj))[np.asarray(match_j[s], np.int64)]
        fj = np.float64(intrinsics[int(view_intrinsic[vj]), 0])
        out.append(pair(b1, b2, np.asarray(view_wh, np.int64).reshape(-1, 2)[vj], fj, int(vi), int(vj), max_iteration,
                        precision_px, seed))
    return out
