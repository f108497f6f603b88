"""NumPy restatement of the uncalibrated query's resection (include/sfmloc.h "Uncalibrated queries", csrc/acransac.hip
"resect6"): the conditioning N1, the sampler, the 12 x 12 design matrix, the fixed-sweep Jacobi, the sign and rank
rules, AC-RANSAC's sequential acceptance rule with its NFA, the un-normalisation, the gates and KRt_From_P.  Only
+ - * / sqrt in f64, elementwise and in the stated order (NumPy does not fuse), vectorised over hypotheses: the results
are the device's bits.  KRt_From_P and the centre are the C oracle's (oracle/sfm_oracle_geom.c), whose bits the device's
are tested against elsewhere (tests/test_gpu_geom.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from merge_np import philox4x32_10  # noqa: E402

STAGE_RESECT6 = 4
SWEEPS = 10
RANK_TOL = 1e-12
S = 6                      # sample size; one model per sample
FLT_EPSILON = float(np.finfo(np.float32).eps)
BATCH = 256                # hypotheses solved together (any partition gives the same result)


def det_log10(x):
    """geom_device.h det_log10 over an array of non-negative doubles (0 -> -inf, inf -> inf)"""
    x = np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        sub = (x.view(np.uint64) >> np.uint64(52)) & np.uint64(0x7FF)
        xs = np.where(sub == 0, x * 18014398509481984.0, x)
        u = xs.view(np.uint64)
        e = ((u >> np.uint64(52)) & np.uint64(0x7FF)).astype(np.int64) - np.where(sub == 0, 54, 0) - 1023
        m = ((u & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(0x3FF0000000000000)).view(np.float64)
        big = m > 1.4142135623730951
        m = np.where(big, m * 0.5, m)
        e = e + big
        z = (m - 1.0) / (m + 1.0)
        z2 = z * z
        p = np.full_like(z, 1.0 / 23.0)
        for d in (21.0, 19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0):
            p = p * z2 + 1.0 / d
        p = p * z2 + 1.0
        ln = e.astype(np.float64) * 0.6931471805599453 + (2.0 * z) * p
        out = ln * 0.4342944819032518
    out = np.where(x == 0.0, -np.inf, out)
    out = np.where(np.isinf(x), np.inf, out)
    return np.where(np.isnan(x) | (x < 0.0), np.nan, out)


def logcombi_tables(s, n):
    """orc_logcombi_tables: logc_n[k] = log10 C(n, k), logc_k[m] = log10 C(m, s), float32, k and m in 0 .. n"""
    L10 = np.zeros(n + 2)
    L10[1:] = det_log10(np.arange(1, n + 2, dtype=np.float64))
    i = np.arange(1, n + 1)
    c = np.concatenate([[0.0], np.cumsum(L10[n - i + 1] - L10[i])])      # c[j] = the sum's first j terms, in order
    k = np.arange(n + 1)
    logc_n = np.where((k >= n) | (k <= 0), 0.0, c[np.minimum(k, n - k)]).astype(np.float32)
    m = np.arange(n + 1)
    kk = np.minimum(s, m - s)
    r = np.zeros(n + 1)
    for j in range(1, s + 1):
        r = np.where(j <= kk, r + (L10[np.maximum(m - j + 1, 0)] - L10[j]), r)
    logc_k = np.where((s >= m) | (s <= 0), 0.0, r).astype(np.float32)
    return logc_n, logc_k


def sample(X, n, seed, stage, stream, iters):
    """ac_sample<X> (geom_device.h) for every iteration in `iters` -> int64 [len(iters), X] sorted positions in [0, n)"""
    iters = np.asarray(iters, np.uint64)
    z = np.zeros_like(iters)
    blocks = [philox4x32_10((iters, z + np.uint64(stream), z + np.uint64(b), z + np.uint64(stage)), seed & 0xFFFFFFFF,
                            seed >> 32) for b in range((X + 3) // 4)]
    s = np.zeros((len(iters), X), np.int64)
    for i in range(X):
        r = (blocks[i >> 2][i & 3] % np.uint64(n - i)).astype(np.int64)
        j = np.zeros(len(iters), np.int64)
        for k in range(i):                      # for (j = 0; j < i && r >= s[j]; ++j) ++r;
            go = (j == k) & (r >= s[:, k])
            r = r + go
            j = j + go
        for k in range(i, 0, -1):
            s[:, k] = np.where(k > j, s[:, k - 1], s[:, k])
        for k in range(i + 1):
            s[:, k] = np.where(j == k, r, s[:, k])
    return s


def jacobi12(G):
    """G [B, 12, 12] symmetric -> (G after SWEEPS cyclic sweeps, V); the rotation of merge_np.jacobi_fixed"""
    G = np.array(G, np.float64)
    B, N = G.shape[0], G.shape[1]
    V = np.zeros_like(G)
    V[:, np.arange(N), np.arange(N)] = 1.0
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(N - 1):
                for q in range(p + 1, N):
                    apq = G[:, p, q]
                    skip = apq == 0.0
                    theta = (G[:, q, q] - G[:, p, p]) / (2.0 * apq)
                    at = np.where(theta < 0.0, -theta, theta)
                    t = np.where(theta < 0.0, -1.0, 1.0) / (at + np.sqrt(theta * theta + 1.0))
                    c = (1.0 / np.sqrt(t * t + 1.0))[:, None]
                    s = t[:, None] * c
                    sk = skip[:, None]
                    akp, akq = G[:, :, p].copy(), G[:, :, q].copy()
                    G[:, :, p] = np.where(sk, akp, c * akp - s * akq)
                    G[:, :, q] = np.where(sk, akq, s * akp + c * akq)
                    apk, aqk = G[:, p, :].copy(), G[:, q, :].copy()
                    G[:, p, :] = np.where(sk, apk, c * apk - s * aqk)
                    G[:, q, :] = np.where(sk, aqk, s * apk + c * aqk)
                    G[:, p, q] = np.where(skip, G[:, p, q], 0.0)
                    G[:, q, p] = np.where(skip, G[:, q, p], 0.0)
                    vkp, vkq = V[:, :, p].copy(), V[:, :, q].copy()
                    V[:, :, p] = np.where(sk, vkp, c * vkp - s * vkq)
                    V[:, :, q] = np.where(sk, vkq, s * vkp + c * vkq)
    return G, V


def design(x, X):
    """x [B, 6, 2] normalised image points, X [B, 6, 3] -> D [B, 12, 12] (3D points translated by -X[:, 0])"""
    B = x.shape[0]
    Xt = X - X[:, :1, :]
    D = np.zeros((B, 12, 12))
    for i in range(6):
        for par in range(2):
            r, o, u = 2 * i + par, 4 * par, x[:, i, par]
            D[:, r, o:o + 3] = Xt[:, i, :]
            D[:, r, o + 3] = 1.0
            D[:, r, 8:11] = -(u[:, None] * Xt[:, i, :])
            D[:, r, 11] = -u
    return D


def solve(x, X):
    """resect6_solve_wave for B hypotheses: x [B, 6, 2], X [B, 6, 3] -> (nm [B] in {0, 1}, M [B, 12])"""
    x, X = np.asarray(x, np.float64), np.asarray(X, np.float64)
    B = x.shape[0]
    D = design(x, X)
    with np.errstate(all="ignore"):
        G = D[:, 0, :, None] * D[:, 0, None, :]
        for r in range(1, 12):
            G = G + D[:, r, :, None] * D[:, r, None, :]
        G, V = jacobi12(G)
        d = G[:, np.arange(12), np.arange(12)]
        imin = np.zeros(B, np.int64)
        dmin = d[:, 0].copy()
        dmax = d[:, 0].copy()
        for i in range(1, 12):
            less = d[:, i] < dmin
            dmin = np.where(less, d[:, i], dmin)
            imin = np.where(less, i, imin)
            dmax = np.where(d[:, i] > dmax, d[:, i], dmax)
        dsec = np.full(B, np.inf)
        for i in range(12):
            take = (imin != i) & (d[:, i] < dsec)
            dsec = np.where(take, d[:, i], dsec)
        P = V[np.arange(B), :, imin].copy()
        X0 = X[:, 0, :]
        for r in range(3):
            P[:, 4 * r + 3] = P[:, 4 * r + 3] - ((P[:, 4 * r] * X0[:, 0] + P[:, 4 * r + 1] * X0[:, 1])
                                                 + P[:, 4 * r + 2] * X0[:, 2])
        behind = np.zeros(B, np.int64)
        for i in range(6):
            w = ((P[:, 8] * X[:, i, 0] + P[:, 9] * X[:, i, 1]) + P[:, 10] * X[:, i, 2]) + P[:, 11]
            behind = behind + (w < 0.0)
        ok = (dsec > RANK_TOL * dmax) & np.isfinite(P).all(axis=1)
        M = np.where((behind > 3)[:, None], -P, P)
    return ok.astype(np.int64), M


def residuals(M, xn, X):
    """err_resection of one model over all points"""
    with np.errstate(all="ignore"):
        p0 = ((M[0] * X[:, 0] + M[1] * X[:, 1]) + M[2] * X[:, 2]) + M[3]
        p1 = ((M[4] * X[:, 0] + M[5] * X[:, 1]) + M[6] * X[:, 2]) + M[7]
        p2 = ((M[8] * X[:, 0] + M[9] * X[:, 1]) + M[10] * X[:, 2]) + M[11]
        dx = p0 / p2 - xn[:, 0]
        dy = p1 / p2 - xn[:, 1]
        e = dx * dx + dy * dy
    return np.where(np.isnan(e), np.inf, e)


def normalize(pt2d, width, height):
    """N1 of the image -> (xn, f, ppx, ppy)"""
    f = np.sqrt(np.float64(width) * np.float64(height))
    ppx, ppy = 0.5 * np.float64(width), 0.5 * np.float64(height)
    inv_f = 1.0 / f
    cx, cy = -ppx * inv_f, -ppy * inv_f
    pt2d = np.asarray(pt2d, np.float64).reshape(-1, 2)
    return np.stack([pt2d[:, 0] * inv_f + cx, pt2d[:, 1] * inv_f + cy], axis=1), f, ppx, ppy


def acransac(xn, X, max_iteration, seed, stream=0, trace=None):
    """The sequential AC-RANSAC (oracle/sfm_oracle_geom.c acransac) with the six-point kernel.
    -> dict(n_in, inliers, model, errmax, nfa, iterations); trace, when a list, receives (iteration, the model's best
    NFA, the sample) of every model evaluated (for the tests' tie check)."""
    n = xn.shape[0]
    out = dict(n_in=0, inliers=np.zeros(0, np.int64), model=np.zeros(12), errmax=np.inf, nfa=np.inf, iterations=0)
    if n <= S:
        return out
    logalpha0 = float(det_log10(np.array([3.14159265358979323846]))[0])
    loge0 = float(det_log10(np.array([1.0 * float(n - S)]))[0])
    logc_n, logc_k = logcombi_tables(S, n)
    tail = logc_n[S + 1:].astype(np.float64), logc_k[S + 1:].astype(np.float64)
    kk = np.arange(S + 1, n + 1)
    kms = (kk - S).astype(np.float64)
    vec_index = np.arange(n)
    n_index = n
    min_nfa, errmax, n_in = np.inf, np.inf, 0
    inliers = np.zeros(0, np.int64)
    model = np.zeros(12)
    n_iter = int(max_iteration)
    n_reserve = n_iter // 10
    n_iter -= n_reserve
    it = 0
    batch_it0, batch_nm, batch_M = 0, None, None
    while it < n_iter:
        if batch_nm is None or it >= batch_it0 + len(batch_nm):
            cnt = min(BATCH, n_iter - it)
            pos = sample(S, n_index, seed, STAGE_RESECT6, stream, np.arange(it, it + cnt))
            smp = vec_index[pos]
            batch_nm, batch_M = solve(xn[smp], X[smp])
            batch_smp = smp
            batch_it0 = it
        b = it - batch_it0
        better = False
        if batch_nm[b]:
            M = batch_M[b]
            e = residuals(M, xn, X)
            order = np.argsort(e, kind="stable")            # (error, index) ascending
            es = e[order]
            with np.errstate(all="ignore"):
                logalpha = logalpha0 + 1.0 * det_log10(es[S:] + FLT_EPSILON)
                nfa = ((loge0 + logalpha * kms) + tail[0]) + tail[1]
            j = int(np.argmin(nfa)) if len(nfa) else 0       # the first minimum
            best_nfa = float(nfa[j]) if len(nfa) else np.inf
            if trace is not None:
                trace.append((it, best_nfa, tuple(int(v) for v in batch_smp[b])))
            if best_nfa < min_nfa:
                better = True
                min_nfa = best_nfa
                n_in = int(kk[j])
                inliers = order[:n_in].copy()
                errmax = float(es[n_in - 1])
                model = M.copy()
        if (better and min_nfa < 0.0) or (it + 1 == n_iter and n_reserve):
            if n_in == 0:
                n_iter += 1
                n_reserve -= 1
            else:
                vec_index = inliers.copy()
                n_index = n_in
                batch_nm = None                              # the coming samples draw from the new index set
                if n_reserve:
                    n_iter = it + 1 + n_reserve
                    n_reserve = 0
        it += 1
    out.update(iterations=it, nfa=min_nfa, errmax=errmax, model=model)
    if min_nfa < 0.0:
        out.update(n_in=n_in, inliers=inliers)
    return out


def localize(pt2d, pt3d, width, height, max_iteration=4096, min_resection_points=8, min_inliers=10,
             seed=0x5f3759df12345678, stream=0, trace=None):
    """The whole stage on n 2D-3D correspondences -> dict with the fields of sfmloc_pose the stage writes"""
    from oracle import oracle_c
    pt2d = np.asarray(pt2d, np.float64).reshape(-1, 2)
    X = np.asarray(pt3d, np.float64).reshape(-1, 3)
    n = pt2d.shape[0]
    res = dict(ok=0, n_inliers=0, n_matches_2d3d=n, iterations=0, nfa=0.0, error_max=0.0, P=np.zeros(12),
               K=np.zeros(9), R=np.zeros(9), t=np.zeros(3), center=np.zeros(3), inliers=np.zeros(0, np.int64))
    if n <= min_resection_points or n <= S:
        return res
    xn, f, ppx, ppy = normalize(pt2d, width, height)
    ac = acransac(xn, X, max_iteration, seed, stream, trace)
    n_final = ac["n_in"]
    M = ac["model"]
    P = np.zeros(12)
    if n_final > 0:
        for j in range(4):
            P[j] = f * M[j] + ppx * M[8 + j]
            P[4 + j] = f * M[4 + j] + ppy * M[8 + j]
            P[8 + j] = M[8 + j]
    inv_f = 1.0 / f
    ok = (float(n_final) > 2.5 * S) and n_final > min_inliers
    res.update(n_inliers=n_final, iterations=ac["iterations"], nfa=ac["nfa"], P=P,
               error_max=(np.sqrt(ac["errmax"]) / inv_f) if n_final > 0 else ac["errmax"])
    if ok:
        K, R, t, c = [np.asarray(v, np.float64).ravel() for v in oracle_c.krt_from_p(P)]
        res.update(ok=1, K=K, R=R, t=t, center=c, inliers=ac["inliers"])
    return res


def _rotate_left(w, R):
    """Exp(w) R by Rodrigues' formula (acransac.hip rotate_left)"""
    th2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    th = np.sqrt(th2)
    if th < 1e-8:
        a, b = 1.0 - th2 / 6.0, 0.5 - th2 / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / th2
    W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
    return (np.eye(3) + a * W + b * (W @ W)) @ R


def _normal_equations(pt2d, X, K, R, t):
    """[J | r]^T [J | r] (7 x 7) of the reprojection residuals under a fixed upper-triangular K with K[2, 2] = 1"""
    fx, sk, cx, fy, cy = K[0, 0], K[0, 1], K[0, 2], K[1, 1], K[1, 2]
    RX = X @ R.T
    Xc = RX + t
    iz = 1.0 / Xc[:, 2]
    num = fx * Xc[:, 0] + sk * Xc[:, 1]
    z = np.zeros(len(X))
    gu = np.stack([fx * iz, sk * iz, -num * iz * iz], 1)
    gv = np.stack([z, fy * iz, -fy * Xc[:, 1] * iz * iz], 1)
    ru = (num * iz + cx) - pt2d[:, 0]
    rv = (fy * Xc[:, 1] * iz + cy) - pt2d[:, 1]
    rows = []
    for g, r in ((gu, ru), (gv, rv)):
        rows.append(np.concatenate([np.cross(RX, g), g, r[:, None]], 1))      # d/dw = RX x g, d/dt = g, residual
    M = np.concatenate(rows, 0)
    return M.T @ M


def refine(pt2d, X, inliers, K, R, t, max_iter=20):
    """refine_pose_block under a general fixed K: Levenberg-Marquardt on R (left increment) and t over the inliers.
    Sums in NumPy's order, not the device's (matrix cores): equal within rounding, not bit for bit.
    -> (R, t, cost, iterations)"""
    pt2d = np.asarray(pt2d, np.float64).reshape(-1, 2)[inliers]
    X = np.asarray(X, np.float64).reshape(-1, 3)[inliers]
    K, R, t = np.asarray(K, np.float64).reshape(3, 3), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64)
    N = _normal_equations(pt2d, X, K, R, t)
    H, g, cost = N[:6, :6], N[:6, 6], N[6, 6]
    lam, it = 1e-4, 0
    while it < max_iter:
        A = H.copy()
        A[np.arange(6), np.arange(6)] = np.diag(H) * (1.0 + lam)
        try:
            d = np.linalg.solve(A, -g)
        except np.linalg.LinAlgError:
            break
        Rn, tn = _rotate_left(d[:3], R), t + d[3:]
        N = _normal_equations(pt2d, X, K, Rn, tn)
        c_new = N[6, 6]
        if c_new < cost:
            rel = (cost - c_new) / cost
            R, t, cost, H, g = Rn, tn, c_new, N[:6, :6], N[:6, 6]
            lam = max(lam * 0.1, 1e-12)
            if rel < 1e-10:
                it += 1
                break
        else:
            lam *= 10.0
            if lam > 1e10:
                break
        it += 1
    return R, t, cost, it
