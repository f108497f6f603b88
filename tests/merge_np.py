"""NumPy restatement of sfmloc_merge (include/sfmloc.h "sfmloc_merge", csrc/merge.hip): sampling, the 4-point and final
fits of both models, the ratio test, the inlier test, the winner rule, the nearest-other-point median and the transform.
Only + - * / sqrt in f64, elementwise and in the stated order (NumPy does not fuse), vectorised over rounds: the results
are the device's bits.  `Ops` below carries the same entry points as sfmlocalization_amd.capi's merge_* functions, so
sfmlocalization_amd.merge can be driven by either (merge.mergeModel(..., ops=merge_np.Ops(seed)))."""
import numpy as np

STAGE_MERGE = 3
SWEEPS = 10
SIMILARITY, AFFINE = 0, 1
U32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(c, k0, k1):
    """c: four uint64 arrays holding 32-bit counters -> four arrays after 10 rounds"""
    c0, c1, c2, c3 = [np.asarray(x, np.uint64) for x in c]
    k0, k1 = np.uint64(k0), np.uint64(k1)
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c0
        p1 = np.uint64(0xCD9E8D57) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ k0
        n1 = p1 & U32
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ k1
        n3 = p0 & U32
        c0, c1, c2, c3 = n0, n1, n2, n3
        k0 = (k0 + np.uint64(0x9E3779B9)) & U32
        k1 = (k1 + np.uint64(0xBB67AE85)) & U32
    return c0, c1, c2, c3


def sample4(n, seed, stream, rounds):
    """ac_sample<4> (geom_device.h) for every round in `rounds` -> int64 [len(rounds), 4], each row ascending"""
    rounds = np.asarray(rounds, np.uint64)
    z = np.zeros_like(rounds)
    draws = philox4x32_10((rounds, z + np.uint64(stream), z, z + np.uint64(STAGE_MERGE)), seed & 0xFFFFFFFF, seed >> 32)
    s = np.zeros((len(rounds), 4), np.int64)
    for i in range(4):
        r = (draws[i] % np.uint64(n - i)).astype(np.int64)
        j = np.zeros(len(rounds), np.int64)
        for k in range(i):                      # for (j = 0; j < i && r >= s[j]; ++j) ++r;  (s[:i] is ascending)
            go = (j == k) & (r >= s[:, k])
            r = r + go
            j = j + go
        for k in range(i, 0, -1):               # shift up the entries above the insertion point
            s[:, k] = np.where(k > j, s[:, k - 1], s[:, k])
        for k in range(i + 1):
            s[:, k] = np.where(j == k, r, s[:, k])
    return s


def jacobi_fixed(A):
    """A: N x N nested list of arrays (symmetric) -> (diagonal list, V nested list); `jacobi` of sfmloc.h"""
    N = len(A)
    A = [[np.array(A[i][j], np.float64) for j in range(N)] for i in range(N)]
    one = np.ones_like(A[0][0])
    V = [[one * (1.0 if i == j else 0.0) for j in range(N)] for i in range(N)]
    with np.errstate(all="ignore"):
        for _ in range(SWEEPS):
            for p in range(N - 1):
                for q in range(p + 1, N):
                    apq = A[p][q]
                    skip = apq == 0.0
                    theta = (A[q][q] - A[p][p]) / (2.0 * apq)
                    at = np.where(theta < 0.0, -theta, theta)
                    t = np.where(theta < 0.0, -1.0, 1.0) / (at + np.sqrt(theta * theta + 1.0))
                    c = 1.0 / np.sqrt(t * t + 1.0)
                    s = t * c
                    for k in range(N):
                        akp, akq = A[k][p], A[k][q]
                        A[k][p] = np.where(skip, akp, c * akp - s * akq)
                        A[k][q] = np.where(skip, akq, s * akp + c * akq)
                    for k in range(N):
                        apk, aqk = A[p][k], A[q][k]
                        A[p][k] = np.where(skip, apk, c * apk - s * aqk)
                        A[q][k] = np.where(skip, aqk, s * apk + c * aqk)
                    A[p][q] = np.where(skip, A[p][q], 0.0)
                    A[q][p] = np.where(skip, A[q][p], 0.0)
                    for k in range(N):
                        vkp, vkq = V[k][p], V[k][q]
                        V[k][p] = np.where(skip, vkp, c * vkp - s * vkq)
                        V[k][q] = np.where(skip, vkq, s * vkp + c * vkq)
    return [A[i][i] for i in range(N)], V


def _finite12(M):
    f = np.isfinite(M[0])
    for m in M[1:]:
        f = f & np.isfinite(m)
    return f


def solve_similarity(ma, mb, S, saa, sbb):
    """-> (M as a list of 12 arrays, ok)"""
    N = [[None] * 4 for _ in range(4)]
    N[0][0] = (S[0][0] + S[1][1]) + S[2][2]
    N[0][1] = S[1][2] - S[2][1]
    N[0][2] = S[2][0] - S[0][2]
    N[0][3] = S[0][1] - S[1][0]
    N[1][1] = (S[0][0] - S[1][1]) - S[2][2]
    N[1][2] = S[0][1] + S[1][0]
    N[1][3] = S[2][0] + S[0][2]
    N[2][2] = (S[1][1] - S[0][0]) - S[2][2]
    N[2][3] = S[1][2] + S[2][1]
    N[3][3] = (S[2][2] - S[0][0]) - S[1][1]
    for i in range(1, 4):
        for j in range(i):
            N[i][j] = N[j][i]
    d, V = jacobi_fixed(N)
    with np.errstate(all="ignore"):
        best, q = d[0], [V[k][0] for k in range(4)]
        for i in range(1, 4):
            take = d[i] > best
            best = np.where(take, d[i], best)
            q = [np.where(take, V[k][i], q[k]) for k in range(4)]
        nq = np.sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3])
        w, x, y, z = q[0] / nq, q[1] / nq, q[2] / nq, q[3] / nq
        R = [[1.0 - 2.0 * (y * y + z * z), 2.0 * (x * y - w * z), 2.0 * (x * z + w * y)],
             [2.0 * (x * y + w * z), 1.0 - 2.0 * (x * x + z * z), 2.0 * (y * z - w * x)],
             [2.0 * (x * z - w * y), 2.0 * (y * z + w * x), 1.0 - 2.0 * (x * x + y * y)]]
        sc = np.sqrt(saa / sbb)
        M = []
        for i in range(3):
            m0, m1, m2 = sc * R[i][0], sc * R[i][1], sc * R[i][2]
            M += [m0, m1, m2, ma[i] - ((m0 * mb[0] + m1 * mb[1]) + m2 * mb[2])]
    return M, _finite12(M)


def gauss4(G, H):
    """G X = H by the elimination of sfmloc.h -> (X 4 x 3 nested list, ok)"""
    G = [[np.array(G[i][j], np.float64) for j in range(4)] for i in range(4)]
    H = [[np.array(H[i][c], np.float64) for c in range(3)] for i in range(4)]
    ok = np.ones(np.shape(G[0][0]), bool)
    X = [[None] * 3 for _ in range(4)]
    with np.errstate(all="ignore"):
        for k in range(4):
            for r in range(k + 1, 4):
                sw = np.abs(G[r][k]) > np.abs(G[k][k])
                for j in range(4):
                    a, b = G[k][j], G[r][j]
                    G[k][j], G[r][j] = np.where(sw, b, a), np.where(sw, a, b)
                for c in range(3):
                    a, b = H[k][c], H[r][c]
                    H[k][c], H[r][c] = np.where(sw, b, a), np.where(sw, a, b)
            piv = G[k][k]
            ok = ok & (piv != 0.0)
            for r in range(k + 1, 4):
                f = G[r][k] / piv
                for j in range(k + 1, 4):
                    G[r][j] = G[r][j] - f * G[k][j]
                for c in range(3):
                    H[r][c] = H[r][c] - f * H[k][c]
        for k in range(3, -1, -1):
            for c in range(3):
                acc = H[k][c]
                for j in range(k + 1, 4):
                    acc = acc - G[k][j] * X[j][c]
                X[k][c] = acc / G[k][k]
    return X, ok


def _affine_M(X):
    return [X[j][i] for i in range(3) for j in range(4)]


def ratio_ok(M, svd_ratio):
    Cm = [[None] * 3 for _ in range(3)]
    with np.errstate(all="ignore"):
        for i in range(3):
            for j in range(i, 3):
                Cm[i][j] = (M[i] * M[j] + M[4 + i] * M[4 + j]) + M[8 + i] * M[8 + j]
                Cm[j][i] = Cm[i][j]
        d, _ = jacobi_fixed(Cm)
        emax, emin = d[0], d[0]
        for i in (1, 2):
            emax = np.where(d[i] > emax, d[i], emax)
            emin = np.where(d[i] < emin, d[i], emin)
        return np.sqrt(emax) / np.sqrt(emin) < svd_ratio


def round_models(A, B, seed, stream, rounds, model, svd_ratio):
    """the 4-point model of every round -> (M [len(rounds), 12], ok [len(rounds)], samples)"""
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    s = sample4(len(A), seed, stream, rounds)
    a = [[A[s[:, p], c] for c in range(3)] for p in range(4)]
    b = [[B[s[:, p], c] for c in range(3)] for p in range(4)]
    fin = np.ones(len(s), bool)
    for p in range(4):
        for c in range(3):
            fin &= np.isfinite(a[p][c]) & np.isfinite(b[p][c])
    with np.errstate(all="ignore"):
        if model == AFFINE:
            G = [[b[p][0], b[p][1], b[p][2], np.ones(len(s))] for p in range(4)]
            X, ok = gauss4(G, a)
            M = _affine_M(X)
            ok = ok & _finite12(M) & ratio_ok(M, svd_ratio)
        else:
            ma = [(((a[0][c] + a[1][c]) + a[2][c]) + a[3][c]) / 4.0 for c in range(3)]
            mb = [(((b[0][c] + b[1][c]) + b[2][c]) + b[3][c]) / 4.0 for c in range(3)]
            a = [[a[p][c] - ma[c] for c in range(3)] for p in range(4)]
            b = [[b[p][c] - mb[c] for c in range(3)] for p in range(4)]
            S = [[((b[0][i] * a[0][j] + b[1][i] * a[1][j]) + b[2][i] * a[2][j]) + b[3][i] * a[3][j] for j in range(3)]
                 for i in range(3)]
            saa, sbb = 0.0, 0.0
            for p in range(4):
                saa = saa + ((a[p][0] * a[p][0] + a[p][1] * a[p][1]) + a[p][2] * a[p][2])
                sbb = sbb + ((b[p][0] * b[p][0] + b[p][1] * b[p][1]) + b[p][2] * b[p][2])
            M, ok = solve_similarity(ma, mb, S, saa, sbb)
    return np.stack(M, 1), ok & fin, s


def inlier_mask(A, B, M, thres):
    """M [12] or [k, 12] -> bool [n] or [k, n]"""
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    M = np.asarray(M, np.float64)
    m = [M[..., i, None] for i in range(12)] if M.ndim == 2 else [M[i] for i in range(12)]
    x0, x1, x2 = B[:, 0], B[:, 1], B[:, 2]
    with np.errstate(all="ignore"):
        dx = (((m[0] * x0 + m[1] * x1) + m[2] * x2) + m[3]) - A[:, 0]
        dy = (((m[4] * x0 + m[5] * x1) + m[6] * x2) + m[7]) - A[:, 1]
        dz = (((m[8] * x0 + m[9] * x1) + m[10] * x2) + m[11]) - A[:, 2]
        return np.sqrt((dx * dx + dy * dy) + dz * dz) < thres


def block_sum(v):
    """sum of v in the order of sfmloc.h "final fit": 256 strided partials, then the pairwise tree"""
    v = np.asarray(v, np.float64)
    pad = (-len(v)) % 256
    rows = np.concatenate([v, np.zeros(pad)]).reshape(-1, 256)
    part = np.zeros(256)
    for r in rows:
        part = part + r          # (+ 0.0 on the padding leaves a partial's bits: it is never -0.0)
    s = 128
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s >>= 1
    return part[0]


def final_fit(A, B, idx, model):
    """-> M [3, 4] or None"""
    A, B = np.asarray(A, np.float64).reshape(-1, 3)[idx], np.asarray(B, np.float64).reshape(-1, 3)[idx]
    m = float(len(idx))
    a, b = [A[:, c] for c in range(3)], [B[:, c] for c in range(3)]
    with np.errstate(all="ignore"):
        if model == AFFINE:
            v = b + [None]
            G = [[None] * 4 for _ in range(4)]
            for j in range(4):
                for k in range(j, 4):
                    if k == 3:
                        G[j][k] = np.float64(m) if j == 3 else block_sum(v[j])
                    else:
                        G[j][k] = block_sum(v[j] * v[k])
                    G[k][j] = G[j][k]
            H = [[block_sum(b[j] * a[c]) for c in range(3)] for j in range(3)] + [[block_sum(a[c]) for c in range(3)]]
            X, ok = gauss4(G, H)
            M = _affine_M(X)
            ok = ok & _finite12(M)
        else:
            ma = [block_sum(a[c]) / m for c in range(3)]
            mb = [block_sum(b[c]) / m for c in range(3)]
            a0 = [a[c] - ma[c] for c in range(3)]
            b0 = [b[c] - mb[c] for c in range(3)]
            S = [[block_sum(b0[i] * a0[j]) for j in range(3)] for i in range(3)]
            saa = block_sum((a0[0] * a0[0] + a0[1] * a0[1]) + a0[2] * a0[2])
            sbb = block_sum((b0[0] * b0[0] + b0[1] * b0[1]) + b0[2] * b0[2])
            M, ok = solve_similarity(ma, mb, S, saa, sbb)
    return np.array([float(x) for x in M]).reshape(3, 4) if bool(ok) else None


def ransac(A, B, thres, rounds, svd_ratio, model, seed, stream=0, chunk=512, want_counts=False):
    """sfmloc_merge_ransac -> dict(M, round, count, inliers[, counts: every round's count, 0 where its key is 0])"""
    A, B = np.asarray(A, np.float64).reshape(-1, 3), np.asarray(B, np.float64).reshape(-1, 3)
    n = len(A)
    out = {"M": None, "round": 0, "count": 0, "inliers": np.zeros(0, np.uint32)}
    if n < 4 or rounds == 0:
        return out
    best_count, best_round, best_M = 0, 0, None
    counts = np.zeros(rounds, np.int64)
    for r0 in range(0, rounds, chunk):
        rr = np.arange(r0, min(rounds, r0 + chunk))
        M, ok, _ = round_models(A, B, seed, stream, rr, model, svd_ratio)
        cnt = inlier_mask(A, B, M, thres).sum(1) * ok
        counts[rr] = cnt
        k = int(np.argmax(cnt))                  # (the first maximum: the lowest round)
        if cnt[k] > best_count:
            best_count, best_round, best_M = int(cnt[k]), int(rr[k]), M[k]
    if want_counts:
        out["counts"] = counts
    if best_count == 0:
        return out
    inl = np.nonzero(inlier_mask(A, B, best_M, thres))[0].astype(np.uint32)
    out.update(round=best_round, count=best_count, inliers=inl, M_round=best_M.reshape(3, 4))
    if best_count >= 4:
        out["M"] = final_fit(A, B, inl, model)
    return out


def nn_distances(X, block=512):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    n = len(X)
    out = np.empty(n)
    for i0 in range(0, n, block):
        P = X[i0:i0 + block]
        dx = P[:, None, 0] - X[None, :, 0]
        dy = P[:, None, 1] - X[None, :, 1]
        dz = P[:, None, 2] - X[None, :, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        d2[np.arange(len(P)), i0 + np.arange(len(P))] = np.inf
        out[i0:i0 + block] = np.sqrt(d2.min(1))
    return out


def median_nn(X):
    X = np.asarray(X, np.float64).reshape(-1, 3)
    n = len(X)
    if n < 2:
        return 0.0
    if not np.isfinite(X).all():
        raise ValueError("a coordinate is not finite")
    d = np.sort(nn_distances(X))
    return float(d[n // 2]) if n % 2 else float((d[n // 2 - 1] + d[n // 2]) / 2.0)


def transform(M, R=None, X=None):
    M = np.asarray(M, np.float64).reshape(3, 4)
    R = np.array(np.zeros((0, 3, 3)) if R is None else R, np.float64).reshape(-1, 3, 3)
    X = np.array(np.zeros((0, 3)) if X is None else X, np.float64).reshape(-1, 3)
    Ro = np.empty_like(R)
    Xo = np.empty_like(X)
    for i in range(3):
        for j in range(3):
            Ro[:, i, j] = (M[i, 0] * R[:, 0, j] + M[i, 1] * R[:, 1, j]) + M[i, 2] * R[:, 2, j]
        Xo[:, i] = ((M[i, 0] * X[:, 0] + M[i, 1] * X[:, 1]) + M[i, 2] * X[:, 2]) + M[i, 3]
    return Ro, Xo


class Ops:
    """The device entry points of sfmlocalization_amd.merge on the host (same names and results as capi.merge_*)."""

    def __init__(self, seed):
        self.seed = seed

    def merge_ransac(self, A, B, thres, rounds, svd_ratio, model, stream=0):
        return ransac(A, B, thres, rounds, svd_ratio, model, self.seed, stream)

    def merge_inliers(self, A, B, M, thres):
        return np.nonzero(inlier_mask(A, B, np.asarray(M, np.float64).reshape(12), thres))[0].astype(np.uint32)

    def merge_median_nn(self, X):
        return median_nn(X)

    def merge_transform(self, M, R=None, X=None):
        return transform(M, R, X)
