"""A second five-point solver and a second decomposition, independent of tests/relpose_np.py, for the CPU tests and the
fixture script: null space by SVD, the ten cubic constraints expanded by a generic polynomial product, elimination by
numpy.linalg.solve, the solutions as eigenvectors of the action matrix of multiplication by x on the quotient basis
(Stewenius, Engels, Nister 2006), numpy.linalg.eig; the decomposition by numpy.linalg.svd.  Nothing here is bit-exact
or meant to be."""
import itertools

import numpy as np

_CUBIC = [(3, 0, 0), (2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 1, 1), (1, 0, 2), (0, 3, 0), (0, 2, 1), (0, 1, 2), (0, 0, 3)]
_BASIS = [(2, 0, 0), (1, 1, 0), (1, 0, 1), (0, 2, 0), (0, 1, 1), (0, 0, 2), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0, 0, 0)]


def _pmul(a, b):
    out = {}
    for (ea, ca), (eb, cb) in itertools.product(a.items(), b.items()):
        e = (ea[0] + eb[0], ea[1] + eb[1], ea[2] + eb[2])
        out[e] = out.get(e, 0.0) + ca * cb
    return out


def _padd(a, b, s=1.0):
    out = dict(a)
    for e, c in b.items():
        out[e] = out.get(e, 0.0) + s * c
    return out


def five_point(x1, x2):
    """x1, x2 [5, 2] bearings (x2^T E x1 = 0) -> E [k, 9], real solutions of unit Frobenius norm"""
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    a, b, u, v = x1[:, 0], x1[:, 1], x2[:, 0], x2[:, 1]
    D = np.stack([u * a, u * b, u, v * a, v * b, v, a, b, np.ones(5)], 1)
    N = np.linalg.svd(D)[2][5:9]
    E = [[{(1, 0, 0): N[0, 3 * i + j], (0, 1, 0): N[1, 3 * i + j], (0, 0, 1): N[2, 3 * i + j], (0, 0, 0): N[3, 3 * i + j]}
          for j in range(3)] for i in range(3)]
    polys = []
    det = {}
    for (i, j, k), sgn in (((0, 1, 2), 1), ((1, 2, 0), 1), ((2, 0, 1), 1), ((0, 2, 1), -1), ((1, 0, 2), -1), ((2, 1, 0), -1)):
        det = _padd(det, _pmul(_pmul(E[0][i], E[1][j]), E[2][k]), sgn)
    polys.append(det)
    EEt = [[{} for _ in range(3)] for _ in range(3)]
    for i in range(3):
        for j in range(3):
            for k in range(3):
                EEt[i][j] = _padd(EEt[i][j], _pmul(E[i][k], E[j][k]))
    tr = _padd(_padd(EEt[0][0], EEt[1][1]), EEt[2][2])
    for i in range(3):
        for j in range(3):
            p = {}
            for k in range(3):
                p = _padd(p, _pmul(EEt[i][k], E[k][j]), 2.0)
            polys.append(_padd(p, _pmul(tr, E[i][j]), -1.0))
    M = np.array([[p.get(e, 0.0) for e in _CUBIC + _BASIS] for p in polys])
    try:
        C = np.linalg.solve(M[:, :10], M[:, 10:])
    except np.linalg.LinAlgError:
        return np.zeros((0, 9))
    A = np.zeros((10, 10))
    for i, e in enumerate(_BASIS):
        xe = (e[0] + 1, e[1], e[2])
        if xe in _CUBIC:
            A[i] = -C[_CUBIC.index(xe)]
        else:
            A[i, _BASIS.index(xe)] = 1.0
    w, V = np.linalg.eig(A)
    out = []
    for k in range(10):
        if abs(w[k].imag) > 1e-9 * max(1.0, abs(w[k].real)):
            continue
        vec = V[:, k]
        vec = (vec / vec[9]).real
        e = vec[6] * N[0] + vec[7] * N[1] + vec[8] * N[2] + N[3]
        e = e / np.linalg.norm(e)
        if np.isfinite(e).all():
            out.append(e)
    return np.array(out).reshape(-1, 9)


def align_distance(e, models):
    """the smallest max-norm distance between the unit-norm e [9] and +-m for m in models [k, 9] (inf for none)"""
    e = np.asarray(e, np.float64)
    e = e / np.linalg.norm(e)
    best = np.inf
    for m in np.asarray(models, np.float64).reshape(-1, 9):
        m = m / np.linalg.norm(m)
        best = min(best, np.abs(e - m).max(), np.abs(e + m).max())
    return best


def decompose(E):
    """E [9] -> the four (R [3, 3], t [3]) of the textbook SVD decomposition (Hartley & Zisserman 9.6.2), det R = +1"""
    U, _, Vt = np.linalg.svd(np.asarray(E, np.float64).reshape(3, 3))
    if np.linalg.det(U) < 0:
        U = -U
    if np.linalg.det(Vt) < 0:
        Vt = -Vt
    W = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    t = U[:, 2]
    return [(U @ W @ Vt, t), (U @ W @ Vt, -t), (U @ W.T @ Vt, t), (U @ W.T @ Vt, -t)]
