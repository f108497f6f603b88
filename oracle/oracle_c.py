"""ctypes loader for oracle/_build/liboracle.so (the C restatement, sfm_oracle.c).

TEST INFRASTRUCTURE ONLY -- never imported by sfmlocalization_amd/.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liboracle.so")
_lib = None


def build(force=False):
    srcs = [os.path.join(_HERE, f) for f in ("sfm_oracle.c", "sfm_oracle_geom.c", "sfm_oracle_bow.c", "sfm_oracle_akaze.c", "Makefile")]
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < max(os.path.getmtime(f) for f in srcs if os.path.exists(f)):
        subprocess.check_call(["make", "-C", _HERE], stdout=subprocess.DEVNULL)
    return _SO


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(_SO):
            build()
        _lib = C.CDLL(_SO)
        _lib.orc_version.restype = C.c_int
        _lib.orc_max_threads.restype = C.c_int
        _lib.orc_ratio_accept.restype = C.c_int
        _lib.orc_ratio_accept.argtypes = [C.c_int, C.c_int, C.c_float]
        _lib.orc_det_log10.restype = C.c_double
        _lib.orc_det_log10.argtypes = [C.c_double]
        _lib.orc_solve_cubic.restype = C.c_int
        _lib.orc_solve_cubic.argtypes = [C.c_double] * 4 + [C.POINTER(C.c_double)]
        _lib.orc_seven_point.restype = C.c_int
        _lib.orc_p3p_kneip.restype = C.c_int
        _lib.orc_fmatrix_filter.restype = C.c_int
        _lib.orc_p3p_localize.restype = C.c_int
        _lib.orc_match_set.restype = C.c_int
        _lib.orc_bow_dist.restype = C.c_float
        _lib.orc_refine_pose.restype = C.c_double
        _lib.orc_bof_cells.restype = C.c_int
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t)) if a is not None else None


def max_threads():
    return int(lib().orc_max_threads())


def hamming_2nn(query, bank, threads=1):
    """-> j0, d0, j1, d1 (int32 arrays over bank rows); sfm_oracle.c orc_hamming_2nn."""
    query = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, 64)
    bank = np.ascontiguousarray(bank, dtype=np.uint8).reshape(-1, 64)
    n = bank.shape[0]
    out = [np.empty(n, dtype=np.int32) for _ in range(4)]
    lib().orc_hamming_2nn(_p(query, C.c_uint8), C.c_uint32(query.shape[0]), _p(bank, C.c_uint8), C.c_uint64(n),
                          *[_p(o, C.c_int32) for o in out], C.c_int(threads))
    return tuple(out)


def ratio_accept(d0, d1, ratio):
    return bool(lib().orc_ratio_accept(int(d0), int(d1), C.c_float(ratio)))


def match_to_query(query, bank, view_off, view_sel=None, ratio=0.6, threads=1):
    """matchAKAZEToQuery restatement -> view_count[V], match_i, match_j, match_d (each [n_rows], lists at
    view_off[v])."""
    query = np.ascontiguousarray(query, dtype=np.uint8).reshape(-1, 64)
    bank = np.ascontiguousarray(bank, dtype=np.uint8).reshape(-1, 64)
    view_off = np.ascontiguousarray(view_off, dtype=np.uint32)
    nv = view_off.shape[0] - 1
    n = bank.shape[0]
    sel = None if view_sel is None else np.ascontiguousarray(view_sel, dtype=np.uint32)
    cnt = np.zeros(nv, dtype=np.uint32)
    mi = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    mj = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    md = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    lib().orc_match_to_query(_p(query, C.c_uint8), C.c_uint32(query.shape[0]), _p(bank, C.c_uint8),
                             _p(view_off, C.c_uint32), C.c_uint32(nv), _p(sel, C.c_uint32),
                             C.c_uint32(0 if sel is None else sel.shape[0]), C.c_float(ratio),
                             _p(cnt, C.c_uint32), _p(mi, C.c_uint32), _p(mj, C.c_uint32), _p(md, C.c_uint32),
                             C.c_int(threads))
    return cnt, mi, mj, md


# ---------------------------------------------------------------------------------------------------
# geometry (sfm_oracle_geom.c)
# ---------------------------------------------------------------------------------------------------
STAGE_FMATRIX, STAGE_P3P = 1, 2


def det_log10(x):
    return float(lib().orc_det_log10(C.c_double(x)))


def philox4x32_10(ctr, key):
    c = (C.c_uint32 * 4)(*ctr)
    lib().orc_philox4x32_10(c, C.c_uint32(key[0]), C.c_uint32(key[1]))
    return [int(v) for v in c]


def ac_sample(X, vec_index, seed, stage, stream, it):
    vi = np.ascontiguousarray(vec_index, dtype=np.int32)
    out = np.zeros(X, np.int32)
    lib().orc_ac_sample(C.c_int(X), _p(vi, C.c_int32), C.c_int(len(vi)), C.c_uint64(seed), C.c_uint32(stage),
                        C.c_uint32(stream), C.c_uint32(it), _p(out, C.c_int32))
    return out


def solve_cubic(a3, a2, a1, a0):
    r = (C.c_double * 3)()
    n = lib().orc_solve_cubic(a3, a2, a1, a0, r)
    return [r[i] for i in range(n)]


def solve_quartic_real(a):
    a = (C.c_double * 5)(*a)
    out = (C.c_double * 4)()
    lib().orc_solve_quartic_real(a, out)
    return [out[i] for i in range(4)]


def seven_point(x1, x2):
    x1 = np.ascontiguousarray(x1, np.float64).reshape(7, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(7, 2)
    F = np.zeros((3, 9), np.float64)
    n = lib().orc_seven_point(_p(x1, C.c_double), _p(x2, C.c_double), _p(F, C.c_double))
    return F[:n].reshape(n, 3, 3)


def p3p_kneip(x2d, X):
    x2d = np.ascontiguousarray(x2d, np.float64).reshape(3, 2)
    X = np.ascontiguousarray(X, np.float64).reshape(3, 3)
    M = np.zeros((4, 12), np.float64)
    n = lib().orc_p3p_kneip(_p(x2d, C.c_double), _p(X, C.c_double), _p(M, C.c_double))
    return M[:n].reshape(n, 3, 4)


def logcombi_tables(s, n):
    a = np.zeros(n + 1, np.float32)
    b = np.zeros(n + 1, np.float32)
    lib().orc_logcombi_tables(C.c_int(s), C.c_int(n), _p(a, C.c_float), _p(b, C.c_float))
    return a, b


def fmatrix_filter(x1, wh1, x2, wh2, precision, n_iter, seed, stream):
    """-> dict(n, inliers, F, nfa, errmax, iters); GeometricFilter_FMatrix_AC for one pair."""
    x1 = np.ascontiguousarray(x1, np.float64).reshape(-1, 2)
    x2 = np.ascontiguousarray(x2, np.float64).reshape(-1, 2)
    m = x1.shape[0]
    inl = np.full(max(m, 1), -1, np.int32)
    F = np.zeros(9, np.float64)
    nfa = C.c_double()
    em = C.c_double()
    it = C.c_int()
    n = lib().orc_fmatrix_filter(_p(x1, C.c_double), C.c_int(wh1[0]), C.c_int(wh1[1]), _p(x2, C.c_double),
                                 C.c_int(wh2[0]), C.c_int(wh2[1]), C.c_int(m), C.c_double(precision),
                                 C.c_int(n_iter), C.c_uint64(seed), C.c_uint32(stream), _p(inl, C.c_int32),
                                 _p(F, C.c_double), C.byref(nfa), C.byref(em), C.byref(it))
    return {"n": n, "inliers": inl[:n].copy(), "F": F.reshape(3, 3), "nfa": nfa.value, "errmax": em.value,
            "iters": it.value}


def guided_match(F_norm, errmax_norm, wh1, wh2, xy1, desc1, xy2, desc2, dist_ratio=0.6):
    """GeometricFilter_FMatrix_AC::Geometry_guided_matching for one pair (F / errmax as fmatrix_filter returns them,
    i.e. in the normalised frame); xy: .feat positions (float32).  -> (i[], j[]), one match per i, ascending."""
    F = np.ascontiguousarray(F_norm, np.float64).reshape(9)
    xy1 = np.ascontiguousarray(xy1, np.float32).reshape(-1, 2)
    xy2 = np.ascontiguousarray(xy2, np.float32).reshape(-1, 2)
    d1 = np.ascontiguousarray(desc1, np.uint8).reshape(-1, 64)
    d2 = np.ascontiguousarray(desc2, np.uint8).reshape(-1, 64)
    n1, n2 = xy1.shape[0], xy2.shape[0]
    oi = np.zeros(max(n1, 1), np.int32)
    oj = np.zeros(max(n1, 1), np.int32)
    L = lib()
    L.orc_guided_match.restype = C.c_int
    n = L.orc_guided_match(_p(F, C.c_double), C.c_double(errmax_norm), C.c_int(wh1[0]), C.c_int(wh1[1]),
                           C.c_int(wh2[0]), C.c_int(wh2[1]), _p(xy1, C.c_float), _p(d1, C.c_uint8), C.c_int(n1),
                           _p(xy2, C.c_float), _p(d2, C.c_uint8), C.c_int(n2), C.c_double(dist_ratio),
                           _p(oi, C.c_int32), _p(oj, C.c_int32))
    return oi[:n].astype(np.uint32), oj[:n].astype(np.uint32)


def unnormalize_f(F_norm, wh1, wh2):
    F = np.ascontiguousarray(F_norm, np.float64).reshape(9)
    out = np.zeros(9, np.float64)
    lib().orc_unnormalize_f(_p(F, C.c_double), C.c_int(wh1[0]), C.c_int(wh1[1]), C.c_int(wh2[0]), C.c_int(wh2[1]),
                            _p(out, C.c_double))
    return out.reshape(3, 3)


def p3p_localize(pt2d, pt3d, focal, ppx, ppy, max_iteration, seed, stream=0):
    pt2d = np.ascontiguousarray(pt2d, np.float64).reshape(-1, 2)
    pt3d = np.ascontiguousarray(pt3d, np.float64).reshape(-1, 3)
    n = pt2d.shape[0]
    inl = np.full(max(n, 1), -1, np.int32)
    P = np.zeros(12, np.float64)
    nfa = C.c_double()
    em = C.c_double()
    it = C.c_int()
    k = lib().orc_p3p_localize(_p(pt2d, C.c_double), _p(pt3d, C.c_double), C.c_int(n), C.c_double(focal),
                               C.c_double(ppx), C.c_double(ppy), C.c_int(max_iteration), C.c_uint64(seed),
                               C.c_uint32(stream), _p(inl, C.c_int32), _p(P, C.c_double), C.byref(em),
                               C.byref(nfa), C.byref(it))
    return {"n": k, "inliers": inl[:k].copy(), "P": P.reshape(3, 4), "nfa": nfa.value, "errmax": em.value,
            "iters": it.value}


def krt_from_p(P):
    P = np.ascontiguousarray(P, np.float64).reshape(12)
    K = np.zeros(9)
    R = np.zeros(9)
    t = np.zeros(3)
    lib().orc_krt_from_p(_p(P, C.c_double), _p(K, C.c_double), _p(R, C.c_double), _p(t, C.c_double))
    c = np.zeros(3)
    lib().orc_center_from_rt(_p(R, C.c_double), _p(t, C.c_double), _p(c, C.c_double))
    return K.reshape(3, 3), R.reshape(3, 3), t, c


def match_set(geo_view, geo_i, geo_j, view_off, put_count, put_i, put_j, put_d, row_landmark, nq):
    gv = np.ascontiguousarray(geo_view, np.uint32)
    gi = np.ascontiguousarray(geo_i, np.uint32)
    gj = np.ascontiguousarray(geo_j, np.uint32)
    vo = np.ascontiguousarray(view_off, np.uint32)
    pc = np.ascontiguousarray(put_count, np.uint32)
    pi = np.ascontiguousarray(put_i, np.uint32)
    pj = np.ascontiguousarray(put_j, np.uint32)
    pd = np.ascontiguousarray(put_d, np.uint32)
    rl = np.ascontiguousarray(row_landmark, np.int32)
    oq = np.zeros(max(nq, 1), np.uint32)
    ol = np.zeros(max(nq, 1), np.int32)
    n = lib().orc_match_set(_p(gv, C.c_uint32), _p(gi, C.c_uint32), _p(gj, C.c_uint32), C.c_int(len(gv)),
                            _p(vo, C.c_uint32), _p(pc, C.c_uint32), _p(pi, C.c_uint32), _p(pj, C.c_uint32),
                            _p(pd, C.c_uint32), _p(rl, C.c_int32), C.c_uint32(nq), _p(oq, C.c_uint32),
                            _p(ol, C.c_int32))
    return oq[:n].copy(), ol[:n].copy()


# ---------------------------------------------------------------------------------------------------
# bag of words (sfm_oracle_bow.c)
# ---------------------------------------------------------------------------------------------------
def bow_dist(a, b):
    a = np.ascontiguousarray(a, np.float32).ravel()
    b = np.ascontiguousarray(b, np.float32).ravel()
    return float(lib().orc_bow_dist(_p(a, C.c_float), _p(b, C.c_float), C.c_int(a.shape[0])))


def bow_select(bow, query, k, cand=None):
    bow = np.ascontiguousarray(bow, np.float32)
    query = np.ascontiguousarray(query, np.float32).ravel()
    cv = None if cand is None else np.ascontiguousarray(cand, np.uint32)
    n_cand = bow.shape[0] if cv is None else cv.shape[0]
    out = np.zeros(max(min(k, n_cand), 1), np.uint32)
    lib().orc_bow_select(_p(bow, C.c_float), C.c_int(bow.shape[1]), C.c_uint32(bow.shape[0]), _p(cv, C.c_uint32),
                         C.c_uint32(n_cand), _p(query, C.c_float), C.c_uint32(k), _p(out, C.c_uint32))
    return out[:min(k, n_cand)].copy()


def bof(desc, kxy, centers, resized=300, levels=2, norm_type=2, pca_mean=None, pca_eigvec=None, pca_eigval=None, n_pca=0):
    desc = np.ascontiguousarray(desc, np.float32)
    kxy = np.ascontiguousarray(kxy, np.float32).reshape(-1, 2)
    centers = np.ascontiguousarray(centers, np.float32)
    cells = int(lib().orc_bof_cells(C.c_int(levels)))
    out = np.zeros(centers.shape[0] * cells, np.float64)
    pm = pe = pv = None
    if n_pca:
        pm = np.ascontiguousarray(pca_mean, np.float32).ravel()
        pe = np.ascontiguousarray(np.asarray(pca_eigvec, np.float32)[:n_pca])
        pv = np.ascontiguousarray(np.asarray(pca_eigval, np.float32).ravel()[:n_pca])
    lib().orc_bof(_p(desc, C.c_float), _p(kxy, C.c_float), C.c_int(desc.shape[0]), C.c_int(desc.shape[1]),
                  _p(pm, C.c_float), _p(pe, C.c_float), _p(pv, C.c_float), C.c_int(n_pca), _p(centers, C.c_float),
                  C.c_int(centers.shape[0]), C.c_int(resized), C.c_int(levels), C.c_int(norm_type), _p(out, C.c_double))
    return out


def refine_pose(pt2d, pt3d, inliers, focal, ppx, ppy, R, t, max_iter=20):
    """A13 extension: LM refinement on the inliers; -> dict(R, t, center, cost0, cost, iters)."""
    pt2d = np.ascontiguousarray(pt2d, np.float64).reshape(-1, 2)
    pt3d = np.ascontiguousarray(pt3d, np.float64).reshape(-1, 3)
    inl = np.ascontiguousarray(inliers, np.int32)
    R = np.ascontiguousarray(R, np.float64).reshape(9).copy()
    t = np.ascontiguousarray(t, np.float64).reshape(3).copy()
    it = C.c_int()
    c0 = C.c_double()
    cost = lib().orc_refine_pose(_p(pt2d, C.c_double), _p(pt3d, C.c_double), _p(inl, C.c_int32), C.c_int(len(inl)),
                                 C.c_double(focal), C.c_double(ppx), C.c_double(ppy), _p(R, C.c_double),
                                 _p(t, C.c_double), C.c_int(max_iter), C.byref(it), C.byref(c0))
    c = np.zeros(3)
    lib().orc_center_from_rt(_p(R, C.c_double), _p(t, C.c_double), _p(c, C.c_double))
    return {"R": R.reshape(3, 3), "t": t, "center": c, "cost0": c0.value, "cost": float(cost), "iters": it.value}


# ---------------------------------------------------------------------------------------------------
# AKAZE (sfm_oracle_akaze.c)
# ---------------------------------------------------------------------------------------------------
def akaze_levels(w, h, omax=4, nsub=4):
    wh = np.zeros(64, np.int32)
    lib().orc_akaze_levels.restype = C.c_int
    n = lib().orc_akaze_levels(C.c_int(w), C.c_int(h), C.c_int(omax), C.c_int(nsub), _p(wh, C.c_int32))
    if n < 0:
        raise ValueError(_akaze_refusal(w, h, omax, nsub))
    return wh[:2 * n].reshape(n, 2)


def _akaze_refusal(w, h, omax, nsub):
    try:
        akaze_plan(w, h, omax, nsub)
    except ValueError as e:
        return str(e)
    return f"AKAZE plan {w}x{h} nOct {omax} nOctLay {nsub} refused"


def akaze_plan(w, h, omax=4, nsub=4):
    """orc_akaze_plan_read -> lev [n x 6] int32 (w, h, octave, sublevel, sigma_size, nsteps), tsteps [n x 64] float32;
    ValueError for a schedule with more than 64 FED steps at one level (the library refuses it too)."""
    lev = np.zeros((32, 6), np.int32)
    ts = np.zeros((32, 64), np.float32)
    bad = np.zeros(2, np.int32)
    lib().orc_akaze_plan_read.restype = C.c_int
    n = lib().orc_akaze_plan_read(C.c_int(w), C.c_int(h), C.c_int(omax), C.c_int(nsub), _p(lev, C.c_int32),
                                  _p(ts, C.c_float), _p(bad, C.c_int32))
    if n < 0:
        raise ValueError(f"AKAZE plan {w}x{h} nOct {omax} nOctLay {nsub}: {int(bad[1])} diffusion steps at level "
                         f"{int(bad[0])} (at most 64 per level)")
    return lev[:n].copy(), ts[:n].copy()


def akaze_detect_and_compute(gray, thres=0.001, omax=4, nsub=4, cap=20000, want_levels=False):
    """-> kpts [n x 6] (x, y, size, angle[rad], response, class_id), desc [n x 61] (+ Ldet, Lt of all levels)."""
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    kp = np.zeros((cap, 6), np.float32)
    desc = np.zeros((cap, 61), np.uint8)
    ldet = lt = None
    if want_levels:
        tot = int(sum(int(a) * int(b) for a, b in akaze_levels(w, h, omax, nsub)))
        ldet = np.zeros(tot, np.float32)
        lt = np.zeros(tot, np.float32)
    lib().orc_akaze_detect_and_compute.restype = C.c_int
    n = lib().orc_akaze_detect_and_compute(_p(gray, C.c_uint8), C.c_int(w), C.c_int(h), C.c_int(omax), C.c_int(nsub),
                                           C.c_float(thres), _p(kp, C.c_float), _p(desc, C.c_uint8), C.c_int(cap),
                                           _p(ldet, C.c_float), _p(lt, C.c_float))
    if n == -2 ** 31:
        raise ValueError(_akaze_refusal(w, h, omax, nsub))
    if n < 0:
        raise OverflowError(f"{-n} keypoints > cap {cap}")
    if want_levels:
        return kp[:n].copy(), desc[:n].copy(), ldet, lt
    return kp[:n].copy(), desc[:n].copy()


def akaze_compute(gray, kin, omax=4, nsub=4):
    """compute() on given keypoints [n x 4] (x, y, size, class_id) -> desc [n x 61], angle [n]."""
    gray = np.ascontiguousarray(gray, np.uint8)
    h, w = gray.shape
    kin = np.ascontiguousarray(kin, np.float32).reshape(-1, 4)
    desc = np.zeros((kin.shape[0], 61), np.uint8)
    ang = np.zeros(kin.shape[0], np.float32)
    lib().orc_akaze_compute.restype = C.c_int
    if lib().orc_akaze_compute(_p(gray, C.c_uint8), C.c_int(w), C.c_int(h), C.c_int(omax), C.c_int(nsub),
                               _p(kin, C.c_float), C.c_int(kin.shape[0]), _p(desc, C.c_uint8), _p(ang, C.c_float)) < 0:
        raise ValueError(_akaze_refusal(w, h, omax, nsub))
    return desc, ang


def akaze_math(x, y):
    out = np.zeros(3, np.float32)
    lib().orc_akaze_math(C.c_float(x), C.c_float(y), _p(out, C.c_float))
    return out


def dense_gray(bgr, size=300):
    """orc_dense_gray: resize(INTER_CUBIC) -> BGR2GRAY -> normalize(MINMAX) restatement (sfm_oracle_bow.c)."""
    bgr = np.ascontiguousarray(bgr, dtype=np.uint8)
    h, w, c = bgr.shape
    assert c == 3
    out = np.zeros((size, size), np.uint8)
    lib().orc_dense_gray(_p(bgr, C.c_uint8), C.c_int(w), C.c_int(h), C.c_int(size), _p(out, C.c_uint8))
    return out


def ud_pixel_k3(xy, f, ppx, ppy, k1, k2, k3):
    """orc_ud_pixel_k3: Pinhole_Intrinsic_Radial_K3::get_ud_pixel on [n, 2] pixels."""
    xy = np.ascontiguousarray(xy, np.float64).reshape(-1, 2)
    out = np.zeros_like(xy)
    lib().orc_ud_pixel_k3(C.c_double(f), C.c_double(ppx), C.c_double(ppy), C.c_double(k1), C.c_double(k2), C.c_double(k3),
                          _p(xy, C.c_double), C.c_int(xy.shape[0]), _p(out, C.c_double))
    return out
