"""NumPy restatement of sfmloc_wedge_scales (include/sfmloc.h "Wedge scales", csrc/pairscales.hip): the bearings of the
inlier matches, their two-view depths, the per-side lists keyed by feature, the candidates of every view, the shared
features of a candidate, and the lower median of the depth quotients.  Only + - * / sqrt in f64, elementwise and in the
stated order (NumPy does not fuse): the records are the device's bits.

global_poses_scaled restates sfmloc_global_poses_scaled ("Scaled global poses"): the stages up to the rotations are
globalposes_np.global_poses itself; the scale graph, the scale averaging and the centres follow here.  As in
globalposes_np every linear system is solved two ways, solver="pcg" (the header's rule) or solver="dense"; what the two
leave between them is the parity bound of the device tests (tests/golden/pairscales_parity.json, written by tests/golden/make_pairscales_fixtures.py)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import globalposes_np as gp  # noqa: E402
from merge_np import jacobi_fixed  # noqa: E402
from relpose_np import bearings  # noqa: E402

OPTIONS = dict(min_shared=8, max_shared=2048)
SCALE_OPTIONS = dict(scale_delta=0.1, function_tolerance=1e-6, pcg_tolerance=1e-6, max_steps=50, max_pcg=20000)


def two_view_depths(R, t, b1, b2):
    """two_view_depths (csrc/twoview_device.h): the points of the matches with bearings b1, b2 [n, 2] from [I | 0] and
    [R | t] (R [9], t [3]) -> (z_I [n], z_J [n], exists [n]); relpose_np.front_count's arithmetic"""
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
    return X[:, 2], zj, ok


def side_list(feat, z):
    """sfmloc.h "lists": the yielded (feature, depth) of one pair side in the order of the inlier list -> (features
    ascending, each once; the depth of its first occurrence)"""
    feat = np.asarray(feat, np.int64)
    order = np.argsort(feat, kind="stable")
    f, zz = feat[order], np.asarray(z, np.float64)[order]
    first = np.ones(len(f), bool)
    first[1:] = f[1:] != f[:-1]
    return f[first], zz[first]


def wedge_ratio(fk, zk, fl, zl, max_shared=2048):
    """sfmloc.h "count" and "ratio" on the two lists of the shared view (features ascending, each once) -> (n_shared,
    ratio): all the shared features are counted; the first max_shared of them in feature order give q = z_k / z_l, and
    the ratio is element (n - 1) // 2 of q sorted by (value, feature).  n_shared = 0: ratio 0.0"""
    shared, ik, il = np.intersect1d(fk, fl, assume_unique=True, return_indices=True)      # ascending
    n_shared = len(shared)
    if n_shared == 0:
        return 0, 0.0
    ik, il, shared = ik[:max_shared], il[:max_shared], shared[:max_shared]
    with np.errstate(all="ignore"):
        q = np.asarray(zk, np.float64)[ik] / np.asarray(zl, np.float64)[il]
    order = sorted(range(len(q)), key=lambda i: (q[i], shared[i]))
    return n_shared, float(q[order[(len(q) - 1) // 2]])


def view_pairs(n_views, pairs, use_pair=None):
    """sfmloc.h "candidates": per view, (pair, side) of the used pairs that name it, ascending by pair index"""
    out = [[] for _ in range(n_views)]
    for k, (a, b) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        if use_pair is None or use_pair[k]:
            out[a].append((k, 0))
            out[b].append((k, 1))
    return out


def pair_lists(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j, rel_R, rel_t,
               inl_off, inl_idx, use_pair=None):
    """sfmloc.h "bearings", "depths", "lists" -> ({(pair, side): (features, depths)}, the number of inlier matches that
    yield depths)"""
    view_off = np.asarray(view_off, np.int64)
    kpt_xy = np.asarray(kpt_xy, np.float32).reshape(-1, 2)
    intrinsics = np.asarray(intrinsics, np.float64).reshape(-1, 6)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    rel_R, rel_t = np.asarray(rel_R, np.float64).reshape(-1, 9), np.asarray(rel_t, np.float64).reshape(-1, 3)
    cache = {}

    def view_bearings(v):
        if v not in cache:
            ii = int(view_intrinsic[v])
            cache[v] = bearings(kpt_xy[view_off[v]:view_off[v + 1]], intrinsics[ii], intrinsic_type[ii])
        return cache[v]
    lists, n_depths = {}, 0
    for k, (vi, vj) in enumerate(pairs):
        if use_pair is not None and not use_pair[k]:
            continue
        pos = int(offsets[k]) + np.asarray(inl_idx[int(inl_off[k]):int(inl_off[k + 1])], np.int64)
        fi, fj = np.asarray(match_i, np.int64)[pos], np.asarray(match_j, np.int64)[pos]
        zi, zj, ok = two_view_depths(rel_R[k], rel_t[k], view_bearings(int(vi))[fi], view_bearings(int(vj))[fj])
        with np.errstate(all="ignore"):
            ok = ok & np.isfinite(zj) & (zi > 0.0) & (zj > 0.0)
        n_depths += int(ok.sum())
        lists[(k, 0)] = side_list(fi[ok], zi[ok])
        lists[(k, 1)] = side_list(fj[ok], zj[ok])
    return lists, n_depths


def wedge_scales(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i, match_j, rel_R,
                 rel_t, inl_off, inl_idx, use_pair=None, min_shared=8, max_shared=2048):
    """The whole call -> dict(records = [(view, k, l, n_shared, ratio)] ordered by (k, l, view), n_candidates, n_depths,
    lists = pair_lists' lists)"""
    lists, n_depths = pair_lists(view_off, kpt_xy, view_intrinsic, intrinsics, intrinsic_type, pairs, offsets, match_i,
                                 match_j, rel_R, rel_t, inl_off, inl_idx, use_pair)
    records, n_candidates = [], 0
    for v, ent in enumerate(view_pairs(len(view_off) - 1, pairs, use_pair)):
        for a in range(len(ent)):
            for b in range(a + 1, len(ent)):
                n_candidates += 1
                (k, sk), (l, sl) = ent[a], ent[b]
                n_shared, ratio = wedge_ratio(*lists[(k, sk)], *lists[(l, sl)], max_shared)
                if n_shared >= min_shared:
                    records.append((v, k, l, n_shared, ratio))
    records.sort(key=lambda r: (r[1], r[2], r[0]))
    return dict(records=records, n_candidates=n_candidates, n_depths=n_depths, lists=lists)


def lower_median(v):
    v = np.sort(np.asarray(v, float))
    return float(v[(len(v) - 1) // 2])


def _solve_nodes(n, K, L, w, dg, rhs, act, o, solver):
    """dg_v x_v - sum w x_n = rhs_v over the active nodes -> x [n], iterations"""
    if solver == "dense":
        idx = -np.ones(n, np.int64)
        idx[act] = np.arange(int(act.sum()))
        A = np.diag(dg[act])
        for k, l, ww in zip(K, L, w):
            if act[k] and act[l]:
                A[idx[k], idx[l]] -= ww
                A[idx[l], idx[k]] -= ww
        x = np.zeros(n)
        if act.any():
            x[act] = np.linalg.solve(A, rhs[act])
        return x, 0

    def apply(p):
        y = dg * p
        np.subtract.at(y, L, w * p[K])
        np.subtract.at(y, K, w * p[L])
        y[~act] = 0.0
        return y

    x, it, _, _ = gp.pcg(apply, lambda r: np.where(dg > 0, r / np.where(dg > 0, dg, 1.0), 0.0), rhs, o["pcg_tolerance"],
                         o["max_pcg"])
    return x, it


def global_poses_scaled(n_views, pairs, rel_R, rel_t, wedge_kl, wedge_ratio, use_t=None, solver="pcg", scale=None,
                        **options):
    """-> the dict of globalposes_np.global_poses with the translation pairs, the view component, C and the trans_* fields
    of the scaled call, and baselines [P], wedge_weights [W], scale_* = the fields of sfmloc_gpscale_report"""
    o = dict(gp.OPTIONS, **options)
    so = dict(SCALE_OPTIONS, **(scale or {}))
    out = dict(gp.global_poses(n_views, pairs, rel_R, rel_t, use_t, solver=solver, **options))
    n = int(n_views)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    rel_t = np.asarray(rel_t, float).reshape(-1, 3)
    kl = np.asarray(wedge_kl, np.int64).reshape(-1, 2)
    ratio = np.asarray(wedge_ratio, float).reshape(-1)
    W = len(kl)
    etr0 = np.asarray(out["used_t"], bool)
    out.update(baselines=np.zeros(P), wedge_weights=np.zeros(W), scale_n_wedges=W, scale_n_wedges_used=0,
               scale_n_scaled_pairs=0, scale_n_scaled_views=0, scale_first_pair=0, scale_steps_tried=0,
               scale_steps_accepted=0, scale_pcg_total=0, scale_stop=0)
    if not out["n_component_views"]:
        return out

    # "scale graph"
    with np.errstate(invalid="ignore"):
        on = etr0[kl[:, 0]] & etr0[kl[:, 1]] & np.isfinite(ratio) & (ratio > 0.0) if W else np.zeros(0, bool)
    out["scale_n_wedges_used"] = int(on.sum())
    sinc, first, size = gp.component(P, kl, on) if on.any() else (np.zeros(P, bool), 0, 0)
    if size < 2:
        out.update(in_component=np.zeros(n, bool), root=0, n_component_views=0, n_translation_pairs=0,
                   used_t=np.zeros(P, bool), R=np.zeros((n, 3, 3)), C=np.zeros((n, 3)), trans_residual=np.zeros(P))
        return out
    etr = sinc
    inc = np.zeros(n, bool)
    inc[pairs[etr].reshape(-1)] = True
    root = int(np.nonzero(inc)[0][0])
    out.update(in_component=inc, root=root, n_component_views=int(inc.sum()), n_translation_pairs=size, used_t=etr,
               scale_n_scaled_pairs=size, scale_n_scaled_views=int(inc.sum()), scale_first_pair=first)

    # "scales"
    on = on & etr[kl[:, 0]]
    K, L, y = kl[on, 0], kl[on, 1], np.log(ratio[on])
    act = etr.copy()
    act[first] = False
    delta = so["scale_delta"]

    def sc_cost(xs):
        r = (xs[L] - xs[K]) - y
        w, rho = gp.huber(np.abs(r), delta)
        return r, w, float(np.sum(rho))

    x = np.zeros(P)
    tried = accepted = pcg_total = 0
    stop = 1
    cost0 = None
    while tried < so["max_steps"]:
        r, w, cost = sc_cost(x)
        cost0 = cost if cost0 is None else cost0
        rhs = np.zeros(P)
        np.subtract.at(rhs, L, w * r)
        np.add.at(rhs, K, w * r)
        rhs[~act] = 0.0
        dg = np.zeros(P)
        np.add.at(dg, K, w)
        np.add.at(dg, L, w)
        tried += 1
        if not cost > 0.0 or not np.any(rhs != 0.0):
            stop = 0
            break
        dx, it = _solve_nodes(P, K, L, w, dg, rhs, act, so, solver)
        pcg_total += it
        xn = x + np.where(act, dx, 0.0)
        cn = sc_cost(xn)[2]
        if not (np.isfinite(cn) and cn < cost):
            stop = 2
            break
        accepted += 1
        x = xn
        if cost - cn <= so["function_tolerance"] * cost:
            stop = 0
            break
    fin = sc_cost(x)
    ww = np.zeros(W)
    ww[on] = fin[1]
    b = np.where(etr, np.exp(x), 0.0)
    b = b / lower_median(b[etr])
    out.update(baselines=b, wedge_weights=ww, scale_steps_tried=tried, scale_steps_accepted=accepted,
               scale_pcg_total=pcg_total, scale_stop=stop, scale_cost_initial=cost0, scale_cost_final=fin[2])

    # "centres": globalposes_np's translation loop around r = D - b d, W = w I
    R = out["R"]
    I, J = pairs[etr, 0], pairs[etr, 1]
    d = -(R[J].transpose(0, 2, 1) @ rel_t[etr][:, :, None])[:, :, 0]
    d /= np.sqrt(np.sum(d * d, 1))[:, None]
    bd = b[etr][:, None] * d
    tdelta = o["translation_delta"]
    act = inc.copy()
    act[root] = False

    def tr_lin(Cs):
        r = (Cs[J] - Cs[I]) - bd
        nr = np.sqrt(np.sum(r * r, 1))
        w, rho = gp.huber(nr, tdelta)
        return w[:, None] * r, w[:, None, None] * np.broadcast_to(np.eye(3), (len(w), 3, 3)), float(np.sum(rho)), nr

    C = np.zeros((n, 3))
    lam, nu = 1e-4, 2.0
    tried = accepted = pcg_total = 0
    stop = 1
    cost0 = None
    while True:
        ev, Wb, cost, _ = tr_lin(C)
        cost0 = cost if cost0 is None else cost0
        A = np.zeros((n, 3, 3))
        np.add.at(A, I, Wb)
        np.add.at(A, J, Wb)
        rhs = np.zeros((n, 3, 1))
        np.subtract.at(rhs, J, ev[:, :, None])
        np.add.at(rhs, I, ev[:, :, None])
        rhs[~act] = 0.0
        Dg = A.copy()
        for a in range(3):
            Dg[:, a, a] += lam * np.clip(A[:, a, a], 1e-6, 1e32)
        Dg[~act] = np.eye(3)
        xx, it, _, _ = gp._solve_blocks(n, I, J, Wb, Dg, np.linalg.inv(Dg), rhs, act, o, solver)
        xx = xx[:, :, 0]
        xx[~act] = 0.0
        tried += 1
        pcg_total += it
        if not cost > 0.0 or not np.any(rhs != 0.0):
            stop = 0
            break
        u = xx[J] - xx[I]
        model = float(np.sum(-np.sum(ev * u, 1) - 0.5 * np.einsum("ea,eab,eb->e", u, Wb, u)))
        cn = tr_lin(C + xx)[2]
        ok = np.isfinite(cn) and np.isfinite(model) and model > 0.0 and cn < cost and (cost - cn) / model > 1e-3
        running = True
        if ok:
            accepted += 1
            q = (cost - cn) / model
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3), 1e-32)
            nu = 2.0
            C = C + xx
            if cost - cn <= o["function_tolerance"] * cost:
                stop, running = 0, False
        else:
            if np.isfinite(model) and 0.0 < model <= o["function_tolerance"] * cost:
                stop, running = 0, False
            lam *= nu
            nu *= 2.0
            if running and not lam < 1e32:
                stop, running = 2, False
        if running and tried >= o["max_steps"]:
            stop, running = 1, False
        if not running:
            break
    fin = tr_lin(C)
    res = np.zeros(P)
    res[etr] = fin[3]
    Rz = R.copy()
    Rz[~inc] = 0.0
    out.update(R=Rz, C=C, trans_residual=res, trans_steps_tried=tried, trans_steps_accepted=accepted,
               trans_pcg_total=pcg_total, trans_stop=stop, trans_cost_initial=cost0, trans_cost_final=fin[2])
    return out
