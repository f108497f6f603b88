"""NumPy restatement of sfmloc_global_poses (include/sfmloc.h "Global poses"): every paragraph of that block, in the
order it stands there.  Every linear system can be solved two ways: solver="pcg", the header's own rule ("PCG": from 0,
the stated preconditioner and stopping), or solver="dense", numpy.linalg.solve on the assembled matrix.  What the two
leave between them is the parity bound of the device tests (profiles/globalposes_parity.json)."""
import math

import numpy as np

OPTIONS = dict(triplet_angle_deg=5.0, rotation_delta=0.0, translation_delta=0.05, function_tolerance=1e-6,
               pcg_tolerance=1e-6, max_steps=50, max_pcg=20000)


def adjacency(n_views, pairs):
    """sfmloc.h "adjacency" -> off [n + 1], nbr, pe (pair index, bit 31 set when the view is the pair's J)"""
    ent = [[] for _ in range(n_views)]
    for k, (a, b) in enumerate(np.asarray(pairs).reshape(-1, 2).tolist()):
        ent[a].append((b, k))
        ent[b].append((a, k | 0x80000000))
    off, nbr, pe = [0], [], []
    for v in range(n_views):
        for b, k in sorted(ent[v], key=lambda e: (e[0], e[1] & 0x7FFFFFFF)):
            nbr.append(b)
            pe.append(k)
        off.append(len(nbr))
    return np.array(off, np.uint32), np.array(nbr, np.uint32), np.array(pe, np.uint32)


def triplets(n_views, pairs, rel_R, angle_deg):
    """sfmloc.h "triplets" -> n_triplets [P], n_triplets_ok [P]"""
    pairs = np.asarray(pairs).reshape(-1, 2)
    edge = {(min(a, b), max(a, b)): k for k, (a, b) in enumerate(pairs.tolist())}
    nbrs = [set() for _ in range(n_views)]
    for a, b in edge:
        nbrs[a].add(b)
        nbrs[b].add(a)
    thr = 1.0 + 2.0 * math.cos(angle_deg * (math.pi / 180.0))

    def rot(x, y):
        k = edge[(min(x, y), max(x, y))]
        return rel_R[k] if pairs[k, 0] == x else rel_R[k].T

    nt, no = np.zeros(len(pairs), np.uint32), np.zeros(len(pairs), np.uint32)
    for (a, b), k in edge.items():
        for c in nbrs[a] & nbrs[b]:
            if c < b:
                continue    # every triangle once, from its pair (a, b) with a < b < c
            tr = np.trace(rot(c, a) @ (rot(b, c) @ rot(a, b)))
            for e in (k, edge[(b, c)], edge[(a, c)]):
                nt[e] += 1
                no[e] += tr > thr
    return nt, no


def component(n_views, pairs, on):
    """sfmloc.h "component" -> in_component [n] bool, root, size (size < 2: none, root 0)"""
    parent = list(range(n_views))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for (a, b), o in zip(np.asarray(pairs).reshape(-1, 2).tolist(), on):
        if o:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    label = np.array([find(v) for v in range(n_views)])
    count = np.bincount(label, minlength=n_views)
    root = int(np.argmax(count))          # (the first largest: the smallest label on a tie)
    if count[root] < 2:
        return np.zeros(n_views, bool), 0, 0
    return label == root, root, int(count[root])


def pcg(apply, minv, b, tol, max_it):
    """sfmloc.h "PCG" -> x, iterations, stop, |r| / |r0|"""
    x = np.zeros_like(b)
    r = b.copy()
    z = minv(r)
    p = z.copy()
    rz, rr0 = float(np.sum(r * z)), float(np.sum(r * r))
    rr, it = rr0, 0
    if not (rr0 > 0.0 and rz > 0.0):
        return x, 0, 0, 0.0
    while True:
        q = apply(p)
        pq = float(np.sum(p * q))
        if not pq > 0.0:
            stop = 2
            break
        alpha = rz / pq
        x += alpha * p
        r -= alpha * q
        z = minv(r)
        rzn, rr = float(np.sum(r * z)), float(np.sum(r * r))
        p = z + (rzn / rz) * p
        rz = rzn
        it += 1
        if not rr > tol * tol * rr0:
            stop = 0
            break
        if not rzn > 0.0:
            stop = 2
            break
        if it >= max_it:
            stop = 1
            break
    return x, it, stop, math.sqrt(rr / rr0)


def _block_system(n, I, J, B, diag, act):
    """the dense matrix of y_v = diag_v x_v - sum Off x_n over the active views: Off = B in J's row, B^T in I's"""
    idx = -np.ones(n, np.int64)
    idx[act] = np.arange(int(act.sum()))
    A = np.zeros((3 * int(act.sum()), 3 * int(act.sum())))
    for v in np.nonzero(act)[0]:
        A[3 * idx[v]:3 * idx[v] + 3, 3 * idx[v]:3 * idx[v] + 3] = diag[v]
    for i, j, b in zip(I, J, B):
        if act[i] and act[j]:
            A[3 * idx[j]:3 * idx[j] + 3, 3 * idx[i]:3 * idx[i] + 3] -= b
            A[3 * idx[i]:3 * idx[i] + 3, 3 * idx[j]:3 * idx[j] + 3] -= b.T
    return A


def _solve_blocks(n, I, J, B, diag, minv_blocks, rhs, act, o, solver):
    """rhs [n, 3, c]; diag, minv_blocks [n, 3, 3]; B [m, 3, 3] -> x [n, 3, c], iterations, stop, residual"""
    if solver == "dense":
        A = _block_system(n, I, J, B, diag, act)
        x = np.zeros_like(rhs)
        if act.any():
            x[act] = np.linalg.solve(A, rhs[act].reshape(-1, rhs.shape[2])).reshape(-1, 3, rhs.shape[2])
        return x, 0, 0, 0.0

    def apply(p):
        y = diag @ p
        np.subtract.at(y, J, B @ p[I])
        np.subtract.at(y, I, B.transpose(0, 2, 1) @ p[J])
        y[~act] = 0.0
        return y

    return pcg(apply, lambda r: minv_blocks @ r, rhs, o["pcg_tolerance"], o["max_pcg"])


def nearest_rotation(X):
    """sfmloc.h "chordal", the projection (the eigenvectors by eigh where the device runs its fixed-sweep Jacobi)"""
    l, V = np.linalg.eigh(X.T @ X)
    s = np.ones(3)
    if np.linalg.det(X) < 0.0:
        s[int(np.argmin(l))] = -1.0
    return X @ V @ np.diag(s / np.sqrt(l)) @ V.T


def huber(s, delta):
    s = np.asarray(s, float)
    small = s <= delta
    w = np.where(small, 1.0, delta / np.where(small, 1.0, s))
    return w, np.where(small, 0.5 * s * s, delta * (s - 0.5 * delta))


def gibbs(R, I, J, Rij):
    """sfmloc.h "IRLS": g [m, 3] and the mask of the pairs that have one (1 + tr E > 1e-12)"""
    E = R[J].transpose(0, 2, 1) @ (Rij @ R[I])
    den = 1.0 + np.trace(E, axis1=1, axis2=2)
    ok = den > 1e-12
    g = np.stack([E[:, 2, 1] - E[:, 1, 2], E[:, 0, 2] - E[:, 2, 0], E[:, 1, 0] - E[:, 0, 1]], 1)
    return np.where(ok[:, None], g / np.where(ok, den, 1.0)[:, None], 0.0), ok


def cayley(x):
    K = np.array([[0.0, -x[2], x[1]], [x[2], 0.0, -x[0]], [-x[1], x[0], 0.0]])
    return np.eye(3) + (2.0 / (1.0 + x @ x)) * (K + K @ K)


def _eye(n, s):
    return np.asarray(s, float).reshape(-1, 1, 1) * np.broadcast_to(np.eye(3), (n, 3, 3))


def global_poses(n_views, pairs, rel_R, rel_t, use_t=None, solver="pcg", **options):
    """-> dict: in_component, root, R [n, 3, 3], C [n, 3], the per-pair arrays of sfmloc_gposes_pair and the fields of
    sfmloc_gposes_report"""
    o = dict(OPTIONS, **options)
    n = int(n_views)
    pairs = np.asarray(pairs, np.int64).reshape(-1, 2)
    P = len(pairs)
    rel_R = np.asarray(rel_R, float).reshape(-1, 3, 3)
    rel_t = np.asarray(rel_t, float).reshape(-1, 3)
    use = np.ones(P, bool) if use_t is None else np.asarray(use_t).astype(bool)
    out = dict(n_views=n, n_pairs=P, in_component=np.zeros(n, bool), root=0, R=np.zeros((n, 3, 3)), C=np.zeros((n, 3)),
               n_triplets=np.zeros(P, np.uint32), n_triplets_ok=np.zeros(P, np.uint32), kept=np.zeros(P, bool),
               used_t=np.zeros(P, bool), rot_residual=np.zeros(P), trans_residual=np.zeros(P), n_component_views=0,
               n_rotation_pairs=0, n_translation_pairs=0, n_pairs_kept=0, n_triplets_total=0, n_triplets_ok_total=0)
    if P == 0:
        return out
    nt, no = triplets(n, pairs, rel_R, o["triplet_angle_deg"])
    kept = no > 0
    out.update(n_triplets=nt, n_triplets_ok=no, kept=kept, n_pairs_kept=int(kept.sum()),
               n_triplets_total=int(nt.sum()) // 3, n_triplets_ok_total=int(no.sum()) // 3)
    inc, root, size = component(n, pairs, kept & use)
    if size < 2:
        return out
    erot = kept & inc[pairs[:, 0]] & inc[pairs[:, 1]]
    etr = erot & use
    act = inc.copy()
    act[root] = False
    out.update(in_component=inc, root=root, n_component_views=size, used_t=etr, n_rotation_pairs=int(erot.sum()),
               n_translation_pairs=int(etr.sum()))

    # "chordal"
    I, J, Rij = pairs[erot, 0], pairs[erot, 1], rel_R[erot]
    deg = np.bincount(np.concatenate([I, J]), minlength=n).astype(float)
    b = np.zeros((n, 3, 3))
    np.add.at(b, J[I == root], Rij[I == root])
    np.add.at(b, I[J == root], Rij[J == root].transpose(0, 2, 1))
    b[~act] = 0.0
    safe = np.where(deg > 0, deg, 1.0)
    X, it, stop, res = _solve_blocks(n, I, J, Rij, _eye(n, deg), _eye(n, 1.0 / safe), b, act, o, solver)
    out.update(chordal_pcg=it, chordal_stop=stop, chordal_residual=res)
    R = np.zeros((n, 3, 3))
    R[root] = np.eye(3)
    for v in np.nonzero(act)[0]:
        R[v] = nearest_rotation(X[v])

    out["chordal_cost"] = float(np.sum((R[J] - Rij @ R[I]) ** 2))

    # "IRLS"
    delta = o["rotation_delta"] if o["rotation_delta"] > 0 else math.tan(o["triplet_angle_deg"] * (math.pi / 180.0) / 6.0)

    def rot_cost(Rs):
        g, ok = gibbs(Rs, I, J, Rij)
        s = np.sqrt(np.sum(g * g, 1))
        w, rho = huber(s, delta)
        return g, np.where(ok, w, 0.0), float(np.sum(np.where(ok, rho, 0.0))), s

    tried = accepted = pcg_total = 0
    stop = 1
    cost0 = None
    while tried < o["max_steps"]:
        g, w, cost, _ = rot_cost(R)
        cost0 = cost if cost0 is None else cost0
        rhs = np.zeros((n, 3, 1))
        np.add.at(rhs, J, (w[:, None] * g)[:, :, None])
        np.subtract.at(rhs, I, (w[:, None] * g)[:, :, None])
        rhs[~act] = 0.0
        dg = np.zeros(n)
        np.add.at(dg, I, w)
        np.add.at(dg, J, w)
        tried += 1
        if not cost > 0.0 or not np.any(rhs != 0.0):
            stop = 0
            break
        x, it, _, _ = _solve_blocks(n, I, J, _eye(len(I), w), _eye(n, dg), _eye(n, np.where(dg > 0, 1.0 / np.where(dg > 0, dg, 1.0), 0.0)),
                                    rhs, act, o, solver)
        pcg_total += it
        Rn = R.copy()
        for v in np.nonzero(act)[0]:
            Rn[v] = R[v] @ cayley(x[v, :, 0])
        cn = rot_cost(Rn)[2]
        if not (np.isfinite(cn) and cn < cost):
            stop = 2
            break
        accepted += 1
        R = Rn
        if cost - cn <= o["function_tolerance"] * cost:
            stop = 0
            break
    rot_final = rot_cost(R)
    res = np.zeros(P)
    res[erot] = rot_final[3]
    out.update(R=R, rot_residual=res, rot_steps_tried=tried, rot_steps_accepted=accepted, rot_pcg_total=pcg_total,
               rot_stop=stop, rot_cost_initial=cost0, rot_cost_final=rot_final[2])

    # "translation"
    I, J = pairs[etr, 0], pairs[etr, 1]
    d = -(R[J].transpose(0, 2, 1) @ rel_t[etr][:, :, None])[:, :, 0]
    d /= np.sqrt(np.sum(d * d, 1))[:, None]
    tdelta = o["translation_delta"]

    def tr_lin(Cs):
        dl = Cs[J] - Cs[I]
        s = np.sum(d * dl, 1)
        r = dl - np.maximum(s, 1.0)[:, None] * d
        nr = np.sqrt(np.sum(r * r, 1))
        w, rho = huber(nr, tdelta)
        W = w[:, None, None] * (np.eye(3) - np.where((s > 1.0)[:, None, None], d[:, :, None] * d[:, None, :], 0.0))
        return w[:, None] * r, W, float(np.sum(rho)), nr

    C = np.zeros((n, 3))
    lam, nu = 1e-4, 2.0
    tried = accepted = pcg_total = 0
    stop = 1
    cost0 = None
    while True:
        ev, W, cost, _ = tr_lin(C)
        cost0 = cost if cost0 is None else cost0
        A = np.zeros((n, 3, 3))
        np.add.at(A, I, W)
        np.add.at(A, J, W)
        rhs = np.zeros((n, 3, 1))
        np.subtract.at(rhs, J, ev[:, :, None])
        np.add.at(rhs, I, ev[:, :, None])
        rhs[~act] = 0.0
        Dg = A.copy()
        for a in range(3):
            Dg[:, a, a] += lam * np.clip(A[:, a, a], 1e-6, 1e32)
        Dg[~act] = np.eye(3)
        x, it, _, _ = _solve_blocks(n, I, J, W, Dg, np.linalg.inv(Dg), rhs, act, o, solver)
        x = x[:, :, 0]
        x[~act] = 0.0
        tried += 1
        pcg_total += it
        if not cost > 0.0 or not np.any(rhs != 0.0):
            stop = 0
            break
        u = x[J] - x[I]
        model = float(np.sum(-np.sum(ev * u, 1) - 0.5 * np.einsum("ea,eab,eb->e", u, W, u)))
        cn = tr_lin(C + x)[2]
        ok = np.isfinite(cn) and np.isfinite(model) and model > 0.0 and cn < cost and (cost - cn) / model > 1e-3
        running = True
        if ok:
            accepted += 1
            q = (cost - cn) / model
            lam = max(lam * max(1.0 / 3.0, 1.0 - (2.0 * q - 1.0) ** 3), 1e-32)
            nu = 2.0
            C = C + x
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
    out.update(C=C, trans_residual=res, trans_steps_tried=tried, trans_steps_accepted=accepted, trans_pcg_total=pcg_total,
               trans_stop=stop, trans_cost_initial=cost0, trans_cost_final=fin[2])
    return out


def align_similarity(A, B):
    """the similarity (s, Q, t) with s Q A + t ~ B in the least-squares sense (Umeyama) -> A mapped onto B"""
    ma, mb = A.mean(0), B.mean(0)
    U, S, Vt = np.linalg.svd((B - mb).T @ (A - ma))
    D = np.diag([1.0, 1.0, np.sign(np.linalg.det(U @ Vt))])
    Q = U @ D @ Vt
    s = np.trace(np.diag(S) @ D) / np.sum((A - ma) ** 2)
    return s * (A - ma) @ Q.T + mb


def rotation_error_deg(R, Rt):
    """the angle of R Rt^T per view, degrees: |R Rt^T - I|_F = 2 sqrt(2) sin(angle / 2), which unlike the arc cosine
    of the trace does not magnify a rounding at small angles"""
    D = R @ Rt.transpose(0, 2, 1) - np.eye(3)
    return np.degrees(2.0 * np.arcsin(np.clip(np.sqrt(np.sum(D * D, (1, 2)) / 8.0), 0.0, 1.0)))
