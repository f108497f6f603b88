"""NumPy restatement of sfmloc_tracks and sfmloc_sfm_triangulate (include/sfmloc.h "Structure from known poses",
csrc/tracks.hip, csrc/triangulate.hip): the components by hooking and pointer jumping, the filter and the order of the
tracks; the projection matrices, the rows, the 4 x 4 normal matrices, the fixed-sweep Jacobi, the sampled rounds, the
inlier test, the winner and the keep masks.  Only + - * / sqrt in f64, elementwise and in the stated order (NumPy does not
fuse), vectorised over hypotheses: X is the device's bits.  Arrays as adjust.sfm_arrays returns them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from adjust_np import ud_pixel_k3  # noqa: E402
from merge_np import jacobi_fixed, philox4x32_10  # noqa: E402

STAGE_TRIANGULATE = 5
ROBUST, BLIND = 0, 1
SEED = 0x5F3759DF12345678          # sfmloc_default_params' seed


# ---- tracks ----------------------------------------------------------------------------------------------------------

def edges(view_off, pairs, offsets, match_i, match_j, view_use=None):
    """one edge per match between global feature rows, pairs with a masked-out view left out (tracks_host.h)"""
    view_off = np.asarray(view_off, np.int64)
    a, b = [], []
    for k, (va, vb) in enumerate(np.asarray(pairs, np.int64).reshape(-1, 2)):
        if view_use is not None and not (view_use[va] and view_use[vb]):
            continue
        s = slice(int(offsets[k]), int(offsets[k + 1]))
        a.append(view_off[va] + np.asarray(match_i[s], np.int64))
        b.append(view_off[vb] + np.asarray(match_j[s], np.int64))
    cat = (lambda x: np.concatenate(x) if x else np.zeros(0, np.int64))
    return cat(a), cat(b)


def components(n, ea, eb):
    """sfmloc.h "components": label[x] = the smallest row of x's component, by passes of hooking (the larger root under
    the smaller, an integer minimum) and pointer jumping until a pass hooks nothing -> (label, passes)"""
    parent = np.arange(n, dtype=np.int64)
    passes = 0
    while True:
        passes += 1
        ra, rb = parent[ea], parent[eb]            # (after a jump every node points at its root)
        hook = ra != rb
        if not hook.any():
            return parent, passes
        np.minimum.at(parent, np.maximum(ra, rb)[hook], np.minimum(ra, rb)[hook])
        while True:
            nxt = parent[parent]
            if (nxt == parent).all():
                break
            parent = nxt


def tracks(view_off, pairs, offsets, match_i, match_j, view_use=None, min_length=2):
    """-> dict(counts [components, conflict, length, kept], off, view, feat, label of every kept track, passes)"""
    view_off = np.asarray(view_off, np.int64)
    n = int(view_off[-1])
    ea, eb = edges(view_off, pairs, offsets, match_i, match_j, view_use)
    label, passes = components(n, ea, eb)
    touched = np.zeros(n, bool)
    touched[ea] = True
    touched[eb] = True
    node = np.nonzero(touched)[0]                                  # ascending row
    order = np.argsort(label[node], kind="stable")                 # components ascend by label, rows inside ascend
    node, key = node[order], label[node][order]
    view = np.searchsorted(view_off, node, side="right") - 1       # the last v with view_off[v] <= row
    head = np.ones(len(node), bool)
    head[1:] = key[1:] != key[:-1]
    start = np.append(np.nonzero(head)[0], len(node))
    comp = np.cumsum(head) - 1
    n_comp = len(start) - 1
    conf = np.zeros(n_comp, bool)
    same = (~head[1:]) & (view[1:] == view[:-1])
    conf[comp[1:][same]] = True
    size = np.diff(start)
    short = ~conf & (size < max(1, min_length))
    kept = ~conf & ~short
    sel = kept[comp]
    off = np.concatenate([[0], np.cumsum(size[kept])]).astype(np.uint64)
    return {"counts": [n_comp, int(conf.sum()), int(short.sum()), int(kept.sum())], "off": off,
            "view": view[sel].astype(np.uint32), "feat": (node[sel] - view_off[view[sel]]).astype(np.uint32),
            "label": key[start[:-1]][kept], "passes": passes}


# ---- triangulation ---------------------------------------------------------------------------------------------------

def projections(a, pose_R, pose_C):
    """sfmloc.h "projection": P [n_views, 12] = K [R | t], t_i = -((R_i0 C0 + R_i1 C1) + R_i2 C2)"""
    pi = a["view_pose"].astype(np.int64)
    R = np.asarray(pose_R, np.float64).reshape(-1, 9)[pi]
    C = np.asarray(pose_C, np.float64).reshape(-1, 3)[pi]
    K = a["intrinsic"][a["view_intrinsic"].astype(np.int64)]
    f, ppx, ppy = K[:, 0], K[:, 1], K[:, 2]
    M = np.zeros((len(pi), 12))
    for i in range(3):
        M[:, 4 * i:4 * i + 3] = R[:, 3 * i:3 * i + 3]
        M[:, 4 * i + 3] = -((R[:, 3 * i] * C[:, 0] + R[:, 3 * i + 1] * C[:, 1]) + R[:, 3 * i + 2] * C[:, 2])
    P = np.zeros_like(M)
    for j in range(4):
        P[:, j] = f * M[:, j] + ppx * M[:, 8 + j]
        P[:, 4 + j] = f * M[:, 4 + j] + ppy * M[:, 8 + j]
        P[:, 8 + j] = M[:, 8 + j]
    return P


def undistorted(a):
    """sfmloc.h "ray": get_ud_pixel of every observation (its own pixel for a pinhole)"""
    ii = a["view_intrinsic"][a["obs_view"].astype(np.int64)].astype(np.int64)
    ud = a["obs_x"].astype(np.float64).copy()
    for o in np.nonzero(a["intrinsic_type"][ii] == 3)[0]:
        ud[o] = ud_pixel_k3(*[float(t) for t in a["intrinsic"][ii[o]]], float(a["obs_x"][o, 0]), float(a["obs_x"][o, 1]))
    return ud


def rows(a, P, ud):
    """the two rows x P2 - P0, y P2 - P1 of every observation -> (A [n_obs, 4], B [n_obs, 4])"""
    Po = P[a["obs_view"].astype(np.int64)]
    with np.errstate(invalid="ignore"):
        A = ud[:, 0:1] * Po[:, 8:12] - Po[:, 0:4]
        B = ud[:, 1:2] * Po[:, 8:12] - Po[:, 4:8]
    return A, B


def add_rows(G, A, B):
    """G [..., 4, 4] with one observation's rows added: G_ij = (G_ij + a_i a_j) + b_i b_j"""
    with np.errstate(invalid="ignore", over="ignore"):
        G = G + A[..., :, None] * A[..., None, :]
        return G + B[..., :, None] * B[..., None, :]


def solve(G):
    """G [H, 4, 4] -> (X [H, 3], ok [H]): the eigenvector of the smallest diagonal entry after the Jacobi sweeps (the first
    on ties), dehomogenised; not ok for a zero or non-finite w or a non-finite point"""
    G = np.asarray(G, np.float64)
    d, V = jacobi_fixed([[G[:, i, j] for j in range(4)] for i in range(4)])
    best = d[0]
    x = [V[k][0] for k in range(4)]
    for i in range(1, 4):
        take = d[i] < best
        best = np.where(take, d[i], best)
        x = [np.where(take, V[k][i], x[k]) for k in range(4)]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        X = np.stack([x[0] / x[3], x[1] / x[3], x[2] / x[3]], 1)
    ok = (x[3] != 0.0) & np.isfinite(x[3]) & np.isfinite(X).all(1)
    return X, ok


def sample2(n, seed, stream, rounds):
    """ac_sample<2> (geom_device.h) for every entry: n, stream and rounds are arrays -> int64 [len, 2], rows ascending"""
    rounds = np.asarray(rounds, np.uint64)
    z = np.zeros_like(rounds)
    d = philox4x32_10((rounds, np.asarray(stream, np.uint64), z, z + np.uint64(STAGE_TRIANGULATE)), seed & 0xFFFFFFFF,
                      seed >> 32)
    n = np.asarray(n, np.uint64)
    s0 = (d[0] % n).astype(np.int64)
    r = (d[1] % (n - np.uint64(1))).astype(np.int64)
    up = r >= s0
    r = r + up
    return np.stack([np.where(up, s0, r), np.where(up, r, s0)], 1)


def inliers(a, pose_R, pose_C, X, idx, thr, depth_only=False):
    """sfmloc.h "inliers" of the points X [H, 3] in the observations idx -> (mask [H, len(idx)], squared residuals)"""
    v = a["obs_view"][idx].astype(np.int64)
    pi, ii = a["view_pose"][v].astype(np.int64), a["view_intrinsic"][v].astype(np.int64)
    R = np.asarray(pose_R, np.float64).reshape(-1, 9)[pi]
    C = np.asarray(pose_C, np.float64).reshape(-1, 3)[pi]
    K = a["intrinsic"][ii]
    radial = a["intrinsic_type"][ii] == 3
    x, y = a["obs_x"][idx, 0], a["obs_x"][idx, 1]
    X = np.asarray(X, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        d0, d1, d2 = X[:, 0:1] - C[:, 0], X[:, 1:2] - C[:, 1], X[:, 2:3] - C[:, 2]
        X0 = (R[:, 0] * d0 + R[:, 1] * d1) + R[:, 2] * d2
        X1 = (R[:, 3] * d0 + R[:, 4] * d1) + R[:, 5] * d2
        X2 = (R[:, 6] * d0 + R[:, 7] * d1) + R[:, 8] * d2
        p0, p1 = X0 / X2, X1 / X2
        r2 = p0 * p0 + p1 * p1
        r4 = r2 * r2
        r6 = r4 * r2
        rc = ((1.0 + K[:, 3] * r2) + K[:, 4] * r4) + K[:, 5] * r6
        p0 = np.where(radial, p0 * rc, p0)
        p1 = np.where(radial, p1 * rc, p1)
        ex, ey = x - (K[:, 0] * p0 + K[:, 1]), y - (K[:, 0] * p1 + K[:, 2])
        sq = ex * ex + ey * ey
        ok = X2 > 0.0
        if not depth_only:
            ok = ok & (np.sqrt(sq) <= thr)
    return ok, sq


def normal_matrix(A, B, idx):
    """G over the observations idx in list order, from 0.0"""
    G = np.zeros((4, 4))
    for o in idx:
        G = add_rows(G, A[o], B[o])
    return G


def triangulate(a, pose_valid, pose_R, pose_C, mode=ROBUST, min_inliers=3, allow_pairs=True, residual_px=4.0, seed=SEED):
    """The whole call -> dict(X, obs_keep, landmark_keep, status [0 kept, 1 too few posed observations, 2 no valid
    hypothesis, 3 too few inliers], report, winner [round per landmark or -1], hyp [(landmark, G, X, ok) of every
    two-view round])"""
    off = a["obs_off"].astype(np.int64)
    n_lm = len(a["landmark_id"])
    P = projections(a, pose_R, pose_C)
    ud = undistorted(a)
    A, B = rows(a, P, ud)
    posed = np.asarray(pose_valid, bool)[a["view_pose"][a["obs_view"].astype(np.int64)].astype(np.int64)]
    lists = [np.arange(off[l], off[l + 1])[posed[off[l]:off[l + 1]]] for l in range(n_lm)]
    n = np.array([len(x) for x in lists], np.int64)
    status = np.zeros(n_lm, np.int64)
    status[n < 2] = 1
    X = np.zeros((n_lm, 3))
    winner = np.full(n_lm, -1, np.int64)
    have = np.zeros(n_lm, bool)
    rounds_run = 0
    hyp = {}
    if mode == BLIND:
        todo = np.nonzero(n >= 2)[0]
        if len(todo):
            Xb, ok = solve(np.stack([normal_matrix(A, B, lists[l]) for l in todo]))
            X[todo[ok]] = Xb[ok]
            have[todo[ok]] = True
            status[todo[~ok]] = 2
    else:
        # every two-view round of every landmark in one batch
        todo = np.nonzero(n >= 2)[0]
        n_rounds = np.where(n[todo] == 2, 1, 2 * n[todo])
        rounds_run = int(n_rounds.sum())
        hl = np.repeat(todo, n_rounds)
        hr = np.concatenate([np.arange(k) for k in n_rounds]) if len(todo) else np.zeros(0, np.int64)
        if len(hl):
            smp = sample2(n[hl], seed, a["landmark_id"][hl], hr)
            oa = np.array([lists[l][s] for l, s in zip(hl, smp[:, 0])])
            ob = np.array([lists[l][s] for l, s in zip(hl, smp[:, 1])])
            G = add_rows(add_rows(np.zeros((len(hl), 4, 4)), A[oa], B[oa]), A[ob], B[ob])
            XH, okH = solve(G)
            hyp = {"landmark": hl, "round": hr, "G": G, "X": XH, "ok": okH, "obs": np.stack([oa, ob], 1)}
        final = []
        for l in todo:
            h = np.nonzero(hl == l)[0]
            inl, sq = inliers(a, pose_R, pose_C, XH[h], lists[l], residual_px)
            cnt = inl.sum(1)
            ssq = np.zeros(len(h))
            for j in range(len(lists[l])):                      # the inliers' squares added in list order from 0.0
                ssq = np.where(inl[:, j], ssq + sq[:, j], ssq)
            cand = np.nonzero(okH[h])[0]
            if not len(cand):
                status[l] = 2
                continue
            cand = cand[cnt[cand] == cnt[cand].max()]           # sfmloc.h "winner"
            cand = cand[ssq[cand] == ssq[cand].min()]
            w = cand[0]
            winner[l] = w
            if cnt[w] < 2:
                status[l] = 3
                continue
            final.append((l, normal_matrix(A, B, lists[l][inl[w]])))
        if final:
            Xf, ok = solve(np.stack([g for _, g in final]))
            for (l, _), x, k in zip(final, Xf, ok):
                if k:
                    X[l] = x
                    have[l] = True
                else:
                    status[l] = 2
    obs_keep = np.zeros(int(off[-1]), bool)
    for l in np.nonzero(have)[0]:                               # sfmloc.h "keep rule"
        inl, _ = inliers(a, pose_R, pose_C, X[l], lists[l], residual_px, depth_only=mode == BLIND)
        need = 2 if (n[l] == 2 and allow_pairs) else min_inliers
        if inl[0].sum() >= need:
            obs_keep[lists[l][inl[0]]] = True
        else:
            status[l] = 3
            X[l] = 0.0
    report = {"landmarks_in": n_lm, "landmarks_kept": int((status == 0).sum()), "failed_posed": int((status == 1).sum()),
              "failed_hypothesis": int((status == 2).sum()), "failed_inliers": int((status == 3).sum()),
              "obs_in": int(off[-1]), "obs_kept": int(obs_keep.sum()), "rounds": rounds_run}
    return {"X": X, "obs_keep": obs_keep, "landmark_keep": status == 0, "status": status, "report": report,
            "winner": winner, "hyp": hyp}
