"""Planted scenes for sfmloc_wedge_scales: cameras and points with known positions, every view's features (the points it
sees, in a shuffled order, projected with pixel noise), every pair's matches (the points both views see, shuffled), the
pair's relative pose from the planted poses with globalposes_scene's noise, and its inlier list (a shuffle of the match
positions).  A scene is a dict with the arguments of capi.WedgeScales / pairscales_np.wedge_scales under "call", the
planted R_true, C_true, the planted baselines b_true [P], and the indices of what was planted."""
import numpy as np

import globalposes_scene as gs

K_PINHOLE = (800.0, 640.0, 480.0, 0.0, 0.0, 0.0)
K_RADIAL = (750.0, 630.0, 470.0, -0.05, 0.01, 0.001)


def look_at(C, target, up=(0.0, 0.0, 1.0)):
    z = (target - C) / np.linalg.norm(target - C)
    x = np.cross(np.array(up), z)
    x /= np.linalg.norm(x)
    return np.stack([x, np.cross(z, x), z])


def assemble(R, C, X, sees, pair_list, rng, px_noise=0.3, rot_noise=np.radians(0.2), dir_noise=0.005, view_intrinsic=None,
             drop=0.0):
    """sees[v]: the points view v has features of.  -> the scene; which[v] maps a point to its feature in v"""
    n = len(R)
    view_intrinsic = np.zeros(n, np.uint32) if view_intrinsic is None else np.asarray(view_intrinsic, np.uint32)
    intr = np.array([K_PINHOLE, K_RADIAL])
    feats, which = [], []
    for v in range(n):
        ids = rng.permutation(np.asarray(sees[v], np.int64))
        Xc = (X[ids] - C[v]) @ R[v].T
        f, ppx, ppy = intr[view_intrinsic[v], :3]
        px = f * Xc[:, :2] / Xc[:, 2:] + np.array([ppx, ppy]) + rng.normal(size=(len(ids), 2)) * px_noise
        feats.append(px.astype(np.float32))
        which.append({int(p): i for i, p in enumerate(ids)})
    mi, mj, offsets, inl, inl_off = [], [], [0], [], [0]
    for a, b in pair_list:
        both = rng.permutation(np.array(sorted(set(which[a]) & set(which[b])), np.int64))
        mi += [which[a][int(p)] for p in both]
        mj += [which[b][int(p)] for p in both]
        offsets.append(len(mi))
        keep = rng.permutation(len(both))
        keep = keep[:len(keep) - int(drop * len(keep))]
        inl += keep.tolist()
        inl_off.append(len(inl))
    s = gs.build(R, C, pair_list, rng, rot_noise, dir_noise)
    s["b_true"] = np.array([np.linalg.norm(C[b] - C[a]) for a, b in pair_list])
    s["which"] = which
    s["call"] = dict(view_off=np.concatenate([[0], np.cumsum([len(f) for f in feats])]).astype(np.uint64),
                     kpt_xy=np.concatenate(feats).astype(np.float32).reshape(-1, 2), view_intrinsic=view_intrinsic,
                     intrinsics=intr, intrinsic_type=np.array([0, 3], np.uint32), pairs=s["pairs"],
                     offsets=np.array(offsets, np.uint64), match_i=np.array(mi, np.uint32), match_j=np.array(mj, np.uint32),
                     rel_R=s["rel_R"], rel_t=s["rel_t"], inl_off=np.array(inl_off, np.uint64),
                     inl_idx=np.array(inl, np.uint32))
    return s


def scene_triplet(seed=11):
    """(a) three views around 40 points all of them see, the second through the radial intrinsic: three pairs, three
    wedges"""
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1.0, 1.0, (40, 3))
    C = np.array([[6.0, 0.0, 0.5], [4.0, 4.5, -0.3], [0.5, 6.5, 0.2]])
    R = np.stack([look_at(c, rng.uniform(-0.2, 0.2, 3)) for c in C])
    return assemble(R, C, X, [range(40)] * 3, [(0, 1), (1, 2), (2, 0)], rng, view_intrinsic=[0, 1, 0])


def scene_corridor(seed=12, n=14, reach=3, n_points=400, wrong=True, rot_noise=np.radians(0.2), dir_noise=0.005):
    """(b) 14 views walking down a corridor, steps of 0.6 to 1.6 units and one of 3, each paired with its next 3; 400
    points on the two walls; a view sees the points 1 to 15 units ahead within 50 degrees of its axis.  wrong: the
    direction of pair `wrong_pair` is replaced by a random one."""
    rng = np.random.default_rng(seed)
    steps = rng.uniform(0.6, 1.6, n - 1)
    steps[n // 2] = 3.0
    xs = np.concatenate([[0.0], np.cumsum(steps)])
    C = np.stack([xs, rng.uniform(-0.05, 0.05, n), rng.uniform(-0.05, 0.05, n)], 1)     # (a walked line, not a ruled one)
    R = np.stack([gs.random_rotation(rng, 0.1) @ look_at(c, c + np.array([1.0, 0.0, 0.0])) for c in C])
    X = np.stack([rng.uniform(-2.0, xs[-1] + 16.0, n_points), np.where(rng.uniform(size=n_points) < 0.5, -2.0, 2.0) +
                  rng.uniform(-0.1, 0.1, n_points), rng.uniform(-1.5, 1.5, n_points)], 1)
    sees = []
    for v in range(n):
        Xc = (X - C[v]) @ R[v].T
        sees.append(np.nonzero((Xc[:, 2] > 1.0) & (Xc[:, 2] < 15.0) &
                               (np.hypot(Xc[:, 0], Xc[:, 1]) < np.tan(np.radians(50.0)) * Xc[:, 2]))[0])
    plist = [(i, i + k) for i in range(n) for k in range(1, reach + 1) if i + k < n]
    s = assemble(R, C, X, sees, plist, rng, rot_noise=rot_noise, dir_noise=dir_noise, drop=0.1)
    s["wrong_pair"] = None
    if wrong:
        s["wrong_pair"] = plist.index((5, 7))
        t = rng.normal(size=3)
        s["rel_t"][s["wrong_pair"]] = t / np.linalg.norm(t)
    return s


def scene_boundaries(seed=13, n=300, reach=3, hub_pairs=80, per_cluster=12, big=2100):
    """(c) n views on a ring, each looking outwards at the clusters of 12 points in front of itself and of its 3
    neighbours on either side, paired with its next 3; a hub above the ring that sees the clusters of the 80 views it is
    paired with (every second view); and four small groups beside the ring:
      short    views s0, s1, s2, pairs (s0, s1), (s0, s2): the wedge at s0 shares exactly 7 features (min_shared - 1)
      exact    the same with exactly 8
      big      views g0, g1, g2 that all see the same 2100 points: three wedges of more than max_shared features
      repeat   views r0, r1, r2: pair (r0, r1) names three features of r0 twice (the second time with another feature of
               r1), before and after the true match in its inlier list
      behind   views h0, h1, h2: pair (h0, h1) has its translation reversed, so that every point is behind a camera
    -> the scene, with the group's pair indices under its name"""
    rng = np.random.default_rng(seed)
    th = 2.0 * np.pi * np.arange(n) / n
    radius = 20.0
    out = np.stack([np.cos(th), np.sin(th), np.zeros(n)], 1)
    C = [radius * out[i] + rng.uniform(-0.1, 0.1, 3) for i in range(n)]
    R = [gs.random_rotation(rng, 0.05) @ look_at(C[i], (radius + 6.0) * out[i]) for i in range(n)]
    X = [(radius + 6.0) * out[i] + rng.uniform(-0.7, 0.7, 3) for i in range(n) for _ in range(per_cluster)]
    cluster = [list(range(per_cluster * i, per_cluster * (i + 1))) for i in range(n)]
    sees = [sum((cluster[(i + d) % n] for d in range(-reach, reach + 1)), []) for i in range(n)]
    plist = gs.ring_pairs(n, reach)
    hub = n
    partners = list(range(0, 2 * hub_pairs, 2))
    C.append(np.array([0.3, -0.2, 30.0]))
    R.append(look_at(C[hub], np.zeros(3), up=(0.0, 1.0, 0.0)))
    sees.append(sum((cluster[j] for j in partners), []))
    plist += [(hub, j) if q % 2 else (j, hub) for q, j in enumerate(partners)]
    groups = {}

    def group(name, origin, n_common, n_own):
        """three views in a row looking at a cloud: `n_common` points all three see, n_own more for each of the two pairs
        of the first view"""
        v0, p0 = len(C), len(X)
        for q in range(3):
            C.append(origin + np.array([1.1 * q, 0.0, 0.1 * q]))
            R.append(gs.random_rotation(rng, 0.05) @ look_at(C[-1], origin + np.array([1.0, 6.0, 0.0])))
        X.extend(origin + np.array([1.0, 6.0, 0.0]) + rng.uniform(-1.5, 1.5, 3) for _ in range(n_common + 2 * n_own))
        common = list(range(p0, p0 + n_common))
        own1 = list(range(p0 + n_common, p0 + n_common + n_own))
        own2 = list(range(p0 + n_common + n_own, p0 + n_common + 2 * n_own))
        sees.extend([common + own1 + own2, common + own1, common + own2])
        groups[name] = dict(views=[v0, v0 + 1, v0 + 2], pairs=[len(plist), len(plist) + 1])
        plist.extend([(v0, v0 + 1), (v0 + 2, v0)])

    group("short", np.array([60.0, 0.0, 0.0]), 7, 13)
    group("exact", np.array([60.0, 20.0, 0.0]), 8, 12)
    group("big", np.array([60.0, 40.0, 0.0]), big, 0)
    groups["big"]["pairs"].append(len(plist))
    plist.append((groups["big"]["views"][1], groups["big"]["views"][2]))
    group("repeat", np.array([60.0, 60.0, 0.0]), 20, 5)
    group("behind", np.array([60.0, 80.0, 0.0]), 20, 5)
    s = assemble(np.stack(R), np.stack(C), np.stack(X), sees, plist, rng)
    s.update(groups, hub=hub)
    c = s["call"]
    # repeat: three more matches of pair (r0, r1), each naming a feature of r0 that a true match names, with the r1 feature
    # of another match; the pair's inlier list is re-shuffled with them in it, so some come before the true match
    k = groups["repeat"]["pairs"][0]
    o0, o1 = int(c["offsets"][k]), int(c["offsets"][k + 1])
    extra_i, extra_j = c["match_i"][o0:o0 + 3].copy(), c["match_j"][o0 + 3:o0 + 6].copy()
    for name, extra in (("match_i", extra_i), ("match_j", extra_j)):
        c[name] = np.concatenate([c[name][:o1], extra, c[name][o1:]])
    c["offsets"] = c["offsets"].copy()
    c["offsets"][k + 1:] += 3
    i0, i1 = int(c["inl_off"][k]), int(c["inl_off"][k + 1])
    c["inl_idx"] = np.concatenate([c["inl_idx"][:i0], rng.permutation(o1 - o0 + 3).astype(np.uint32), c["inl_idx"][i1:]])
    c["inl_off"] = c["inl_off"].copy()
    c["inl_off"][k + 1:] += (o1 - o0 + 3) - (i1 - i0)
    groups["repeat"]["features"] = extra_i.tolist()
    # behind: the reversed translation
    s["rel_t"][groups["behind"]["pairs"][0]] *= -1.0
    return s
