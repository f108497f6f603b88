"""The case library of the K3 form tests (test_k3_cases_cpu.py, test_gpu_k3_forms.py): image pairs with an exact number
of putative matches, filtered by sfmloc_geometric_pairs, which copies a pair's list straight into K3's buffers and runs
it with min_putative = 0.  NumPy only (the `outliers85` content asks the oracle's sampler for one sample).

A scene is one map per (content, ransac_round): views 0 .. N-1 are the first images of the N = len(SIZES) pairs, one
per size, and view N is the one second image -- the query side of K3 -- whose rows are the concatenation of the pairs'
second-image points; pair k's match_j point into its own slice.  (The second image stands last so that a first image
can have view id 0: the id of the FIRST image is the pair's sampling stream.  sfmloc_map_create takes ids below 2^24,
so the ids run from 0 to 2^24 - 2, the second image has 2^24 - 1.)  First and second images have different non-square
sizes.  SIZES are the list lengths at which K3's residuals per lane, instance or kernel change ("K3: which
form takes a list"); CONTENTS says what each content guarantees, test_k3_cases_cpu.py checks it on the oracle."""
import collections
import functools

import numpy as np

SIZES = (7, 8, 17, 18, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4097)
WH1, WH2 = (800, 600), (960, 540)       # first images, the second image
SEED = 0x5f3759df12345678               # params.seed (sfmloc_default_params) = oracle.pipeline.geometric_match's default
GEOM_PRECISION = 4.0
ID_TOP = (1 << 24) - 1                  # the largest view id sfmloc_map_create takes
BOUNDARIES = (64, 256, 512, 1024)       # `ties`: a group lies across list positions b - 1 | b
GROUP_SIZES = (2, 3, 5, 8)              # ... of that many correspondences; the group at the very end has END_GROUP
END_GROUP = 4
LATE_ITER = 9                           # `outliers85`: the iteration whose sample is all inliers
CLEAN_NOISE_PX = 0.002                  # uniform, per coordinate
TIE_NOISE_PX = 0.05

# content -> the ransac_round budgets it runs at.  36: the uniform phase is 33 > kF2Batch iterations, a second batch;
# 2: wide_b0 = 2, the smallest wide grid; 4 096 (the map side's default) on the sizes up to 512 only
BUDGETS = collections.OrderedDict([
    ("clean", (25, 2, 3, 36, 4096)), ("outliers30", (25,)), ("outliers85", (25,)), ("outliers100", (25,)), ("ties", (25,)),
    ("shuffled", (25,)), ("degenerate_line", (25,)), ("degenerate_point", (25,)), ("collinear", (25,))])
# (degenerate_line and degenerate_point have no model; collinear is the rank-deficient case that HAS one: with both
# images on a line the reference's algorithm keeps the pair -- see collinear())
BIG_BUDGET_MAX_SIZE = 512

Scene = collections.namedtuple("Scene", "content budget sizes view_id view_off view_wh kpt desc matches")


def view_ids(n_first):
    """ids of the first images (ascending from 0, the last one 2^24 - 2) and of the second image"""
    ids = [1009 * i for i in range(n_first)]
    ids[-1] = ID_TOP - 1
    return np.array(ids + [ID_TOP], np.uint32)


def _rot(a, b, c):
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def two_views(n, rng):
    """n points seen by two pinhole cameras: exact projections [n, 2] into a WH1 and a WH2 image, all inside"""
    f1, f2 = 700.0, 820.0
    R = _rot(*rng.uniform(-0.15, 0.15, 3))
    t = rng.uniform(-1.0, 1.0, 3) + np.array([1.5, 0.0, 0.0])
    a, b = np.zeros((0, 2)), np.zeros((0, 2))
    while len(a) < n:
        uv = rng.uniform([10.0, 10.0], [WH1[0] - 10.0, WH1[1] - 10.0], (2 * n + 16, 2))
        depth = rng.uniform(4.0, 12.0, len(uv))
        X = np.stack([(uv[:, 0] - WH1[0] / 2) / f1 * depth, (uv[:, 1] - WH1[1] / 2) / f1 * depth, depth], 1)
        Y = X @ R.T + t
        pq = f2 * Y[:, :2] / Y[:, 2:3] + np.array([WH2[0] / 2, WH2[1] / 2])
        ok = (Y[:, 2] > 1.0) & (pq[:, 0] > 10) & (pq[:, 0] < WH2[0] - 10) & (pq[:, 1] > 10) & (pq[:, 1] < WH2[1] - 10)
        a, b = np.concatenate([a, uv[ok]]), np.concatenate([b, pq[ok]])
    return a[:n], b[:n]


def uniform_points(n, wh, rng):
    return rng.uniform([0.0, 0.0], [float(wh[0]), float(wh[1])], (n, 2))


Pair = collections.namedtuple("Pair", "kp1 kp2 mi mj groups")   # mj index kp2 (the pair's own slice)


def _inliers(m, rng, noise):
    a, b = two_views(m, rng)
    return a + rng.uniform(-noise, noise, a.shape), b + rng.uniform(-noise, noise, b.shape)


def _identity(a, b, groups=()):
    m = len(a)
    return Pair(a, b, np.arange(m, dtype=np.uint32), np.arange(m, dtype=np.uint32), tuple(groups))


def clean(m, rng, stream):
    """every match an inlier, noise far below a pixel: the best k is all of them"""
    return _identity(*_inliers(m, rng, CLEAN_NOISE_PX))


def _outliers(m, rng, share, keep=()):
    a, b = _inliers(m, rng, CLEAN_NOISE_PX)
    free = np.setdiff1d(np.arange(m), np.asarray(keep, np.int64))
    out = rng.permutation(free)[:int(share * m)]
    b[out] = uniform_points(len(out), WH2, rng)
    return _identity(a, b)


def outliers30(m, rng, stream):
    """30 % of the second-image points replaced by uniform ones"""
    return _outliers(m, rng, 0.30)


def first_sample(m, stream, it):
    """the 7 list positions AC-RANSAC's uniform phase draws at iteration `it` of a list of m on `stream`"""
    from oracle import oracle_c
    return np.asarray(oracle_c.ac_sample(7, np.arange(m, dtype=np.int32), SEED, oracle_c.STAGE_FMATRIX, int(stream), it),
                      np.int64)[:7]


def outliers85(m, rng, stream):
    """85 % replaced (int(0.85 m)).  A 7-sample of such a list is all inliers once in 600 000 draws, so the inliers
    include the sample of iteration LATE_ITER of the pair's stream: the model appears late in the first batch, every
    earlier iteration has none."""
    return _outliers(m, rng, 0.85, keep=first_sample(m, stream, LATE_ITER) if m > 7 else ())


def outliers100(m, rng, stream):
    """both sides uniform: the pair must be dropped"""
    return _identity(uniform_points(m, WH1, rng), uniform_points(m, WH2, rng))


def tie_groups(m):
    """list positions of the planted groups: one across each boundary of BOUNDARIES that lies inside the list, one at
    the very end (where the list is long enough to hold it apart from the others)"""
    groups = []
    for b, g in zip(BOUNDARIES, GROUP_SIZES):
        if m > b:
            lo = b - (g + 1) // 2
            hi = min(lo + g, m)
            groups.append(tuple(range(lo, hi)))
    used = {p for g in groups for p in g}
    end = tuple(range(m - min(END_GROUP, max(2, m // 4)), m))
    if m >= 8 and not used.intersection(end):
        groups.append(end)
    return tuple(groups)


def ties(m, rng, stream):
    """every match an inlier at TIE_NOISE_PX of noise, and groups of 2 .. 8 correspondences whose keypoints are bit-equal
    in both images (distinct rows, the same float32 coordinates), so that their residuals are equal under every model"""
    a, b = _inliers(m, rng, TIE_NOISE_PX)
    groups = tie_groups(m)
    for g in groups:
        src = int(rng.integers(0, m))
        a[list(g)], b[list(g)] = a[src], b[src]
    return _identity(a, b, groups)


def shuffled(m, rng, stream):
    """clean, the list in random order, the first image three times as many rows as matches (the rest uniform)"""
    a, b = _inliers(m, rng, CLEAN_NOISE_PX)
    kp1 = uniform_points(3 * m, WH1, rng)
    rows = rng.permutation(3 * m)[:m]
    kp1[rows] = a
    order = rng.permutation(m)
    return Pair(kp1, b, rows[order].astype(np.uint32), order.astype(np.uint32), ())


def degenerate_line(m, rng, stream):
    """the first image's points on one line, the second's uniform: every 7-point sample is rank-deficient (its null space
    holds the rank-one matrices that send the whole line to zero, whose residuals are 0 / 0), and nothing fits"""
    t = rng.uniform(0.0, 1.0, m)
    a = np.array([60.0, 80.0]) + t[:, None] * np.array([640.0, 410.0])
    return _identity(a, uniform_points(m, WH2, rng))


def collinear(m, rng, stream):
    """both images' points on one line each.  x2^T F x1 is then a bilinear form in the two line parameters: four numbers
    that any seven matches force to zero, so EVERY matrix of a sample's (five-dimensional) null space fits EVERY match to
    rounding, and the pair survives with residuals that are rounding noise -- the order of its list is the arithmetic of
    the rank-deficient solve, bit for bit"""
    t = rng.uniform(0.0, 1.0, m)
    s = np.clip(t + rng.uniform(-0.05, 0.05, m), 0.0, 1.0)
    a = np.array([60.0, 80.0]) + t[:, None] * np.array([640.0, 410.0])
    b = np.array([900.0, 50.0]) + s[:, None] * np.array([-800.0, 430.0])
    return _identity(a, b)


def degenerate_point(m, rng, stream):
    """one repeated point in each image"""
    return _identity(np.tile([[301.25, 417.5]], (m, 1)), np.tile([[622.75, 88.5]], (m, 1)))


CONTENTS = collections.OrderedDict([
    ("clean", clean), ("outliers30", outliers30), ("outliers85", outliers85), ("outliers100", outliers100),
    ("ties", ties), ("shuffled", shuffled), ("degenerate_line", degenerate_line),
    ("degenerate_point", degenerate_point), ("collinear", collinear)])
# Seeds (pair()): 1 000 000 x the content's position + 5 000 x the budget + m, plus a bump where the oracle says a seed's
# case is not what its content claims (test_k3_cases_cpu.py states the claims; a bump is found by running that test).
# So far none.
SEED_BUMP = {}


def sizes_of(budget):
    return tuple(s for s in SIZES if budget < 4096 or s <= BIG_BUDGET_MAX_SIZE)


@functools.lru_cache(maxsize=None)
def pair(content, m, budget, stream):
    """one pair of a scene (read-only float32 keypoints)"""
    seed = 1000000 * (list(CONTENTS).index(content) + 1) + 5000 * budget + m + SEED_BUMP.get((content, m, budget), 0)
    p = CONTENTS[content](m, np.random.Generator(np.random.PCG64(seed)), stream)
    kp1, kp2 = np.ascontiguousarray(p.kp1, np.float32), np.ascontiguousarray(p.kp2, np.float32)
    assert len(p.mi) == len(p.mj) == m and len(kp2) == m and kp1.shape[1] == 2
    for a in (kp1, kp2, p.mi, p.mj):
        a.setflags(write=False)
    return Pair(kp1, kp2, p.mi, p.mj, p.groups)


def descriptors(n, seed):
    return np.random.Generator(np.random.PCG64(seed)).integers(0, 256, (n, 64), dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def scene(content, budget):
    """the map of one content at one budget (module docstring): Scene(view_id, view_off, view_wh, kpt [rows, 2] float32,
    desc [rows, 64], matches {(k, N): (match_i, match_j)} over view indices)"""
    sizes = sizes_of(budget)
    N = len(sizes)
    ids = view_ids(N)
    pairs = [pair(content, m, budget, int(ids[k])) for k, m in enumerate(sizes)]
    rows = [len(p.kp1) for p in pairs] + [sum(len(p.kp2) for p in pairs)]
    view_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    kpt = np.concatenate([p.kp1 for p in pairs] + [p.kp2 for p in pairs]).astype(np.float32)
    desc = descriptors(len(kpt), 77 + budget)
    matches, base = {}, 0
    for k, p in enumerate(pairs):
        matches[(k, N)] = (p.mi.copy(), (p.mj.astype(np.int64) + base).astype(np.uint32))
        if content == "clean":               # guided matching compares descriptors: a match is a near copy (6 bits flipped)
            d = desc[int(view_off[N]) + base + p.mj.astype(np.int64)].copy()
            d[:, :6] ^= 1
            desc[int(view_off[k]) + p.mi.astype(np.int64)] = d
        base += len(p.kp2)
    wh = np.array([WH1] * N + [WH2], np.uint32)
    return Scene(content, budget, sizes, ids, view_off, wh, kpt, desc, matches)


def all_scenes():
    return [(c, b) for c, budgets in BUDGETS.items() for b in budgets]


def view_kpts(sc):
    off = sc.view_off.astype(np.int64)
    return [sc.kpt[off[v]:off[v + 1]] for v in range(len(sc.view_id))]


def view_descs(sc):
    off = sc.view_off.astype(np.int64)
    return [sc.desc[off[v]:off[v + 1]] for v in range(len(sc.view_id))]


def ranges(sc):
    """the pairs of a scene by the form that owns them: (name, lo, hi, {pair: lists}) for the list lengths up to 512,
    513 .. 1 024, 1 025 .. 2 048 and beyond"""
    out = []
    for name, lo, hi in (("le512", 0, 512), ("le1024", 513, 1024), ("le2048", 1025, 2048), ("large", 2049, 1 << 30)):
        sub = {k: v for k, v in sc.matches.items() if lo <= len(v[0]) <= hi}
        if sub:
            out.append((name, lo, hi, sub))
    return out


def expectations(oracle_c, content, ransac_round, guided=False):
    """oracle.pipeline.geometric_match on the scene's lists: {(k, N): (i[], j[])} for the pairs that survive"""
    from oracle import pipeline as opipe
    sc = scene(content, ransac_round)
    return opipe.geometric_match(view_kpts(sc), sc.view_wh, sc.view_id, sc.matches, ransac_round=ransac_round,
                                 geom_precision=GEOM_PRECISION, seed=SEED, guided=guided,
                                 descs=view_descs(sc) if guided else None)


# ----- the further cases (test_gpu_k3_forms.py, `default` and `wide4` only) -----
def many_pairs(n_sel):
    """n_sel first images of 20 rows against one second image (256: the wide form's last list; 257: the plain form)"""
    rng = np.random.Generator(np.random.PCG64(4200 + n_sel))
    pairs = [_identity(*_inliers(20, rng, CLEAN_NOISE_PX)) for _ in range(n_sel)]
    return _assemble(pairs, ids=np.arange(n_sel + 1, dtype=np.uint32) * 3 + 1)


def large_views(n_views=10, m=2049):
    """more lists beyond kFMaxM than k_fmatrix_large has slots (kFLargeSlots = 8): two are taken in a second turn"""
    rng = np.random.Generator(np.random.PCG64(4300))
    pairs = [_outliers(m, rng, 0.3) for _ in range(n_views)]
    return _assemble(pairs, ids=np.arange(n_views + 1, dtype=np.uint32) * 5 + 2)


def last_query_row():
    """a second image of exactly 65 535 rows and one clean list of 64 whose match_j include 65 534: the 16-bit query
    index of the packed match key"""
    rng = np.random.Generator(np.random.PCG64(4400))
    p = _identity(*_inliers(64, rng, CLEAN_NOISE_PX))
    kp2 = uniform_points(65535, WH2, rng)
    rows = np.sort(rng.permutation(65534)[:63])
    rows = np.concatenate([rows, [65534]])[rng.permutation(64)]
    kp2[rows] = p.kp2
    return _assemble([Pair(p.kp1, kp2, p.mi, rows.astype(np.uint32), ())], ids=np.array([11, 12], np.uint32))


def _assemble(pairs, ids):
    N = len(pairs)
    rows = [len(p.kp1) for p in pairs] + [sum(len(p.kp2) for p in pairs)]
    view_off = np.concatenate([[0], np.cumsum(rows)]).astype(np.uint32)
    kpt = np.concatenate([p.kp1 for p in pairs] + [p.kp2 for p in pairs]).astype(np.float32)
    matches, base = {}, 0
    for k, p in enumerate(pairs):
        matches[(k, N)] = (np.asarray(p.mi, np.uint32), (np.asarray(p.mj, np.int64) + base).astype(np.uint32))
        base += len(p.kp2)
    wh = np.array([WH1] * N + [WH2], np.uint32)
    return Scene("further", 25, tuple(len(p.mi) for p in pairs), ids, view_off, wh, kpt, descriptors(len(kpt), 78), matches)


def expect_scene(sc, budget=25):
    from oracle import pipeline as opipe
    return opipe.geometric_match(view_kpts(sc), sc.view_wh, sc.view_id, sc.matches, ransac_round=budget,
                                 geom_precision=GEOM_PRECISION, seed=SEED)


# ----- handing expectations to a child process -----
def save_expectations(path, sets):
    """sets: {set name: {(a, b): (i[], j[])}} -> one .npz (a set with no surviving pair keeps its name)"""
    flat = {}
    for s, exp in sets.items():
        flat[f"{s}|pairs"] = np.array(sorted(exp), np.int64).reshape(-1, 2)
        for (a, b), (i, j) in exp.items():
            flat[f"{s}|{a}|{b}"] = np.stack([np.asarray(i, np.uint32), np.asarray(j, np.uint32)])
    np.savez(path, **flat)


def load_expectations(path):
    sets = {}
    with np.load(path) as z:
        for key in z.files:
            if key.endswith("|pairs"):
                s = key[:-6]
                sets[s] = {(int(a), int(b)): (z[f"{s}|{a}|{b}"][0], z[f"{s}|{a}|{b}"][1]) for a, b in z[key]}
    return sets
