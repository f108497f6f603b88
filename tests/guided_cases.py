"""Scenes of the guided-matching tests (params.guided_matching, -gm) and what both of their sides share: the CPU test
(tests/test_guided_cases_cpu.py) asserts on the oracle's side that every scene reaches the path it is for, the GPU test
(tests/test_gpu_guided.py) and its child tool (tests/tools/guided_forms_cases.py) take the same scenes through the device.
No GPU and no product code here: synthdata, NumPy, and the oracle's `localize` handed in by the caller.

A Scene is a map, its queries in the order they run, a view shortlist per query (None = the whole map) and the parameters
that the device map and the oracle both get.  Every scene is a function of a seed; SEEDS holds the ones the tests use, and
the CPU test is what says that a seed is fit -- a seed whose scene misses its property is replaced, the property is not.

band_stats restates Geometry_guided_matching's band for one view in NumPy (matrix form, as oracle/twins_np.py does), so
that the edges of the selection rule -- equal best and second best, a best of 0, one candidate in the band, none -- are
counted from the data and not assumed."""
from dataclasses import dataclass, field

import numpy as np

import synthdata as synth

TILE_NQ = (40, 511, 512, 513, 1024, 1025)      # around kGTile = 512 query positions per LDS tile of k_guided_rows
NO_DIST = 1 << 30                               # band_stats: "no such candidate"


@dataclass
class Scene:
    name: str
    m: object
    queries: list
    params: dict = field(default_factory=lambda: dict(ransac_round=25))
    sels: list = None                           # per query: ascending view indices, or None

    def sel(self, k):
        return None if self.sels is None else self.sels[k]


def small_map(seed, **kw):
    """the 40 x 400 map of test_gpu_geom.make_scene"""
    args = dict(n_views=40, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=140)
    args.update(kw)
    return synth.make_map(seed, **args)


def plant_twice(m, seed, per_view):
    """Per view, `per_view` rows without a landmark become copies of a landmark row's descriptor with one to three bits
    flipped: both rows then match the same query feature, at different distances -- a query feature twice in the view's
    putative list, which is what makes "the LAST putative match with this query feature" (featDist) a choice."""
    rng = np.random.Generator(np.random.PCG64(seed))
    for v in range(m.n_views):
        a, b = int(m.view_off[v]), int(m.view_off[v + 1])
        lm = a + np.nonzero(m.row_landmark[a:b] >= 0)[0]
        free = a + np.nonzero(m.row_landmark[a:b] < 0)[0]
        k = min(per_view, len(lm), len(free))
        if k == 0:
            continue
        src = rng.choice(lm, k, replace=False)
        dst = rng.choice(free, k, replace=False)
        d = m.desc[src].copy()
        for r in range(k):
            for p in rng.choice(synth.VALID_BITS, int(rng.integers(1, 4)), replace=False):
                d[r, p >> 3] ^= np.uint8(1 << (p & 7))
        m.desc[dst] = d
    return m


def plant_same_descriptor(q, seed, n):
    """`n` correctly placed copies get a twin elsewhere in the image: a feature that was clutter takes their descriptor
    and keeps its own position.  The map row of such a copy then has two equal nearest neighbours in the query, fails the
    putative ratio test, and -- unless the twin happens to lie in the row's band -- comes back as a guided match whose
    query feature no putative match of the view has: the one case without a featDist entry (SfMDataUtils.cpp:105-106)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    inl, free = np.nonzero(q.is_inlier)[0], np.nonzero(q.landmark < 0)[0]
    n = min(n, len(inl), len(free))
    src, dst = rng.choice(inl, n, replace=False), rng.choice(free, n, replace=False)
    q.desc[dst] = q.desc[src]
    return q


def inlier_last(q):
    """the query's last feature changes places with a correctly placed copy: the position that is alone in the last LDS
    tile when nq = 513 or 1 025 (and closes a full tile when nq = 512 or 1 024) is then one that guided matches name"""
    a, b = int(np.nonzero(q.is_inlier)[0][0]), len(q.desc) - 1
    for arr in (q.desc, q.kpt_xy, q.landmark, q.is_inlier):
        arr[[a, b]] = arr[[b, a]]
    return q


def tile_edges(seed):
    m = small_map(seed)
    qs = []
    for k, nq in enumerate(TILE_NQ):
        if nq == 40:        # a query this small still has to reach min_putative = 16 in a view: every feature a copy
            qs.append(synth.make_query(m, 100 * seed + k, n_feat=40, n_copies=40, outlier_frac=0.1, place=k % 4))
        else:
            qs.append(inlier_last(synth.make_query(m, 100 * seed + k, n_feat=nq, n_copies=230, outlier_frac=0.3, place=k % 4)))
    return Scene("tile_edges", m, qs)


def radial(seed):
    """one tile_edges query (nq = 513) under a pinhole_radial_k3 intrinsic"""
    s = tile_edges(seed)
    s.m.intrinsic = tuple(s.m.intrinsic[:3]) + (0.05, -0.02, 0.001)
    return Scene("radial", s.m, [s.queries[TILE_NQ.index(513)]])


def ragged_map(seed):
    m = synth.make_map(seed, n_views=20, desc_per_view=700, views_per_place=10, landmarks_per_place=500, obs_per_view=260,
                       ragged=True)
    return plant_twice(m, seed + 1, 6)


def ragged(seed):
    m = ragged_map(seed)
    qs = [plant_same_descriptor(synth.make_query(m, 100 * seed + k, n_feat=600 + 50 * k, n_copies=260, outlier_frac=0.3,
                                                 place=k % 2), seed + 10 + k, 10) for k in range(2)]
    return Scene("ragged", m, qs)


def shortlist(seed):
    """the ragged map; every other view: views of the query's place (some survive) and of the other (none does), while
    the odd views of the query's place stay outside"""
    s = ragged(seed)
    sel = np.arange(0, s.m.n_views, 2, dtype=np.uint32)
    return Scene("shortlist", s.m, s.queries, sels=[sel for _ in s.queries])


def reuse(seed, tiny_seed=0):
    """one context: 1 025 features on the whole map, 40 features of the same place on a shortlist, the first again.  The
    second query's views are views the first one left guided rows and lists in."""
    s = tile_edges(seed)
    big = s.queries[TILE_NQ.index(1025)]
    tiny = synth.make_query(s.m, 100 * seed + 50 + tiny_seed, n_feat=40, n_copies=40, outlier_frac=0.1, place=big.place)
    sel = np.nonzero(s.m.view_place == big.place)[0].astype(np.uint32)[::2]
    return Scene("reuse", s.m, [big, tiny, big], sels=[None, sel, None])


def ties(seed, n_dup=30):
    """No bit flips on either side, so a true match has distance 0; `n_dup` matched features a second time (descriptor and
    keypoint) at the index of a feature that was clutter: a map row whose match is one of them finds best == second == 0
    and is rejected.  A query of 160 features leaves rows with two, one and no candidate in their band."""
    m = small_map(seed, map_flips=0)
    q = synth.make_query(m, 100 * seed, n_feat=160, n_copies=110, outlier_frac=0.1, query_flips=0)
    src = np.nonzero(q.is_inlier)[0][:n_dup]
    dst = np.nonzero(q.landmark < 0)[0][:n_dup]
    assert len(src) == len(dst) == n_dup
    q.desc[dst] = q.desc[src]
    q.kpt_xy[dst] = q.kpt_xy[src]
    q.landmark[dst] = q.landmark[src]
    q.is_inlier[dst] = True
    return Scene("ties", m, [q])


def k4_walk(seed):
    """put_count in [16, 127] for every view that reaches K4: the backward walk in LDS"""
    m = plant_twice(small_map(seed), seed + 1, 4)
    qs = [plant_same_descriptor(synth.make_query(m, 100 * seed + k, n_feat=600, n_copies=190, outlier_frac=0.3, place=k),
                                seed + 10 + k, 10) for k in range(2)]
    return Scene("k4_walk", m, qs)


def k4_hash_big(seed):
    """views of 513 .. 1 024 putative matches, three queries in a row: the block-wide LDS form of K3 first, then -- the
    map's credit -- k_fmatrix_fast<W, 1024>; K4's hash table"""
    m = synth.make_map(seed, n_views=4, desc_per_view=1100, views_per_place=4, landmarks_per_place=1300, obs_per_view=1000,
                       map_flips=8)
    plant_twice(m, seed + 1, 12)
    qs = [plant_same_descriptor(synth.make_query(m, 100 * seed + k, n_feat=1200, n_copies=1000, outlier_frac=0.1,
                                                 query_flips=10), seed + 10 + k, 12) for k in range(3)]
    return Scene("k4_hash_big", m, qs, params=dict(ransac_round=25, p3p_max_iteration=300))


def k4_hash_huge(seed):
    """views of 1 025 .. 2 048 putative matches, three queries in a row: k_fmatrix_filter first, then
    k_fmatrix_fast<4, 2048, wide>"""
    m = synth.make_map(seed, n_views=3, desc_per_view=2100, views_per_place=3, landmarks_per_place=2500, obs_per_view=2000,
                       map_flips=8)
    plant_twice(m, seed + 1, 12)
    qs = [plant_same_descriptor(synth.make_query(m, 100 * seed + k, n_feat=2300, n_copies=2000, outlier_frac=0.1,
                                                 query_flips=10), seed + 10 + k, 12) for k in range(3)]
    return Scene("k4_hash_huge", m, qs, params=dict(ransac_round=25, p3p_max_iteration=200))


def k4_global(seed):
    """views of more than kFMaxM = 2 048 putative matches: the global-store form of K3, K4's walk in global memory"""
    m = synth.make_map(seed, n_views=3, desc_per_view=2600, views_per_place=3, landmarks_per_place=2900, obs_per_view=2500,
                       map_flips=8)
    plant_twice(m, seed + 1, 12)
    qs = [plant_same_descriptor(synth.make_query(m, 100 * seed, n_feat=2700, n_copies=2600, outlier_frac=0.05,
                                                 query_flips=10), seed + 10, 12)]
    return Scene("k4_global", m, qs, params=dict(ransac_round=25, p3p_max_iteration=300))


def pair_images(seed):
    """two images of 2 100 features of one place (the pair path, sfmloc_geometric_pairs)"""
    return synth.make_map(seed, n_views=2, desc_per_view=2100, views_per_place=2, landmarks_per_place=2500, obs_per_view=1900,
                          map_flips=8)


SCENES = dict(tile_edges=tile_edges, radial=radial, ragged=ragged, shortlist=shortlist, reuse=reuse, ties=ties,
              k4_walk=k4_walk, k4_hash_big=k4_hash_big, k4_hash_huge=k4_hash_huge, k4_global=k4_global)
SEEDS = dict(tile_edges=161, radial=161, ragged=162, shortlist=162, reuse=161, ties=163, k4_walk=164, k4_hash_big=165,
             k4_hash_huge=166, k4_global=169, pair_images=168)
FORM_SCENES = ("tile_edges", "k4_hash_big", "k4_hash_huge", "k4_global")     # what the K3 form knobs are run on
_made = {}


def scene(name):
    """the scene of SEEDS[name] (made once per process; nobody writes to it)"""
    if name not in _made:
        _made[name] = SCENES[name](SEEDS[name])
    return _made[name]


def form_queries(name):
    """indices of a form scene's queries that the knob runs take"""
    return [TILE_NQ.index(513)] if name == "tile_edges" else list(range(len(scene(name).queries)))


_oracle = {}


def expected(name, localize):
    """the oracle's intermediates for every query of a scene with guided matching on (once per process)"""
    if name not in _oracle:
        s = scene(name)
        _oracle[name] = [localize(s.m, q.desc, q.kpt_xy, (q.width, q.height), view_sel=s.sel(k), guided=True, **s.params)
                         for k, q in enumerate(s.queries)]
    return _oracle[name]


def guided_lists(m, exp, v):
    """(i[], j[]) of view v in an oracle result"""
    off, n = int(m.view_off[v]), int(exp["geo_count"][v])
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32)
    return exp["geo_idx"][off:off + n], exp["geo_j"][off:off + n]


def surviving(exp):
    """views that passed the F-matrix filter (their guided list may still be empty)"""
    return sorted(int(v) for v, r in exp["f_stats"].items() if r["n"] > 0)


def band_stats(m, q, exp, v):
    """Geometry_guided_matching's band for every row of view v under the oracle's F and errorMax (exp["f_stats"][v]), in
    matrix form: -> dict(n_band[n_v], best[n_v], second[n_v] (Hamming distances; NO_DIST where there is no such
    candidate), margin = the smallest |e - threshold| / threshold over all (row, query feature) pairs, defining_pair = the
    (row, query feature) of the inlier whose residual IS errorMax, margin_defining = its relative distance, margin_others =
    the smallest over every other pair)."""
    st = exp["f_stats"][v]
    off, end = int(m.view_off[v]), int(m.view_off[v + 1])
    (w1, h1), (w2, h2) = (int(t) for t in m.view_wh[v]), (q.width, q.height)

    def norm_mat(w, h):
        s = 1.0 / np.sqrt(float(w) * float(h))
        return np.array([[s, 0, -0.5 * w * s], [0, s, -0.5 * h * s], [0, 0, 1.0]])
    F = norm_mat(w2, h2).T @ np.asarray(st["F"], np.float64).reshape(3, 3) @ norm_mat(w1, h1)
    thr = (np.sqrt(st["errmax"]) * np.sqrt(float(w2) * float(h2))) ** 2
    x1 = np.c_[m.kpt_xy[off:end].astype(np.float64), np.ones(end - off)]
    q6 = synth.round6(q.kpt_xy).astype(np.float64)              # the .feat round trip of the query's positions
    x2 = np.c_[q6, np.ones(len(q6))]
    lines = x1 @ F.T
    num = lines @ x2.T
    e = num * num / (lines[:, 0] ** 2 + lines[:, 1] ** 2)[:, None]
    b1 = np.unpackbits(m.desc[off:end], axis=1).astype(np.float32)      # (counts <= 512: exact in float32)
    b2 = np.unpackbits(np.asarray(q.desc, np.uint8), axis=1).astype(np.float32)
    ham = (b1.sum(1)[:, None] + b2.sum(1)[None, :] - 2.0 * (b1 @ b2.T)).astype(np.int64)
    inside = e < thr
    d = np.where(inside, ham, NO_DIST)
    n_band = inside.sum(1)
    if d.shape[1] >= 2:
        two = np.partition(d, 1, axis=1)[:, :2]
        best, second = two[:, 0], two[:, 1]
    else:
        best = d.min(1) if d.shape[1] else np.full(len(d), NO_DIST)
        second = np.full(len(d), NO_DIST)
    rel = np.abs(e - thr) / thr
    margin = float(rel.min()) if e.size else np.inf
    # the pair the threshold was taken from: errorMax is the residual of AC-RANSAC's last inlier, so that pair's error
    # EQUALS the threshold but for the rounding of two different routes (normalised frame / pixels)
    p = int(st["inliers"][-1])
    di, dj = int(exp["put_i"][off + p]), int(exp["put_j"][off + p])
    margin_defining = float(rel[di, dj])
    rel[di, dj] = np.inf
    margin_others = float(rel.min()) if e.size else np.inf
    return dict(n_band=n_band, best=best, second=second, margin=margin, threshold=thr, defining_pair=(di, dj),
                margin_defining=margin_defining, margin_others=margin_others)


def no_dist_matches(m, exp, v):
    """guided matches of view v at rows with a landmark whose query feature no putative match of the view has: the ones
    matchProviderToMatchSet skips for want of a featDist entry (SfMDataUtils.cpp:105-106)"""
    off, c = int(m.view_off[v]), int(exp["put_count"][v])
    gi, gj = guided_lists(m, exp, v)
    has = np.isin(gj, exp["put_j"][off:off + c])
    return int(((m.row_landmark[off + gi.astype(np.int64)] >= 0) & ~has).sum())


def twice_in_putative(m, exp, v):
    """query features that occur twice in view v's putative list with different distances AND are the query feature of a
    guided match at a row with a landmark (so that K4 looks them up)"""
    off, c = int(m.view_off[v]), int(exp["put_count"][v])
    pj, pd = exp["put_j"][off:off + c], exp["put_d"][off:off + c]
    gi, gj = guided_lists(m, exp, v)
    wanted = set(int(j) for i, j in zip(gi, gj) if m.row_landmark[off + int(i)] >= 0)
    out = []
    for j in np.unique(pj):
        w = np.nonzero(pj == j)[0]
        if len(w) >= 2 and len(set(int(x) for x in pd[w])) >= 2 and int(j) in wanted:
            out.append(int(j))
    return out
