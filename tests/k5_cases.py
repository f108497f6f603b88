"""The case library of the K5 form tests (test_k5_cases_cpu.py, test_gpu_k5_forms.py): single views with an exact number
of 2D-3D correspondences, resected by sfmloc_sfm_resect, which copies a view's observation list straight into K5's
buffers.  NumPy only.

A content is a function (n, seed) -> (pixels [n, 2], landmarks [n, 3]): one view on the shared pinhole intrinsic
INTRINSIC, list index = position in the arrays (assemble() gives the landmarks ascending ids in that order).  SIZES are
the correspondence counts at which K5's evaluators change ("K5: which evaluator a round runs"); CASES is the
fixed list of (content, n) the tests run, each with its own seed and its own id_view -- the view's AC-RANSAC sampling
stream.  expectations() is the oracle's resection of every case, computed once per process."""
import collections
import functools
from concurrent.futures import ThreadPoolExecutor

import numpy as np

# focal, ppx, ppy of the one pinhole intrinsic; the image is 640 x 480.  The focal length is short on purpose: K5 works
# on K^-1-normalised points with logalpha0 = log10(pi) (SfM_Localizer::Localize), so a residual e counts as unlikely in
# proportion to pi e, while pixels scattered over the image fall within e of anything with probability pi e f^2 / (w h)
# at most.  With f^2 < w h random pixels support no model (the `none` and `late` contents rely on it); with f = 800
# on this image AC-RANSAC calls nearly any pose of 257 random pixels meaningful.
INTRINSIC = (400.0, 320.0, 240.0)
WIDTH, HEIGHT = 640, 480
NOISE_PX = 0.5
SIZES = (11, 12, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 4095, 4096,
         4097)
EDGE_SIZES = (64, 65, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 4096, 4097)
NONE_SIZES = (12, 257, 1025)
DEGENERATE_SIZES = tuple(n for n in SIZES if n <= 257)
PAIR_DISTANCES = (1, 64, 256, 1024)    # list distances of planted copies: one lane-row, rows of a wave, runs, waves
DEGENERATE_COPIES = 40
ID_VIEW0 = 1000                        # id_view of CASES[0]; CASES[i] has ID_VIEW0 + i
# a second set of streams for a handle that lists the cases in another order (view ids must ascend): id_view of the
# case at position j of that handle's list is ID_VIEW_ALT0 + j
ID_VIEW_ALT0 = 5000

Case = collections.namedtuple("Case", "name content n seed id_view")


def _camera(rng):
    """a world -> camera rotation (rows right, down, forward) and a centre"""
    a, b, c = rng.uniform(-0.4, 0.4, 3)
    ca, sa, cb, sb, cc, sc = np.cos(a), np.sin(a), np.cos(b), np.sin(b), np.cos(c), np.sin(c)
    Rx = np.array([[1, 0, 0], [0, ca, -sa], [0, sa, ca]])
    Ry = np.array([[cb, 0, sb], [0, 1, 0], [-sb, 0, cb]])
    Rz = np.array([[cc, -sc, 0], [sc, cc, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx, rng.uniform(-3.0, 3.0, 3)


def _scene(n, rng):
    """n landmarks in front of a camera and their noise-free projections"""
    f, ppx, ppy = INTRINSIC
    R, C = _camera(rng)
    uv = rng.uniform([20.0, 20.0], [WIDTH - 20.0, HEIGHT - 20.0], (n, 2))
    depth = rng.uniform(4.0, 20.0, n)
    Xc = np.stack([(uv[:, 0] - ppx) / f * depth, (uv[:, 1] - ppy) / f * depth, depth], 1)
    X = Xc @ R + C                                   # R^T Xc + C
    Xc = (X - C) @ R.T
    pix = f * Xc[:, :2] / Xc[:, 2:3] + np.array([ppx, ppy])
    return pix, X


def _noisy(n, rng, outlier_frac, n_outliers=None):
    """-> pixels, landmarks: projections with NOISE_PX of noise, a share of them replaced by a random pixel"""
    pix, X = _scene(n, rng)
    pix = pix + rng.normal(0.0, NOISE_PX, (n, 2))
    n_out = int(round(outlier_frac * n)) if n_outliers is None else n_outliers
    out = rng.permutation(n)[:n_out]
    pix[out] = rng.uniform([0.0, 0.0], [WIDTH, HEIGHT], (n_out, 2))
    return pix, X


def clean(n, seed):
    """about 25 % outliers, half-pixel noise"""
    return _noisy(n, np.random.Generator(np.random.PCG64(seed)), 0.25)


def _pairs(n, rng):
    """disjoint (lower, higher) index pairs at the PAIR_DISTANCES that fit n, about n / 3 pairs in all, spread evenly over
    the distances; the largest distance is placed first (it has the fewest free places)"""
    dists = [d for d in PAIR_DISTANCES if d < n]
    used = np.zeros(n, bool)
    pairs = []
    for left, d in zip(range(len(dists), 0, -1), reversed(dists)):
        want, got = -(-(n // 3 - len(pairs)) // left), 0   # (what a distance could not place goes to the shorter ones)
        for i in rng.permutation(n - d):
            if got == want:
                break
            if not used[i] and not used[i + d]:
                used[i] = used[i + d] = True
                pairs.append((int(i), int(i + d)))
                got += 1
    return sorted(pairs)


def _tied(n, seed, ulp):
    rng = np.random.Generator(np.random.PCG64(seed))
    pix, X = _noisy(n, rng, 0.25)
    pairs = _pairs(n, rng)
    for j, (lo, hi) in enumerate(pairs):            # inliers and outliers alike: whatever `lo` is
        X[hi] = X[lo]
        pix[hi] = pix[lo]
        if ulp:                                     # alternate: the copy one ulp above / below in x
            pix[hi, 0] = np.nextafter(pix[lo, 0], np.inf if j % 2 == 0 else -np.inf)
    return pix, X, pairs


def ties(n, seed):
    """exact copies of correspondences (same X, same pixel) at list distances 1, 64, 256 and 1 024"""
    return _tied(n, seed, False)[:2]


def near_ties(n, seed):
    """as ties, the copy's x pixel one ulp away, the direction alternating from pair to pair"""
    return _tied(n, seed, True)[:2]


def planted_pairs(n, seed):
    """the (lower, higher) list positions of the copies ties(n, seed) and near_ties(n, seed) plant"""
    return _tied(n, seed, False)[2]


def exact(n, seed):
    """every correspondence a noise-free projection"""
    return _scene(n, np.random.Generator(np.random.PCG64(seed)))


def late(n, seed):
    """85 % outliers"""
    return _noisy(n, np.random.Generator(np.random.PCG64(seed)), 0.85, n_outliers=int(0.85 * n))


def none(n, seed):
    """every pixel random: no model"""
    return _noisy(n, np.random.Generator(np.random.PCG64(seed)), 1.0)


def degenerate_copies(n):
    return min(DEGENERATE_COPIES, n // 2)


def degenerate(n, seed):
    """the first degenerate_copies(n) correspondences (40 from n = 80 on) are copies of three, the rest clean"""
    rng = np.random.Generator(np.random.PCG64(seed))
    pix, X = _noisy(n, rng, 0.25)
    m = degenerate_copies(n)
    src = m + rng.permutation(n - m)[:3]
    for i in range(m):
        pix[i], X[i] = pix[src[i % 3]], X[src[i % 3]]
    return pix, X


CONTENTS = collections.OrderedDict([
    ("clean", (clean, SIZES)), ("ties", (ties, EDGE_SIZES)), ("near_ties", (near_ties, EDGE_SIZES)),
    ("exact", (exact, EDGE_SIZES)), ("late", (late, EDGE_SIZES)), ("none", (none, NONE_SIZES)),
    ("degenerate", (degenerate, DEGENERATE_SIZES))])

# Seeds: 100 000 x the content's position + n, plus a bump where the oracle says that seed's case is not what its
# content claims (test_k5_cases_cpu.py states the claims; a bump is found by running that test).
# So far: a first sample that holds both members of a planted pair gives a model of a handful of exact inliers with a
# negative NFA, sampling narrows to them and the view fails (near_ties 64 and 257, ties 512); five `late` seeds met an
# all-inlier sample within their first 64 iterations.
SEED_BUMP = {("near_ties", 64): 1, ("near_ties", 257): 1, ("ties", 512): 1, ("late", 256): 1, ("late", 512): 1,
             ("late", 2048): 1, ("late", 2049): 2, ("late", 4097): 2}


def _make_cases():
    rows = []
    for ci, (content, (_, sizes)) in enumerate(CONTENTS.items()):
        for n in sizes:
            rows.append((n, ci, content))
    rows.sort()                                     # ascending n, then content order
    return tuple(Case(f"{content}_{n}", content, n, 100000 * ci + n + SEED_BUMP.get((content, n), 0), ID_VIEW0 + i)
                 for i, (n, ci, content) in enumerate(rows))


CASES = _make_cases()
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _arrays(content, n, seed):
    pix, X = CONTENTS[content][0](n, seed)
    pix, X = np.ascontiguousarray(pix, np.float64), np.ascontiguousarray(X, np.float64)
    assert pix.shape == (n, 2) and X.shape == (n, 3)
    pix.setflags(write=False)
    X.setflags(write=False)
    return pix, X


def case_arrays(case):
    """-> pixels [n, 2], landmarks [n, 3] of a case (read-only, cached)"""
    return _arrays(case.content, case.n, case.seed)


def assemble(cases, id_views=None):
    """Any list of cases as one sfmloc_sfm_desc (the arrays capi.Sfm takes, as adjust_scene.two_pass_case gives them):
    one view per case in list order, id_view = the case's own unless id_views names others (strictly ascending either
    way); every view has its own landmarks, one observation each, ids ascending in list order; one shared pinhole
    intrinsic; a pose per view (identity: the resection replaces it)."""
    ids = np.array([c.id_view for c in cases] if id_views is None else id_views, np.uint32)
    assert len(ids) == len(cases) and np.all(np.diff(ids.astype(np.int64)) > 0), "id_view must ascend"
    nv = len(cases)
    pix = np.concatenate([case_arrays(c)[0] for c in cases])
    X = np.concatenate([case_arrays(c)[1] for c in cases])
    n_obs = len(pix)
    return dict(view_id=ids, view_intrinsic=np.zeros(nv, np.uint32), view_pose=np.arange(nv, dtype=np.uint32),
                intrinsic_type=np.zeros(1, np.uint32), intrinsic=np.array([list(INTRINSIC) + [0.0, 0.0, 0.0]]),
                pose_valid=np.ones(nv, np.uint8), pose_R=np.tile(np.eye(3).reshape(1, 9), (nv, 1)),
                pose_C=np.zeros((nv, 3)), landmark_id=np.arange(n_obs, dtype=np.uint32) * 2 + 1, landmark_X=X,
                obs_off=np.arange(n_obs + 1, dtype=np.uint64),
                obs_view=np.repeat(np.arange(nv, dtype=np.uint32), [c.n for c in cases]), obs_x=pix)


def expect(case, oracle_c, id_view=None):
    """the oracle's resection of one case on the stream id_view (the case's own by default): the record
    adjust_scene.oracle_resect gives per view"""
    import adjust_scene as AS
    return AS.oracle_resect(assemble([case], None if id_view is None else [id_view]), oracle_c)[0][0]


def descending(cases):
    """-> the cases by descending n and the ids they get in that order (ID_VIEW_ALT0 + position)"""
    order = sorted(cases, key=lambda c: (-c.n, c.id_view))
    return order, [ID_VIEW_ALT0 + j for j in range(len(order))]


_EXPECTED = {}


def expectations(oracle_c, alt=False):
    """{case name: expect(case)} for all of CASES, computed once per process (the C oracle releases the GIL: eight
    threads); alt=True: on the streams descending(CASES) gives them."""
    if alt not in _EXPECTED:
        oracle_c.lib()                              # (loaded before the threads ask for it)
        jobs = list(zip(*descending(CASES))) if alt else [(c, None) for c in CASES]
        with ThreadPoolExecutor(8) as pool:
            got = list(pool.map(lambda j: expect(j[0], oracle_c, j[1]), jobs))
        _EXPECTED[alt] = {j[0].name: e for j, e in zip(jobs, got)}
    return _EXPECTED[alt]


FIELDS = ("ran", "ok", "n_obs", "n", "iters", "errmax", "nfa", "P", "R", "center", "inliers", "inl_raw")


def save_expectations(path, sets):
    """sets: {set name: {case name: record}} -> one .npz"""
    flat = {}
    for s, exp in sets.items():
        for name, e in exp.items():
            for f in FIELDS:
                if f in e:
                    flat[f"{s}/{name}/{f}"] = np.asarray(e[f])
    np.savez(path, **flat)


def load_expectations(path):
    sets = {}
    with np.load(path) as z:
        for key in z.files:
            s, name, f = key.split("/")
            v = z[key]
            sets.setdefault(s, {}).setdefault(name, {})[f] = v if v.ndim else v.item()
    return sets
