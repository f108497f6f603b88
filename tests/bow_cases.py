"""Inputs and CPU references for the BoW view shortlist (K8: k_bow_dist, k_bow_topk, k_bow_keys, k_bow_merge_select).
No GPU here: tests/test_bow_cases_cpu.py checks that every case reaches what it is for and that the C oracle agrees
with the references; tests/test_gpu_bow_edges.py runs the kernels on the same cases.

Maps are (view_id, view_off, desc) with ONE all-zero descriptor row per view (K8 never reads descriptors), so 40 000
views cost 2.5 MB.  View ids ascend with a stride; the 40 000-view maps' ids end at 2**24 - 1, the largest a map takes.

References (a case names its own):
  R1  exact integers.  Vectors and query take values in {0..3}, dim <= 500: every squared distance is an integer below
      2^24, so float32 is exact in ANY summation order; the reference is np.int64 arithmetic.
  R2  dim = 1.  The distance is one IEEE float32 subtract and one multiply (the 63 idle lanes add +0); the reference is
      the same two operations in np.float32.
  R3  real-valued vectors.  Distances in float64; the float32 result of any order is within
      g = (ceil(dim / 64) + 8) * 2**-24 relative: 3 roundings per term (subtract, square, its first add), at most
      ceil(dim / 64) - 1 further adds in a lane and 6 in the butterfly, all of non-negative terms.  With T the k-th
      smallest float64 distance, every view below T (1 - 2 g) must be selected and none above T (1 + 2 g) may be; the
      cases are drawn so that at most 4 views lie in between (asserted on the CPU).
The selection under R1 / R2 is the k smallest by (distance, position in the candidate list), returned ascending.

NaN distances are left out on purpose: the reference's behaviour on them is undefined (its k-NN search compares with <),
and the sign bit of a NaN that an arithmetic operation produces differs between hosts, so no CPU reference could state
the bits a shortlist should rank.
"""
import functools

import numpy as np

SIZES = (2, 63, 64, 65, 1023, 1024, 1025, 16383, 16384, 16385, 40000)
REG_LIMIT = 16 * 1024            # k_bow_topk keeps its distances in registers up to this many candidates
DIMS = (1, 24, 63, 64, 65, 127, 128, 129, 500, 1000)
RUN = 40                         # length of a tie run
PAD = np.uint64(0xFFFFFFFFFFFFFFFF)
INF_BITS, MIN_NORMAL_BITS = 0x7F800000, 0x00800000
INF_GROUP = 50


def ks_for(n):
    return sorted({k for k in (1, 2, 1023, 1024, 1025, n - 1) if 1 <= k < n})


def chunk_of(n):
    """views per thread in k_bow_topk's order-preserving compaction"""
    return (n + 1023) // 1024


def map_arrays(n, stride=3, last_id=None):
    """-> view_id, view_off, desc of an n-view map with one zero descriptor row per view"""
    first = 5 if last_id is None else last_id - stride * (n - 1)
    assert first >= 0
    view_id = (first + stride * np.arange(n, dtype=np.int64)).astype(np.uint32)
    return view_id, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 64), np.uint8)


def map_ids(n):
    """the ids every select / keys case of n views is given"""
    return map_arrays(n, last_id=2 ** 24 - 1 if n == 40000 else None)[0]


def geometry_kwargs(n):
    """the least geometry a map needs for the stages after K8 to run (no landmark observed anywhere)"""
    return dict(view_wh=np.tile(np.array([[640, 480]], np.uint32), (n, 1)), kpt_xy=np.zeros((n, 2), np.float32),
                row_landmark=np.full(n, -1, np.int32), landmark_id=np.array([7], np.uint32),
                landmark_X=np.zeros((1, 3)), intrinsic=(800.0, 320.0, 240.0))


def bits_of(d_f32):
    return np.ascontiguousarray(d_f32, np.float32).view(np.uint32)


class Case:
    """One map's BoW vectors, one query, and the selections (k, candidate list or None) asked of them."""

    def __init__(self, name, ref, bow, query, picks, meta=None):
        self.name, self.ref = name, ref
        self.bow = np.ascontiguousarray(bow, np.float32).reshape(len(bow), -1)
        self.query = np.ascontiguousarray(query, np.float32).ravel()
        self.picks = picks
        self.meta = meta or {}
        self.n, self.dim = self.bow.shape

    def __repr__(self):
        return self.name

    @functools.cached_property
    def dist(self):
        """the reference's distance of every view: int64 (R1), float32 (R2), float64 (R3)"""
        if self.ref == "R1":
            d = self.bow.astype(np.int64) - self.query.astype(np.int64)
            return (d * d).sum(1)
        if self.ref == "R2":
            with np.errstate(over="ignore", under="ignore"):
                d = self.bow[:, 0] - self.query[0]
                return (d * d).astype(np.float32)
        d = self.bow.astype(np.float64) - self.query.astype(np.float64)
        return (d * d).sum(1)

    @functools.cached_property
    def dist_f32(self):
        """R1 / R2: the float32 distances every correct implementation gives, bit for bit"""
        assert self.ref in ("R1", "R2")
        return self.dist.astype(np.float32)

    def sort_key(self):
        return bits_of(self.dist) if self.ref == "R2" else self.dist        # non-negative floats order like their bits

    def expected(self, k, cand=None):
        """R1 / R2: the k smallest by (distance, position in the candidate list), ascending"""
        assert self.ref in ("R1", "R2")
        key = self.sort_key()
        if cand is not None:
            key = key[cand]
        pos = np.sort(np.lexsort((np.arange(len(key)), key))[:k])
        return (pos if cand is None else np.asarray(cand)[pos]).astype(np.uint32)

    def r3_band(self, k, cand=None):
        """R3: (views that must be selected, views that may be, the count in between)"""
        g = ((self.dim + 63) // 64 + 8) * 2.0 ** -24
        views = np.arange(self.n) if cand is None else np.asarray(cand, np.int64)
        d = self.dist[views]
        T = np.sort(d)[k - 1]
        must, may = views[d < T * (1 - 2 * g)], views[d <= T * (1 + 2 * g)]
        return must, may, len(may) - len(must)

    def check_r3(self, sel, k, cand=None):
        must, may, _ = self.r3_band(k, cand)
        sel = np.asarray(sel, np.int64)
        assert len(sel) == k and (np.diff(sel) > 0).all(), self.name
        assert np.isin(must, sel).all() and np.isin(sel, may).all(), (self.name, k)


def _cands(rng, n):
    """candidate lists of 16 384 (the register form's largest), 16 385 and 3 out of n views"""
    return [np.sort(rng.choice(n, m, replace=False)).astype(np.uint32) for m in (REG_LIMIT, REG_LIMIT + 1, 3)]


def _picks(rng, n, ks, with_cands):
    picks = [(k, None) for k in ks]
    if with_cands:
        for c in _cands(rng, n):
            picks += [(k, c) for k in sorted({1, 2, 1024, len(c) - 1}) if k < len(c)]
    return picks


# ----- R2: distance patterns -------------------------------------------------------------------------------------------
def _from_bits(t_bits):
    """bow values sqrt(t): the distances to a zero query are fl(fl(sqrt t)^2), within 2 ulp of t"""
    return np.sqrt(np.asarray(t_bits, np.uint32).view(np.float32).astype(np.float64)).astype(np.float32)


def _pattern_values(pattern, n, rng):
    if pattern == "uniform":
        return np.sqrt(rng.random(n)).astype(np.float32), {}
    if pattern == "top11":       # one value of the top 11 bits (pass 1 decides nothing), the low 21 bits random
        return _from_bits((0x1FC << 21) | rng.integers(1 << 10, (1 << 21) - (1 << 10), n)), {}
    if pattern == "top22":       # one value of the top 22 bits: passes 1 and 2 decide nothing
        return _from_bits((0x1FC << 21) | (0x2A5 << 10) | rng.integers(8, 1016, n)), {}
    if pattern == "all_equal":
        return np.full(n, 0.75, np.float32), {}
    assert pattern == "edge_values"
    v = np.sqrt(rng.random(n)).astype(np.float32)
    where = rng.permutation(n)
    n_zero, n_sub = min(3, n // 8), min(12, n // 4)
    g = min(INF_GROUP, n // 2)
    zero, sub, inf = where[:n_zero], where[n_zero:n_zero + n_sub], where[n_zero + n_sub:n_zero + n_sub + g]
    v[zero] = 0.0
    # |a - b| from 1e-23 to 1e-19: the squares run from below the smallest subnormal (-> 0) up to 1e-38
    v[sub] = (10.0 ** np.linspace(-23, -19, n_sub) * rng.choice([-1.0, 1.0], n_sub)).astype(np.float32)
    v[inf] = np.where(rng.random(g) < 0.5, -1e20, 1e20).astype(np.float32)            # 1e40 -> +inf
    return v, {"n_inf": g, "k_in_inf": n - g + g // 2}


@functools.lru_cache(maxsize=None)
def pattern_case(pattern, n):
    rng = np.random.Generator(np.random.PCG64([sum(map(ord, pattern)), n]))
    v, meta = _pattern_values(pattern, n, rng)
    ks = ks_for(n) if pattern == "uniform" else sorted({1, min(1024, n - 1), n - 1})
    if "k_in_inf" in meta:
        ks = sorted(set(ks) | {meta["k_in_inf"]})
    return Case(f"{pattern}-{n}", "R2", v[:, None], [0.0], _picks(rng, n, ks, n == 40000), meta)


PATTERNS = ("uniform", "top11", "top22", "all_equal", "edge_values")
PATTERN_SIZES = (REG_LIMIT, REG_LIMIT + 1, 40000)      # every pattern: at the register form's limit, and in the other form


def pattern_cases():
    out = [pattern_case("uniform", n) for n in SIZES]
    out += [pattern_case(p, n) for p in PATTERNS[1:] for n in PATTERN_SIZES]
    return out


def _value_pool(rng, n):
    """n bow values, ascending, whose float32 squares are distinct (and ascending)"""
    v = np.unique(rng.uniform(0.5, 1.5, 3 * n + 100).astype(np.float32))
    _, first = np.unique(v * v, return_index=True)
    v = v[first]
    return np.sort(rng.choice(v, n, replace=False))


def run_starts(n):
    """Where the tie runs go: across a thread's chunk boundary a third into the list, across index 64 * chunk (a wave
    boundary of the compaction), and at the end of the list; a run that does not fit a short list is dropped.
    -> [(name, start, length)]"""
    L, chunk = min(RUN, n), chunk_of(n)
    want = [("end", n - L), ("wave", 64 * chunk - L // 2), ("chunk", chunk * max(1, n // chunk // 3) - L // 2)]
    kept = []
    for name, s in want:
        if s >= 0 and s + L <= n and all(s + L <= a or a + L <= s for _, a, _ in kept):
            kept.append((name, s, L))
    return kept[::-1]


@functools.lru_cache(maxsize=None)
def tie_runs_case(n, k, variant):
    """Runs of RUN consecutive equal distances; the k-th smallest distance is one run's, and k takes its first
    (variant 0), its first half (1) or all (2) of that run -- fewer where k or the list is too short for it."""
    rng = np.random.Generator(np.random.PCG64([7, n, k, variant]))
    runs = run_starts(n)
    L = runs[0][2]
    cut = variant % len(runs)
    singles = n - L * len(runs)
    others = len(runs) - 1
    r = min((1, max(1, L // 2), L)[variant], k)
    r = max(r, k - singles - L * others)                   # (not enough other views to put below the run)
    less = k - r
    j = next(j for j in range(min(others, less // L), -1, -1) if 0 <= less - L * j <= singles)
    s = less - L * j
    other_runs = [i for i in rng.permutation(len(runs)) if i != cut]
    below = [("s", None)] * s + [("r", i) for i in other_runs[:j]]
    above = [("s", None)] * (singles - s) + [("r", i) for i in other_runs[j:]]
    groups = [below[i] for i in rng.permutation(len(below))] + [("r", cut)] + [above[i] for i in rng.permutation(len(above))]
    pool = _value_pool(rng, len(groups))
    v = np.zeros(n, np.float32)
    in_run = np.zeros(n, bool)
    for _, a, ln in runs:
        in_run[a:a + ln] = True
    single_pos = rng.permutation(np.nonzero(~in_run)[0])
    sp = 0
    for (kind, i), val in zip(groups, pool):
        if kind == "s":
            v[single_pos[sp]] = val
            sp += 1
        else:
            v[runs[i][1]:runs[i][1] + L] = val
    meta = {"runs": runs, "cut": runs[cut], "taken": r, "less": less}
    picks = _picks(rng, n, [k], n == 40000 and variant == 0 and k == 1024)
    return Case(f"tie_runs-{n}-k{k}-v{variant}", "R2", v[:, None], [0.0], picks, meta)


def tie_runs_cases(n):
    return [tie_runs_case(n, k, variant) for k in ks_for(n) for variant in range(3)]


# ----- R1 / R3: dimensions ----------------------------------------------------------------------------------------------
def _n_for_dim(dim):
    return {24: 40000, 500: 20000}.get(dim, 1500)      # the global-memory form at the two largest maps a test may build


@functools.lru_cache(maxsize=None)
def r1_case(dim):
    assert dim <= 500
    rng = np.random.Generator(np.random.PCG64([1, dim]))
    n = _n_for_dim(dim)
    bow = rng.integers(0, 4, (n, dim)).astype(np.float32)
    q = rng.integers(0, 4, dim).astype(np.float32)
    return Case(f"r1-dim{dim}", "R1", bow, q, _picks(rng, n, sorted({1, 2, 100, 1024, 1025, n - 1}), n > REG_LIMIT + 1))


@functools.lru_cache(maxsize=None)
def r3_case(dim):
    rng = np.random.Generator(np.random.PCG64([3, dim]))
    n = 1500
    bow = np.sqrt(rng.random((n, dim))).astype(np.float32)
    q = (bow[rng.integers(0, n)] + rng.normal(0, 0.02, dim)).astype(np.float32)
    cand = np.sort(rng.choice(n, 700, replace=False)).astype(np.uint32)
    return Case(f"r3-dim{dim}", "R3", bow, q, [(k, None) for k in (1, 2, 100, 1024, 1025, n - 1)] + [(100, cand)])


def dim_cases():
    return [r1_case(d) for d in DIMS if d <= 500] + [r3_case(d) for d in DIMS]


# ----- keys of a shard ---------------------------------------------------------------------------------------------------
def key_of(dist_f32, view_id):
    return (bits_of(dist_f32).astype(np.uint64) << np.uint64(32)) | np.asarray(view_id, np.uint64)


def expected_keys(case, view_id, knn):
    """the sorted (distance bits << 32 | view id) of the shard's min(knn, n) best, padded with ~0 up to knn"""
    sel = case.expected(min(knn, case.n))
    out = np.full(knn, PAD, np.uint64)
    out[:len(sel)] = np.sort(key_of(case.dist_f32[sel], np.asarray(view_id)[sel]))
    return out


@functools.lru_cache(maxsize=None)
def five_view_case():
    return Case("five-views", "R1", [[0, 1], [3, 3], [0, 1], [2, 0], [1, 1]], [1, 1], [])


# ----- merge of the gathered key lists ----------------------------------------------------------------------------------
def shard_ids(p, nv):
    """ascending view ids of shard p (no two shards share one; a shard's ids lie below the next shard's)"""
    return (np.arange(nv, dtype=np.int64) * 3 + 1 + p * 30000).astype(np.uint32)


class MergeCase:
    """keys [n_parts, part_stride] u64 as all-gathered; the local shard's ascending view ids; the shortlist size"""

    def __init__(self, name, keys, k, local_id, meta=None):
        self.name, self.k = name, k
        self.keys = np.ascontiguousarray(keys, np.uint64)
        self.n_parts, self.part_stride = self.keys.shape
        self.local_id = np.ascontiguousarray(local_id, np.uint32)
        self.n_views = len(self.local_id)
        self.meta = meta or {}

    def __repr__(self):
        return self.name

    def gathered(self):
        return self.keys[:, :self.k]

    def winners(self):
        """the k smallest of all keys that are not padding"""
        real = self.gathered().ravel()
        return np.sort(real[real != PAD])[:self.k]

    def expected(self):
        """brute force: of the winners, those whose id is the local shard's, as ascending local indices, padded with
        the phantom view n_views up to min(k, n_views)"""
        ids = {int(x) & 0xFFFFFFFF for x in self.winners()}
        mine = [i for i, vid in enumerate(self.local_id.tolist()) if vid in ids]
        n_pad = min(self.k, self.n_views)
        assert len(mine) <= n_pad
        return np.array(mine + [self.n_views] * (n_pad - len(mine)), np.uint32)

    def n_owned(self):
        return int((self.expected() != self.n_views).sum())


def _part(rng, ids, n_real, k, lo, hi, stride=None):
    """one shard's list: n_real keys of random views with distinct float32 distances in [lo, hi), ascending, padded to k"""
    out = np.full(stride or k, PAD, np.uint64)
    d = np.sort(rng.choice(np.unique(rng.uniform(lo, hi, 4 * n_real + 8).astype(np.float32)), n_real, replace=False))
    out[:n_real] = key_of(d, rng.choice(ids, n_real, replace=False))        # (ascending distances: ascending keys)
    return out


@functools.lru_cache(maxsize=None)
def merge_cases():
    rng = np.random.Generator(np.random.PCG64(88))
    out = []
    # cap: 8 x 1024 keys (kBowMergeMaxKeys), all 1024 winners in part 5; the same keys seen from shard 2, which owns none
    nv = [1500] * 8
    nv[5] = 2000
    keys = np.stack([_part(rng, shard_ids(p, nv[p]), 1024, 1024, *((0.1, 0.2) if p == 5 else (0.5, 1.0))) for p in range(8)])
    out.append(MergeCase("cap", keys, 1024, shard_ids(5, nv[5])))
    out.append(MergeCase("cap_none", keys, 1024, shard_ids(2, nv[2])))
    # short_shard: the local shard (part 1) has 5 views, k = 1024; three of them are among the winners
    keys = np.stack([_part(rng, shard_ids(p, 1500), 1024, 1024, 0.2, 0.8) for p in range(3)])
    keys[1] = PAD
    keys[1, :5] = np.sort(key_of(np.array([0.01, 0.3, 0.35, 0.9, 0.95], np.float32), shard_ids(1, 5)[[3, 0, 4, 1, 2]]))
    out.append(MergeCase("short_shard", keys, 1024, shard_ids(1, 5)))
    # cross_tie: k = 100; the 100th and the 101st smallest keys carry the same distance bits B, the 100th in part 0 (the
    # lower view id), the 101st in part 1
    B = np.float32(0.5)
    p0, p1 = _part(rng, shard_ids(0, 300), 99, 100, 0.1, 0.9), _part(rng, shard_ids(1, 300), 99, 100, 0.1, 0.9)

    def with_tie(part, n_small, ids, tie_view):
        d = (part[:99] >> np.uint64(32)).astype(np.uint32).view(np.float32)
        small = np.sort(d)[:n_small] * np.float32(0.25) + np.float32(0.1)             # < 0.35: below B
        large = np.sort(d)[n_small:] * np.float32(0.25) + np.float32(0.6)             # > 0.6: above B
        views = np.setdiff1d(np.arange(300), [tie_view])[:99]
        return np.sort(np.concatenate([key_of(small, ids[views[:n_small]]), key_of([B], ids[[tie_view]]),
                                       key_of(large, ids[views[n_small:]])]))
    keys = np.stack([with_tie(p0, 49, shard_ids(0, 300), 123), with_tie(p1, 50, shard_ids(1, 300), 45)])
    out.append(MergeCase("cross_tie_lo", keys, 100, shard_ids(0, 300), {"tie_view": 123, "tie_taken": True}))
    out.append(MergeCase("cross_tie_hi", keys, 100, shard_ids(1, 300), {"tie_view": 45, "tie_taken": False}))
    # mostly_pad: three real keys in all, two of them the local shard's (7 views)
    keys = np.full((4, 100), PAD, np.uint64)
    keys[0, 0] = key_of([np.float32(0.3)], shard_ids(0, 9)[[4]])[0]
    keys[2, :2] = np.sort(key_of(np.array([0.7, 0.2], np.float32), shard_ids(2, 7)[[1, 6]]))
    out.append(MergeCase("mostly_pad", keys, 100, shard_ids(2, 7)))
    # strided: part_stride_keys = 3 k; what lies between the lists would win, and is the local shard's, if it were read
    k = 64
    keys = np.stack([_part(rng, shard_ids(p, 400), 64, k, 0.2, 0.8, stride=3 * k) for p in range(3)])
    for p in range(3):
        keys[p, k:] = key_of(rng.uniform(0.001, 0.002, 2 * k).astype(np.float32), rng.choice(shard_ids(1, 400), 2 * k, replace=False))
    out.append(MergeCase("strided", keys, k, shard_ids(1, 400)))
    return out
