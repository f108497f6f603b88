"""Seeded pair lists that take sfmloc_tracks_build's device primitives past their smallest configuration: the
multi-block scan of csrc/tracks.hip (k_trk_scan_block / k_scan_excl / k_trk_scan_add) and the radix sort of
csrc/radix_sort.h.  No device here: the cases are inputs, what each is for is asserted in test_tracks_cases_cpu.py.

What a case controls: n = view_off[-1] (all feature rows) sets the key bits of the sort, radix_key_bits(n - 1), and the
length n + 1 of the flags scan; m = the rows some match touches sets the blocks of the sort and of the heads scan; a
component's label is its smallest row, so the rows a case deals out choose the digits."""
from collections.abc import Mapping

import numpy as np

LENGTHS = (64, 2, 3, 17, 40, 2, 2, 9)
FOUR_PASS_OFF = (0, 300, 2 ** 16 + 5, 2 ** 24 - 7, 2 ** 24 + 1000, 2 ** 24 + 40000, 2 ** 24 + 2 ** 16)


def radix_key_bits(max_key):
    """csrc/radix_sort.h radix_key_bits: the key bits a sort of keys 0..max_key looks at"""
    return int(max_key).bit_length()


# ---- edges -----------------------------------------------------------------------------------------------------------

def join(nodes, rng):
    """edges of a random spanning tree over nodes [(view, feature), ...] plus about 30 % extra ones, none inside a view"""
    edges = []
    for i in range(1, len(nodes)):
        js = [j for j in range(i) if nodes[j][0] != nodes[i][0]]
        edges.append((nodes[js[int(rng.integers(len(js)))]], nodes[i]))
    for _ in range(int(0.3 * (len(nodes) - 1) + rng.random())):
        i, j = (int(x) for x in rng.choice(len(nodes), 2, replace=False))
        if nodes[i][0] != nodes[j][0]:
            edges.append((nodes[i], nodes[j]))
    return edges


def join_conflict(a, b, rng):
    """two trees that share a view, joined by one cross edge: one component with two features of that view"""
    assert {v for v, _ in a} & {v for v, _ in b}
    cross = [(x, y) for x in a for y in b if x[0] != y[0]]
    return join(a, rng) + join(b, rng) + [cross[int(rng.integers(len(cross)))]]


def assemble(view_off, edges, rng):
    """edges [((va, fa), (vb, fb)), ...] -> (pairs [n, 2] ascending (I, J), offsets, match_i, match_j) as
    sfmloc_tracks_build takes them; the matches inside a pair are shuffled"""
    by_pair = {}
    for (va, fa), (vb, fb) in edges:
        assert va != vb and fa < view_off[va + 1] - view_off[va] and fb < view_off[vb + 1] - view_off[vb]
        if va > vb:
            va, fa, vb, fb = vb, fb, va, fa
        by_pair.setdefault((va, vb), []).append((fa, fb))
    pairs, offsets, mi, mj = [], [0], [], []
    for p in sorted(by_pair):
        ms = np.array(by_pair[p], np.uint32)[rng.permutation(len(by_pair[p]))]
        pairs.append(p)
        mi.append(ms[:, 0])
        mj.append(ms[:, 1])
        offsets.append(offsets[-1] + len(ms))
    return (np.array(pairs, np.uint32).reshape(-1, 2), np.array(offsets, np.uint64), np.concatenate(mi), np.concatenate(mj))


def reversed_pair_list(pairs, offsets, match_i, match_j):
    """the same matches with the pair list reversed and the matches inside every pair reversed"""
    offsets = np.asarray(offsets, np.int64)
    return (np.ascontiguousarray(pairs[::-1]), np.concatenate([[0], np.cumsum(np.diff(offsets)[::-1])]).astype(np.uint64),
            np.ascontiguousarray(match_i[::-1]), np.ascontiguousarray(match_j[::-1]))


# ---- dealing features out --------------------------------------------------------------------------------------------

class Dealer:
    """Hands every component distinct views and a feature of each that no other component has.  pools[v] = the features
    of view v that may be dealt (a seeded shuffle).  balanced: a component takes the views with the most features left
    (ties at random), which empties equal pools exactly; otherwise views are drawn with weight = features left."""

    def __init__(self, pools, rng, balanced):
        self.pools = [list(rng.permutation(np.asarray(p, np.int64))) for p in pools]
        self.rng, self.balanced, self.dealt = rng, balanced, 0

    def views(self, length, must=(), avoid=()):
        left = np.array([0 if v in avoid or v in must else len(p) for v, p in enumerate(self.pools)], np.float64)
        k = length - len(must)
        assert (left > 0).sum() >= k, "not enough views with features left"
        if self.balanced:
            order = np.lexsort((self.rng.random(len(left)), -left))[:k]
        else:
            order = self.rng.choice(len(left), k, replace=False, p=left / left.sum())
        return list(must) + [int(v) for v in order]

    def take(self, views):
        self.dealt += len(views)
        return sorted((v, int(self.pools[v].pop())) for v in views)

    def plain(self, length):
        return self.take(self.views(length))

    def conflict(self, la, lb, first=None):
        """-> (a, b): two node lists over distinct views each that share one view; first = a view a must contain"""
        a = self.take(self.views(la, must=() if first is None else (first,)))
        shared = [v for v, _ in a if v != first and self.pools[v]]
        b = self.take(self.views(lb, must=(shared[int(self.rng.integers(len(shared)))],),
                                 avoid=() if first is None else (first,)))
        return a, b


def lengths_to(total, cycle, reserve=0):
    """component lengths cycling through `cycle` that sum to total - reserve exactly (none of length 1)"""
    out, left, i = [], total - reserve, 0
    while left > 0:
        n = min(cycle[i % len(cycle)], left)
        if left - n == 1:
            n = left if n + 1 <= max(cycle) else n - 1
        out.append(n)
        left -= n
        i += 1
    assert sum(out) == total - reserve and min(out) >= 2
    return out


def _mixed(view_off, lengths, conflicts, rng, balanced=True, pools=None, joins=0):
    """plain components of the given lengths and `conflicts` = [(la, lb), ...] conflict components; `joins` of the plain
    ones are then joined in twos that share a view, by one cross edge each -> pair list, m"""
    view_off = np.asarray(view_off, np.int64)
    if pools is None:
        pools = [np.arange(view_off[v + 1] - view_off[v]) for v in range(len(view_off) - 1)]
    d = Dealer(pools, rng, balanced)
    edges = []
    for la, lb in conflicts:                                   # first: they need a shared view with features left
        edges += join_conflict(*d.conflict(la, lb), rng)
    # (weighted draws: the long components first, while every view still has features)
    comps = [d.plain(n) for n in (sorted(lengths, reverse=True) if not balanced else lengths)]
    for c in comps:
        edges += join(c, rng)
    order = rng.permutation(len(comps))
    for i, j in zip(order[0::2], order[1::2]):
        cross = [(x, y) for x in comps[i] for y in comps[j] if x[0] != y[0]]
        if joins and cross and {v for v, _ in comps[i]} & {v for v, _ in comps[j]}:
            edges.append(cross[int(rng.integers(len(cross)))])
            joins -= 1
    assert joins == 0
    rng.shuffle(edges)
    return assemble(view_off, edges, rng), d.dealt


# ---- the cases -------------------------------------------------------------------------------------------------------

def _rows(n, seed):
    """8 views, n rows: radix_key_bits(n - 1) = 8 at 256 (one pass: the result ends in the scratch pair), 9 at 257"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.concatenate([np.arange(8) * 32, [n]])
    pl, m = _mixed(view_off, [8, 2, 3, 5, 2, 4] * 7, [(3, 2), (2, 2), (4, 3)], rng)
    return view_off, pl, None, 2, m


def _touched(m, n, seed):
    """8 views, exactly m touched rows of n: m is dealt out, not found by trial"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.concatenate([[0], np.cumsum([n // 8 + (1 if v < n % 8 else 0) for v in range(8)])])
    conflicts = [(3, 2), (2, 2), (5, 3), (2, 4)]
    pl, dealt = _mixed(view_off, lengths_to(m, (8, 2, 3, 5, 2, 4, 7), reserve=sum(a + b for a, b in conflicts)),
                       conflicts, rng)
    assert dealt == m
    return view_off, pl, None, 2, m


def _wide(per_view, seed, all_conflict=False):
    """64 views x per_view features, about 2 500 components whose lengths cycle through LENGTHS, 40 conflict joins (or
    every component one): more than 40 blocks of touched rows, a 64-view track has its equal keys spread over all"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.arange(65) * per_view
    lengths = [LENGTHS[i % 8] for i in range(2500)]
    if all_conflict:
        pl, m = _mixed(view_off, [], [(n, 2) for n in lengths], rng)
    else:
        pl, m = _mixed(view_off, lengths, [(LENGTHS[(3 * i) % 8], LENGTHS[(3 * i + 1) % 8]) for i in range(40)], rng)
    return view_off, pl, None, 2, m


def _low_byte_zero(seed):
    """8 views x 65 536 features, 256 components whose smallest row is a multiple of 256 in view 0: pass 0 of the sort
    puts every key of a block into bucket 0, so the ranks inside a block reach 1023 and come from all 16 waves"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.arange(9) * 65536
    d = Dealer([np.arange(256) * 256] + [np.arange(65536)] * 7, rng, balanced=True)
    edges = []
    for i in range(256):
        if i % 40 == 7:                                          # seven conflict components, their labels in view 0 too
            edges += join_conflict(*d.conflict(4, 3, first=0), rng)
        else:
            edges += join(d.take(d.views((8, 6, 8, 8, 5, 8, 8, 3)[i % 8], must=(0,))), rng)
    rng.shuffle(edges)
    return view_off, assemble(view_off, edges, rng), None, 2, d.dealt


def _four_pass(seed):
    """six views up to 2^24 + 2^16 rows (25 key bits: four passes), features from the first and last 750 of each view so
    that labels lie on both sides of 2^24; the flags scan has some 16 450 block totals: 17 chunks in k_scan_excl"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.array(FOUR_PASS_OFF, np.int64)
    size = np.diff(view_off)
    pools = [np.unique(np.concatenate([np.arange(min(750, s)), np.arange(max(0, s - 750), s)])) for s in size]
    lengths = [(2, 3, 6, 2, 4)[i % 5] for i in range(1500)]
    pl, m = _mixed(view_off, lengths, [], rng, balanced=False, pools=pools, joins=12)
    return view_off, pl, None, 2, m


def _zigzag(seed):
    """one path of 3 000 rows alternating between views 0 and 1, its edges shuffled: one conflict component, counted once
    and emitting nothing, whose hooking needs many passes; plus 50 pairs between views 2 and 3"""
    rng = np.random.Generator(np.random.PCG64(seed))
    view_off = np.array([0, 2000, 4000, 4100, 4200])
    path = [(i % 2, ((7 if i % 2 == 0 else 11) * (i // 2)) % 1500) for i in range(3000)]
    assert len(set(path)) == 3000
    edges = [(path[i], path[i + 1]) for i in range(2999)]
    fa, fb = rng.permutation(100)[:50], rng.permutation(100)[:50]
    edges += [((2, int(a)), (3, int(b))) for a, b in zip(fa, fb)]
    rng.shuffle(edges)
    return view_off, assemble(view_off, edges, rng), None, 2, 3100


def _derived(base, view_use=None, min_length=None):
    view_off, pl, use, ml, m = CASES.built(base)
    return view_off, pl, use if view_use is None else view_use(len(view_off) - 1), ml if min_length is None else min_length, m


_BUILDERS = {
    "rows256": lambda: _rows(256, 1),
    "rows257": lambda: _rows(257, 2),
    "touched1023": lambda: _touched(1023, 1023, 3),              # n + 1 = 1024: the flags scan fills one block exactly
    "touched1024": lambda: _touched(1024, 1024, 4),              # n + 1 = 1025: a second block with the total alone
    "touched1025": lambda: _touched(1025, 1280, 5),
    "rows65536": lambda: _wide(1024, 6),
    "rows65537plus": lambda: _wide(1025, 7),
    "low_byte_zero": lambda: _low_byte_zero(8),
    "four_pass": lambda: _four_pass(9),
    "zigzag": lambda: _zigzag(10),
    "all_conflict": lambda: _wide(1024, 11, all_conflict=True),
    "all_short": lambda: _derived("rows65536", min_length=65),
    "masked": lambda: _derived("rows65537plus", view_use=lambda nv: (np.arange(nv) % 3 != 0).astype(np.uint8)),
}


class _Cases(Mapping):
    """name -> (view_off, (pairs, offsets, match_i, match_j), view_use, min_length), built on first use and cached"""

    def __init__(self):
        self._built = {}

    def built(self, name):
        if name not in self._built:
            self._built[name] = _BUILDERS[name]()
        return self._built[name]

    def __getitem__(self, name):
        return self.built(name)[:4]

    def __iter__(self):
        return iter(_BUILDERS)

    def __len__(self):
        return len(_BUILDERS)

    def dealt(self, name):
        """the touched rows the case was built to have"""
        return self.built(name)[4]


CASES = _Cases()
