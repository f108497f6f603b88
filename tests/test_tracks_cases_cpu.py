"""CPU: the pair lists of tests/tracks_cases.py.  On every case the NumPy restatement of sfmloc_tracks
(structure_np.tracks, what test_gpu_tracks_sizes.py holds the device to) equals the plain dictionary union-find, and every
case is what it exists for: the row counts, key bits and block counts that take the scan of csrc/tracks.hip and the sort
of csrc/radix_sort.h through each of their paths.  Integers only, no tolerance."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import structure_np as tw  # noqa: E402
from test_structure_cpu import union_find_tracks  # noqa: E402
from tracks_cases import CASES, radix_key_bits  # noqa: E402

BOUNDARY = ("rows256", "rows257", "touched1023", "touched1024", "touched1025")
# name -> (n = all rows, m = touched rows (None: see below), radix_key_bits(n - 1))
SIZES = {"rows256": (256, None, 8), "rows257": (257, None, 9),
         "touched1023": (1023, 1023, 10), "touched1024": (1024, 1024, 10), "touched1025": (1280, 1025, 11),
         "rows65536": (65536, None, 16), "rows65537plus": (65600, None, 17), "low_byte_zero": (524288, None, 19),
         "four_pass": (2 ** 24 + 2 ** 16, None, 25), "zigzag": (4200, 3100, 13), "all_conflict": (65536, None, 16),
         "all_short": (65536, None, 16), "masked": (65600, None, 17)}

_twins = {}


def twin(name):
    if name not in _twins:
        view_off, pl, use, min_length = CASES[name]
        _twins[name] = tw.tracks(view_off, *pl, view_use=use, min_length=min_length)
    return _twins[name]


def touched_rows(name):
    view_off, pl, use, _ = CASES[name]
    ea, eb = tw.edges(view_off, *pl, view_use=use)
    return np.unique(np.concatenate([ea, eb]))


def blocks(count):
    return (count + 1023) // 1024


@pytest.mark.parametrize("name", list(CASES))
def test_twin_tracks_equal_a_plain_union_find(name):
    view_off, pl, use, min_length = CASES[name]
    t = twin(name)
    exp, counts = union_find_tracks(view_off, *pl, view_use=use, min_length=min_length)
    assert t["counts"] == counts
    off = t["off"].astype(np.int64)
    view, feat = t["view"].tolist(), t["feat"].tolist()
    got = [list(zip(view[off[k]:off[k + 1]], feat[off[k]:off[k + 1]])) for k in range(len(off) - 1)]
    assert got == exp
    assert sum(counts[1:]) == counts[0]


def test_what_the_cases_are_for():
    assert set(SIZES) == set(CASES)
    m = {}
    for name, (n, m_exact, bits) in SIZES.items():
        view_off = CASES[name][0]
        m[name] = len(touched_rows(name))
        assert int(view_off[-1]) == n and radix_key_bits(n - 1) == bits, name
        assert m_exact is None or m[name] == m_exact, name
        if CASES[name][2] is None:
            assert m[name] == CASES.dealt(name), name                    # every feature dealt out is matched
        assert (twin(name)["passes"] >= 3) or name in BOUNDARY, name    # hooking: more than one round of races
    assert len(CASES["rows256"][0]) - 1 == 8 and len(CASES["touched1024"][0]) - 1 == 8
    # the sort: one, two, three and four passes, so the result ends in either buffer pair
    assert {-(-b // 8) for _, _, b in SIZES.values()} == {1, 2, 3, 4}
    assert [-(-SIZES[k][2] // 8) for k in ("rows256", "rows257", "rows65536", "rows65537plus", "four_pass")] == [1, 2, 2, 3, 4]
    # blocks of the sort and of the heads scan (m), of the flags scan (n + 1): one, two with a single entry, 256 * nb
    # within and past one chunk of k_scan_excl, block totals past one chunk
    assert [blocks(m[k]) for k in ("touched1023", "touched1024", "touched1025")] == [1, 1, 2]
    assert [SIZES[k][0] + 1 for k in ("touched1023", "touched1024")] == [1024, 1025]
    assert [blocks(SIZES[k][0] + 1) for k in ("touched1023", "touched1024")] == [1, 2]
    assert 2 <= blocks(m["low_byte_zero"]) <= 4 and m["low_byte_zero"] >= 1024
    assert m["four_pass"] > 4096 and blocks(m["four_pass"]) >= 5
    assert min(m["rows65536"], m["rows65537plus"]) > 40000 and min(blocks(m["rows65536"]), blocks(m["rows65537plus"])) >= 40
    assert blocks(blocks(SIZES["four_pass"][0] + 1)) == 17 and SIZES["four_pass"][0] + 1 > 2 ** 20   # 16 449 totals
    # a 64-view track of rows65536: equal keys in at least 32 different blocks of the sort
    t = twin("rows65536")
    off = t["off"].astype(np.int64)
    k = int(np.nonzero(np.diff(off) == 64)[0][0])
    view_off = np.asarray(CASES["rows65536"][0], np.int64)
    rows = view_off[t["view"][off[k]:off[k + 1]].astype(np.int64)] + t["feat"][off[k]:off[k + 1]]
    assert len(set((np.searchsorted(touched_rows("rows65536"), rows) // 1024).tolist())) >= 32
    assert t["counts"][1] == 40 and t["counts"][0] == 2540
    # labels on both sides of 2^24, at least ten conflicts among 1 500 components
    t = twin("four_pass")
    assert (t["label"] < 2 ** 24).any() and (t["label"] >= 2 ** 24).any()
    assert t["counts"][1] >= 10 and t["counts"][0] + t["counts"][1] == 1500 and t["counts"][2] == 0
    t = twin("low_byte_zero")
    assert t["counts"][0] == 256 and t["counts"][1] == 7 and (t["label"] % 256 == 0).all()
    assert (touched_rows("low_byte_zero")[:256] == np.arange(256) * 256).all()     # view 0: every component's label
    assert twin("zigzag")["counts"] == [51, 1, 0, 50]
    # nothing kept: the scans over the kept flags and sizes are multi-block and all zero
    t = twin("all_conflict")
    assert t["counts"][0] == t["counts"][1] == 2500 and len(t["view"]) == 0
    t = twin("all_short")
    assert t["counts"][0] == 2540 and t["counts"][2] == 2500 and t["counts"][3] == 0 and CASES["all_short"][3] == 65
    use = CASES["masked"][2]
    assert use.tolist() == [int(v % 3 != 0) for v in range(64)]
    assert 0 < twin("masked")["counts"][3] and m["masked"] < m["rows65537plus"] and blocks(m["masked"]) >= 5
    assert not (set(twin("masked")["view"].tolist()) & set(range(0, 64, 3)))
