"""sfmloc_tracks_build on the pair lists of tests/tracks_cases.py against the NumPy restatement (structure_np.tracks, which
test_tracks_cases_cpu.py holds to a plain union-find): the multi-block scan of csrc/tracks.hip and the radix sort of
csrc/radix_sort.h with one to four passes, one to forty-odd blocks, scans past one chunk of k_scan_excl and a digit
bucket that holds a whole block.  Integers only: every comparison is exact."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import structure_np as tw  # noqa: E402
from tracks_cases import CASES, reversed_pair_list  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def twin():
    """name -> structure_np.tracks of the case, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            view_off, pl, use, min_length = CASES[name]
            cache[name] = tw.tracks(view_off, *pl, view_use=use, min_length=min_length)
        return cache[name]
    return get


def equal(got, want):
    assert got.counts == want["counts"]
    np.testing.assert_array_equal(got.off, want["off"])
    np.testing.assert_array_equal(got.view, want["view"])
    np.testing.assert_array_equal(got.feat, want["feat"])


@pytest.mark.parametrize("name", list(CASES))
def test_tracks_equal_the_twin(twin, name):
    view_off, pl, use, min_length = CASES[name]
    want = twin(name)
    for _ in range(2):                       # the same arrays twice
        equal(capi.Tracks(view_off, *pl, view_use=use, min_length=min_length), want)
    # the hooking races differ with the edge order; the result must not
    equal(capi.Tracks(view_off, *reversed_pair_list(*pl), view_use=use, min_length=min_length), want)
