"""GPU: what the typed transfers (csrc/devmem.h "Transfers") order by construction -- a context's setup clears and the
statistics reset run on the context's own stream, so a scan queued right behind either is ordered after it.  The shapes
are test_gpu_hamming.py::test_view_selection_and_query_split's: the eight-view selection is the smallest case of the
suite that takes the sliced scan with the flagged-row merge."""
import numpy as np
import pytest

import sfmlocalization_amd as S
import synthdata as synth

pytestmark = pytest.mark.gpu
SEL = np.array([1, 2, 5, 17, 18, 19, 33, 39], np.uint32)


@pytest.fixture(scope="module")
def scene():
    m = synth.make_map(5, n_views=40, desc_per_view=300, views_per_place=8, landmarks_per_place=200,
                       obs_per_view=80, ragged=True)
    q = synth.make_query(m, 9, n_feat=1200, n_copies=120)
    return m, q


def open_map(m):
    nv = len(m.view_off) - 1
    return S.Map(np.arange(nv, dtype=np.uint32) * 2 + 1, m.view_off, m.desc, params=S.default_params(dist_ratio=0.6))


def test_first_scan_of_a_fresh_map_equals_its_second(oracle_c, scene):
    m, q = scene
    with open_map(m) as dev:
        qq = dev.query(q.desc)
        dev.match_putative(qq, SEL)
        first = dev.putative_read()
        dev.match_putative(qq, SEL)
        second = dev.putative_read()
        qq.close()
    exp = oracle_c.match_to_query(q.desc, m.desc, m.view_off, SEL, 0.6, threads=4)
    assert exp[0].sum() > 0
    for name, a, b, e in zip(("view_count", "match_i", "match_j", "match_d"), first, second, exp):
        np.testing.assert_array_equal(a, b, err_msg="first vs second scan: " + name)
        np.testing.assert_array_equal(a, e, err_msg="first scan vs the oracle: " + name)


def test_scan_right_behind_a_statistics_reset_is_counted_whole(scene):
    """hamming_pairs: query features x bank rows scanned.  The scan's unit is the 64-row bank block, so the rows are
    those of the distinct blocks the selected views overlap, worked out here from view_off (a selection on block
    boundaries would make them the selected rows themselves).  hamming_rows_flagged and hamming_pairs_finished are
    counted on the device; a reset that ran late would take part of them away, so two repetitions agree (with a sync
    between reset and scan they are the same from run to run, on a fresh map too: this scan form counts 0 of either)."""
    m, q = scene
    off = np.asarray(m.view_off, np.int64)
    blocks = set()
    for v in SEL:
        if off[v + 1] > off[v]:
            blocks.update(range(int(off[v]) // 64, (int(off[v + 1]) - 1) // 64 + 1))
    pairs = len(q.desc) * 64 * len(blocks)
    assert pairs >= len(q.desc) * int((off[SEL + 1] - off[SEL]).sum()) > 0
    seen = []
    with open_map(m) as dev:
        qq = dev.query(q.desc)
        for _ in range(2):
            dev.stats_reset()
            dev.match_putative(qq, SEL)  # (no sync between the reset and the scan)
            st = dev.stats()
            print("hamming_pairs", st.hamming_pairs, "rows_flagged", st.hamming_rows_flagged, "pairs_finished",
                  st.hamming_pairs_finished)
            assert st.hamming_pairs == pairs
            seen.append((st.hamming_rows_flagged, st.hamming_pairs_finished))
        qq.close()
    assert seen[0] == seen[1]
