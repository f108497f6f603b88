"""GPU: the matrix-core form of the view-list scan (k_hamming_screen_mfma, hamming.hip; params.k1_mfma) -- its match
lists equal the CPU oracle's AND the popcount form's (k1_mfma = 0) on the same inputs; the cases are in
tests/tools/k1_mfma_cases.py, run here in child processes because the launch-shape knobs that route small test scans
down the shortlist branch (SFMLOC_K1_SCREEN_BATCH=1, SFMLOC_K1_QSPLIT=1) are read when the library first scans.

  sizes       query sizes 768 (the smallest screened), 769, 1 000, 2 000, 2 047, 2 049, 5 000 x ratios 0.3 / 0.6 / 0.95 /
              1.5 on uniform descriptors with planted near-duplicates, exact ties between query rows, bank rows equal to
              a query row (distance 0), all-ones against all-zeros rows (distance 512); the flagged set covers every
              accepted row and, at every ratio, is at most 2 x the popcount form's on the same input
  structured  sparse and M-LDB-like descriptors (synthdata.mldb_like_bank) at the four ratios
  views       long unaligned views, view lists that share bank blocks (flagged rows within 2 x here too), a
              device-built list padded with kNoBlock
  gang        gang sessions of 2 and of 32 members = single flight, fingerprint for fingerprint
  whole_path  begin_bow .. end with the form on and off: result_fingerprint equal for 64 queries on a map shaped like
              the headline's at reduced size
  (gang and whole_path read the map's statistics to make sure the intended form ran)
"""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("group", ["sizes", "structured", "views", "gang", "whole_path"])
def test_matrix_core_scan(oracle_c, group):
    env = dict(os.environ, SFMLOC_K1_SCREEN_BATCH="1", SFMLOC_K1_QSPLIT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "k1_mfma_cases.py"), group], env=env,
                       capture_output=True, text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.rstrip().endswith("OK")
