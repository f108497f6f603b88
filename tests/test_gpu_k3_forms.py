"""GPU: K3 (k_fmatrix_fast<W, 512|1024|2048[, wide]>, k_fmatrix_filter, k_fmatrix_large) through every launch form
plan_k3 chooses among ("K3: which form takes a list"), on explicit putative lists handed to
sfmloc_geometric_pairs, at the list lengths where the residuals per lane, the instance or the kernel change -- 64 / 65,
128 / 129, 256 / 257, 512 / 513, 1 024 / 1 025, 2 048 / 2 049 and the rest of k3_cases.SIZES, down to the 7 that do not
run, the 8 that do and the 17 | 18 of the "> 2.5 * 7 inliers" rule -- on clean lists, 30 / 85 / 100 % outliers, bit-equal
keypoints (tied residuals), shuffled indices and rank-deficient samples (tests/k3_cases.py; what each content guarantees
is checked on the CPU by test_k3_cases_cpu.py).

Every group runs every content at every size: which pairs survive and each survivor's match list in AC-RANSAC's inlier
order equal oracle.pipeline.geometric_match's exactly, and sfmloc_debug_k3_list_counts shows per range of list lengths
that the form the group forces is the form that ran.  The cases run in tests/tools/k3_forms_cases.py (its docstring has
the table of counter conditions and the further cases), one child process per group: the forcing knobs are read when
the library first runs.  The oracle's expectations are computed once per session here and handed over in an .npz."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import k3_cases as KC  # noqa: E402

PLAIN = dict(SFMLOC_K3_WIDE="0", SFMLOC_K3_BIG="0")
# group -> the children it runs: (k3_forms_cases.py group, the knobs set for it; every other form knob is unset).
# plain_big's first child is the same plain launch without the 1 024-match instance: its list counts are the second's
# reference for the range the instance must leave alone
GROUPS = {
    "plain16": [("plain16", dict(PLAIN, SFMLOC_K3_WAVES_ALONE="16", SFMLOC_K3_WAVES_SHARED="16"))],
    "plain8": [("plain8", dict(PLAIN, SFMLOC_K3_WAVES_ALONE="8", SFMLOC_K3_WAVES_SHARED="8"))],
    "plain4": [("plain4", dict(PLAIN, SFMLOC_K3_WAVES_ALONE="4", SFMLOC_K3_WAVES_SHARED="4"))],
    "plain_big": [("plain_ref", PLAIN), ("plain_big", dict(SFMLOC_K3_WIDE="0", SFMLOC_K3_BIG="2"))],
    "wide4": [("wide4", dict(SFMLOC_K3_WIDE="2", SFMLOC_K3_WIDE_2048="0", SFMLOC_K3_WIDE_WAVES="4"))],
    "wide8": [("wide8", dict(SFMLOC_K3_WIDE="2", SFMLOC_K3_WIDE_2048="0", SFMLOC_K3_WIDE_WAVES="8"))],
    "wide_huge": [("wide_huge", dict(SFMLOC_K3_WIDE="2", SFMLOC_K3_WIDE_2048="2"))],
    "default": [("default", {})],
}


@pytest.fixture(scope="session")
def k3_expectations(oracle_c, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("k3_forms") / "expectations.npz")
    sets = {f"{c}_{b}": KC.expectations(oracle_c, c, b) for c, b in KC.all_scenes()}
    sets["clean_25_gm"] = KC.expectations(oracle_c, "clean", 25, guided=True)
    for name, sc in (("many_256", KC.many_pairs(256)), ("many_257", KC.many_pairs(257)), ("large10", KC.large_views()),
                     ("row65534", KC.last_query_row())):
        sets[name] = KC.expect_scene(sc)
    # the further cases are what they are for: every pair of 20 clean matches survives whole, all ten large lists
    # survive, and the list that names the second image's last row keeps it
    assert all(len(sets[n]) == int(n[5:]) and all(len(v[0]) == 20 for v in sets[n].values()) for n in ("many_256", "many_257"))
    assert len(sets["large10"]) == 10
    assert 65534 in next(iter(sets["row65534"].values()))[1]
    KC.save_expectations(path, sets)
    return path


@pytest.mark.parametrize("group", list(GROUPS))
def test_k3_forms(k3_expectations, group, tmp_path):
    counts = str(tmp_path / "counts.json")
    for child, knobs in GROUPS[group]:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("SFMLOC_P3P_", "SFMLOC_K1_", "SFMLOC_K3_"))}
        env.update(knobs)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "k3_forms_cases.py"), child,
                            k3_expectations, counts], env=env, capture_output=True, text=True, timeout=300)
        print(r.stdout[-12000:])
        assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
        assert r.stdout.rstrip().endswith("OK")
