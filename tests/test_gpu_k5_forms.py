"""GPU: K5 (k_p3p_round, k_p3p_round_small, k_p3p_finish) through every launch form and every evaluator its table names
("K5: which evaluator a round runs"), at the correspondence counts where the evaluators change -- 256 / 257,
512 / 513, 1 024 / 1 025, 2 048 / 2 049, 4 096 / 4 097 and the rest of k5_cases.SIZES -- on contents with exact ties,
one-ulp near-ties, all-zero residuals, late and missing models and degenerate samples (tests/k5_cases.py; what each
content guarantees is checked on the CPU by test_k5_cases_cpu.py).  sfmloc_sfm_resect copies a view's observation list
straight into K5's buffers, so a view has exactly the n its case names.

Every view's ran, ok, n_obs, n_inliers, iterations, error_max, nfa, P, R, centre and its inlier list in order equal the
C oracle's bit for bit (resect_compare.compare_view), and sfmloc_debug_k5_round_counts shows that the form the group
forces is the form that ran.  The cases run in tests/tools/k5_forms_cases.py (its docstring has the group table), one
child process per group: the forcing knobs are read when the library first runs.  The oracle's expectations are computed
once per session here and handed over in an .npz."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import k5_cases as KC  # noqa: E402

# group -> the children it runs: (k5_forms_cases.py group, the knobs set for it; every other form knob is unset)
GROUPS = {
    "small": [("small", dict(SFMLOC_P3P_SMALL="2"))],
    "small_refuted": [("small_refuted", dict(SFMLOC_P3P_SMALL="2"))],
    "plain_regs_lds": [("plain_regs_lds", dict(SFMLOC_P3P_SMALL="0"))],
    "plain_large": [("plain_large", dict(SFMLOC_P3P_SMALL="0"))],
    "wide": [("wide", dict(SFMLOC_P3P_WIDE_ALONE="2"))],
    "default": [("default", {})],
    "prepared": [("prepared_small", dict(SFMLOC_P3P_PREP_AHEAD="2", SFMLOC_P3P_SMALL="2")),
                 ("prepared_full", dict(SFMLOC_P3P_PREP_AHEAD="2", SFMLOC_P3P_SMALL="0"))],
}


@pytest.fixture(scope="session")
def k5_expectations(oracle_c, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("k5_forms") / "expectations.npz")
    KC.save_expectations(path, {"own": KC.expectations(oracle_c), "alt": KC.expectations(oracle_c, alt=True)})
    return path


@pytest.mark.parametrize("group", list(GROUPS))
def test_k5_forms(k5_expectations, group):
    for child, knobs in GROUPS[group]:
        env = {k: v for k, v in os.environ.items() if not k.startswith(("SFMLOC_P3P_", "SFMLOC_K1_", "SFMLOC_K3_"))}
        env.update(knobs)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "tools", "k5_forms_cases.py"), child,
                            k5_expectations], env=env, capture_output=True, text=True, timeout=300)
        print(r.stdout[-12000:])
        assert r.returncode == 0, r.stdout[-6000:] + r.stderr[-3000:]
        assert r.stdout.rstrip().endswith("OK")
