"""GPU: the tail of a view in K3's wide form (fmatrix_fast.body.inc) -- what the workgroup that arrives last does alone
after the first batch: on four or on eight waves (k_fmatrix_fast<4 / 8, 1024, true>, SFMLOC_K3_WIDE_WAVES), a new best
model's sorted inlier list copied from the segment of the wave that evaluated it, or rebuilt by wave 0 when that wave has
evaluated another model since (and always after the first batch, which other workgroups evaluated).  Same samples, same
arithmetic, same replay: every case's pose bits, inlier pairs, n_putative_views and n_geometric_views are the oracle's
under the default, under SFMLOC_K3_WIDE_WAVES=4 and under =8.  The knob is read when the library first runs, so each
setting takes all the cases (tests/tools/k3_wide_tail_cases.py) in one child process.  No timing here."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

from oracle import pipeline as opipe

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOL = os.path.join(ROOT, "tests", "tools", "k3_wide_tail_cases.py")
_spec = importlib.util.spec_from_file_location("k3_wide_tail_cases", TOOL)
cases = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(cases)
bits = cases.shared.bits

SETTINGS = ("default", "4", "8")


@pytest.fixture(scope="module")
def runs(oracle_c):
    """(the oracle's record per case and query, the oracle's intermediates, {setting: the child's JSON})"""
    sc = cases.scenes(opipe.localize)
    want, exps = {}, {}
    for name, (scene, n, params, _) in cases.CASES.items():
        m, qs = sc[scene]
        exps[name] = [opipe.localize(m, q.desc, q.kpt_xy, (q.width, q.height), **params) for q in qs[:n]]
        min_put = params.get("min_putative", 16)
        want[name] = [{"ok": bool(e["ok"]), "P": [int(x) for x in bits(e["P"].ravel())] if e["ok"] else None,
                       "pq": [int(x) for x in e["pair_qfeat"]] if e["ok"] else None,
                       "pl": [int(x) for x in e["pair_landmark"]] if e["ok"] else None,
                       "n_put": int((e["put_count"] >= min_put).sum()), "n_geo": int((e["geo_count"] > 0).sum()),
                       "n_inl": int(e["n_inliers"]) if e["ok"] else 0} for e in exps[name]]
    children = {}
    for s in SETTINGS:                                        # started together, one GPU process each
        env = dict(os.environ)
        env.pop("SFMLOC_K3_WIDE_WAVES", None)
        if s != "default":
            env["SFMLOC_K3_WIDE_WAVES"] = s
        children[s] = subprocess.Popen([sys.executable, TOOL], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    got = {}
    for s, p in children.items():
        out, err = p.communicate(timeout=300)
        assert p.returncode == 0, (s, out[-2000:] + err[-2000:])
        got[s] = json.loads(out.strip().splitlines()[-1])
    return want, exps, got


def check(runs, name):
    want, _, got = runs
    for s in SETTINGS:
        assert len(got[s][name]) == len(want[name])
        for i, (g, w) in enumerate(zip(got[s][name], want[name])):
            what = f"{name}, query {i}, SFMLOC_K3_WIDE_WAVES {s}"
            assert g["ok"] == w["ok"] and g["n_put"] == w["n_put"] and g["n_geo"] == w["n_geo"], (what, g, w)
            if w["ok"]:
                assert g["n_inl"] == w["n_inl"] and g["pq"] == w["pq"] and g["pl"] == w["pl"] and g["P"] == w["P"], what
        assert got[s][name] == got["default"][name], f"{name}: SFMLOC_K3_WIDE_WAVES {s} against the default"


def test_default_budget(runs):
    """scene25 (40 views x 400 rows), 800-feature queries, ransac_round 25: a first batch of 23 iterations, one workgroup
    each, and a tail of reserve iterations by the last to arrive."""
    check(runs, "default_budget")
    _, exps, got = runs
    assert sum(e["ok"] for e in exps["default_budget"]) >= 3
    assert all((e["geo_count"] > 0).sum() >= 2 for e in exps["default_budget"])    # several views with a tail per query
    for s in SETTINGS:                                        # every surviving view fetched a list after its first batch
        assert sum(got[s]["list_counts"]["default_budget"]) >= sum(int((e["geo_count"] > 0).sum()) for e in exps["default_budget"])


@pytest.mark.parametrize("rounds", [3, 40, 200])
def test_ransac_round(runs, rounds):
    """3: two uniform iterations and a tail of at most one.  40: 36 uniform iterations > 32, so the tail begins while
    sampling is still uniform.  200: a reserve of 20 iterations -- several set changes per view, batches cut short by the
    end of the budget; the set changes served by copy AND by rebuild both occur, or the test could not tell the reuse from
    a permanent fall-back."""
    name = f"ransac_round_{rounds}"
    check(runs, name)
    _, exps, got = runs
    assert any((e["geo_count"] > 0).sum() > 0 for e in exps[name])
    if rounds == 200:
        for s in SETTINGS:
            copied, rebuilt = got[s]["list_counts"][name]
            print(f"SFMLOC_K3_WIDE_WAVES {s}: lists copied {copied}, rebuilt {rebuilt}")
            assert copied > 0 and rebuilt > 0, (s, copied, rebuilt)


def test_views_of_513_to_1024_matches(runs):
    """three views x 1 100 rows, queries that nearly duplicate a map frame: 16 residuals per lane in the register sort of
    an eight-wave workgroup"""
    check(runs, "views_513_to_1024")
    _, exps, _ = runs
    assert all(512 < int(e["put_count"].max()) <= 1024 for e in exps["views_513_to_1024"])
    assert all((e["geo_count"] > 0).sum() > 0 for e in exps["views_513_to_1024"])


def test_smallest_views(runs):
    """views of exactly min_putative = 16 matches, of 15 and of 10; and with min_putative = 8 the view of 10 is the
    kernel's own: a tail batch wants more samples than the set of a view that small can offer"""
    _, exps, _ = runs
    for name in ("min_putative_16", "min_putative_8"):
        assert list(exps[name][0]["put_count"][[33, 34, 37]]) == [15, 16, 10]
        check(runs, name)
    assert exps["min_putative_16"][0]["geo_count"][37] == 0 and exps["min_putative_16"][0]["geo_count"][33] == 0


def test_three_contexts_interleaved(runs):
    """six queries through three contexts with begin / end interleaved: several views' last arrivals at once, other
    queries' kernels beside them"""
    check(runs, "three_contexts")
    want, _, _ = runs
    assert want["three_contexts"][:4] == want["default_budget"]    # (the same queries alone: the same results)
