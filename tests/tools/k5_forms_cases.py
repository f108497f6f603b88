#!/usr/bin/env python3
"""The device side of tests/test_gpu_k5_forms.py: one launch-form group of K5 per process, because the knobs that force a
form (SFMLOC_P3P_SMALL, SFMLOC_P3P_WIDE_ALONE, SFMLOC_P3P_PREP_AHEAD) are read when the library first runs.  The cases
are tests/k5_cases.py's; the oracle's expectations come from the parent in an .npz (k5_cases.save_expectations).  Every
view of every handle is compared with them bit for bit (resect_compare.compare_view), then the group's condition on
sfmloc_debug_k5_round_counts is checked: a group that forces a form through a knob fails when the knob no longer
routes there.  Prints the cases run, the three counter values per step and a final OK.

usage: k5_forms_cases.py GROUP EXPECTATIONS.npz      (the parent sets the group's environment: GROUPS in the test)

  small           one handle, every case of at most 512 correspondences            plain = wide = 0, small > 0
  small_refuted   one handle per case of 513: the small rounds leave at once       small >= 1, plain >= 1, wide = 0
  plain_regs_lds  one handle, every case of at most 512                            small = wide = 0, plain > 0
  plain_large     one handle per case of 513 and more (a map has no wide credit
                  until its first large view is done)                              small = wide = 0, plain > 0
  wide            one handle, every case                                           small = plain = 0, wide > 0
  default         one handle, every case by ascending n; a second by descending n
                  on its own streams (the wide credit appears mid-session)         small + plain + wide > 0
  prepared_small  hypotheses prepared ahead, small rounds: one handle with every
                  case of at most 512, then one per case of 513 .. 1 025           as small, then as small_refuted
  prepared_full   hypotheses prepared ahead, no small rounds: one handle, every
                  case of at most 1 025                                            small = 0
"""
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import k5_cases as KC  # noqa: E402
from resect_compare import compare_view  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402


def upto(n):
    return [c for c in KC.CASES if c.n <= n]


def each(lo, hi):
    return [[c] for c in KC.CASES if lo <= c.n <= hi]


IS_SMALL = (lambda s, p, w: p == 0 and w == 0 and s > 0, "plain = wide = 0, small > 0")
IS_REFUTED = (lambda s, p, w: s >= 1 and p >= 1 and w == 0, "small >= 1, plain >= 1, wide = 0")
IS_PLAIN = (lambda s, p, w: s == 0 and w == 0 and p > 0, "small = wide = 0, plain > 0")
IS_WIDE = (lambda s, p, w: s == 0 and p == 0 and w > 0, "small = plain = 0, wide > 0")
BIGGEST = KC.SIZES[-1]

# group -> steps of (handles, whether they run on the alternative streams, (condition, its text)); a handle = a case list
GROUPS = {
    "small": [([upto(512)], False, IS_SMALL)],
    "small_refuted": [(each(513, 513), False, IS_REFUTED)],
    "plain_regs_lds": [([upto(512)], False, IS_PLAIN)],
    "plain_large": [(each(513, BIGGEST), False, IS_PLAIN)],
    "wide": [([upto(BIGGEST)], False, IS_WIDE)],
    "default": [([upto(BIGGEST)], False, (lambda s, p, w: s + p + w > 0, "small + plain + wide > 0")),
                ([KC.descending(KC.CASES)[0]], True, (lambda s, p, w: s + p + w > 0, "small + plain + wide > 0"))],
    "prepared_small": [([upto(512)], False, IS_SMALL), (each(513, 1025), False, IS_REFUTED)],
    "prepared_full": [([upto(1025)], False, (lambda s, p, w: s == 0 and p + w > 0, "small = 0"))],
}


def run_handle(cases, exp, ids):
    """-> [(case name, what differed)]"""
    h = S.Sfm(**KC.assemble(cases, ids))
    bad = []
    try:
        ran, ok = h.resect()
        res = h.resect_read()
        want = [exp[c.name] for c in cases]
        if (ran, ok) != (sum(e["ran"] for e in want), sum(e["ok"] for e in want)):
            bad.append(("(handle)", f"resected {ran}, succeeded {ok}"))
        for k, (c, r, e) in enumerate(zip(cases, res, want)):
            try:
                compare_view(h, k, r, e)
            except AssertionError as err:
                text = " ".join(str(err).split())
                bad.append((c.name, text[:200]))
    finally:
        h.close()
    return bad


def main():
    group, path = sys.argv[1], sys.argv[2]
    sets = KC.load_expectations(path)
    failed = False
    for step, (handles, alt, (cond, cond_text)) in enumerate(GROUPS[group]):
        exp = sets["alt" if alt else "own"]
        S.k5_round_counts(reset=True)
        t0 = time.time()
        bad, n_views = [], 0
        for cases in handles:
            bad += run_handle(cases, exp, KC.descending(KC.CASES)[1] if alt else None)
            n_views += len(cases)
        counts = S.k5_round_counts()
        print(f"{group} step {step}: {len(handles)} handle(s), {n_views} views, {time.time() - t0:.2f} s: "
              + " ".join(c.name for cases in handles for c in cases))
        print(f"{group} step {step}: rounds small {counts[0]} plain {counts[1]} wide {counts[2]} (must show: {cond_text})")
        for name, text in bad:
            print(f"MISMATCH {name}: {text}")
        if not cond(*counts):
            print(f"COUNTER: {counts} is not {cond_text}")
        failed = failed or bool(bad) or not cond(*counts)
    if failed:
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
