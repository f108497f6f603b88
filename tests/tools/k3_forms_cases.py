#!/usr/bin/env python3
"""The device side of tests/test_gpu_k3_forms.py: one launch-form group of K3 per process, because the knobs that force a
form (SFMLOC_K3_WIDE, _WIDE_2048, _WIDE_WAVES, _BIG, _WAVES_ALONE, _WAVES_SHARED) are read when the library first runs.
The scenes are tests/k3_cases.py's; the oracle's expectations come from the parent in an .npz
(k3_cases.save_expectations).  Every group runs every content at every size -- a form's duty includes leaving alone what
is not its own: each scene goes through sfmloc_geometric_pairs once whole (one call, n_sel = every pair) and, at budget
25, once more by the range of list lengths a form owns -- up to 512, 513 .. 1 024, 1 025 .. 2 048, beyond -- with
sfmloc_debug_k3_list_counts read and reset around each call.  Which pairs survive and every surviving pair's match list
in AC-RANSAC's inlier order equal the oracle's exactly; `clean` at budget 25 also runs with guided matching.  The
counters (inlier lists taken inside the register forms) show which form ran: a group fails when its knob stops routing.
Prints the calls, their times and counters, and a final OK.

usage: k3_forms_cases.py GROUP EXPECTATIONS.npz [COUNTS.json]  (the parent sets the group's environment: GROUPS in the test)

  group                 register form's lists > 0 in the ranges      == 0 in the ranges
  plain16/plain8/plain4 up to 512                                    513 .. 1 024, 1 025 .. 2 048, beyond
  plain_ref             as plain16, on the wave count the plan picks; writes its lists per content and range to COUNTS.json
  plain_big             up to 512, 513 .. 1 024                      1 025 .. 2 048, beyond
                        and up to 512 exactly as many as plain_ref's COUNTS.json: the instance behind the plain launch
                        (fast_min = 512) takes no list the plain launch has taken -- a list taken twice gives the same
                        bits, only the count shows it
  wide4 / wide8         up to 512, 513 .. 1 024                      1 025 .. 2 048, beyond
  wide_huge             up to 512, 513 .. 1 024, 1 025 .. 2 048      beyond
  default               up to 512                                    beyond
(> 0 is asked of the contents whose pairs survive: a list is taken only when a model is accepted.)
`default` and `wide4` also run the further cases: 256 and 257 pairs in one call, ten lists of 2 049 for the eight slots
of k_fmatrix_large, the second image's row 65 534, reuse of the map's context across ranges and across a localised
query, a pair named twice, empty and 7-match lists."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for p in (ROOT, TESTS):
    if p not in sys.path:
        sys.path.insert(0, p)
import k3_cases as KC  # noqa: E402
import sfmlocalization_amd as S  # noqa: E402
from sfmlocalization_amd import capi  # noqa: E402

REGISTER = {"plain_ref": ("le512",), "plain16": ("le512",), "plain8": ("le512",), "plain4": ("le512",),
            "plain_big": ("le512", "le1024"), "wide4": ("le512", "le1024"), "wide8": ("le512", "le1024"),
            "wide_huge": ("le512", "le1024", "le2048"), "default": ("le512",)}
BLOCK_WIDE = {g: tuple(r for r in ("le1024", "le2048", "large") if r not in own) for g, own in REGISTER.items()}
BLOCK_WIDE["default"] = ("large",)
SURVIVING = ("clean", "outliers30", "outliers85", "ties", "shuffled", "collinear")
FURTHER = ("default", "wide4")
failures = []
totals = {}              # content -> range -> lists taken in a register form


def open_map(sc, budget, guided=0):
    p = S.default_params(ransac_round=budget, geom_precision=KC.GEOM_PRECISION, guided_matching=guided)
    return S.Map(sc.view_id, sc.view_off, sc.desc, params=p, view_wh=sc.view_wh, kpt_xy=sc.kpt)


def differences(got, exp, sizes):
    """-> text of what differs between two {(a, b): (i[], j[])} (empty: nothing)"""
    bad = []
    if sorted(got) != sorted(exp):
        bad.append(f"survivors {[sizes.get(k, k) for k in sorted(got)]} != {[sizes.get(k, k) for k in sorted(exp)]}")
    for k in sorted(set(got) & set(exp)):
        for side in (0, 1):
            g, e = np.asarray(got[k][side]), np.asarray(exp[k][side])
            if g.shape != e.shape or not np.array_equal(g, e):
                n = min(len(g), len(e))
                at = np.nonzero(g[:n] != e[:n])[0]
                bad.append(f"pair of {sizes.get(k, k)} matches: {'ij'[side]} differs ({len(g)} vs {len(e)} entries, first at "
                           f"{int(at[0]) if len(at) else n})")
                break
    return bad


def check(label, got, exp, sizes):
    bad = differences(got, exp, sizes)
    for b in bad:
        print(f"MISMATCH {label}: {b}")
        failures.append(f"{label}: {b}")
    return not bad


def sub(exp, keys):
    return {k: v for k, v in exp.items() if k in keys}


def run_scene(group, content, budget, sets):
    sc = KC.scene(content, budget)
    N = len(sc.sizes)
    sizes = {(k, N): m for k, m in enumerate(sc.sizes)}
    exp = sets[f"{content}_{budget}"]
    t0 = time.time()
    with open_map(sc, budget) as dm:
        check(f"{content}/{budget} whole", dm.geometric_pairs(sc.matches), exp, sizes)
        line = []
        if budget == 25:
            for name, lo, hi, part in KC.ranges(sc):
                capi.k3_list_counts(reset=True)
                got = dm.geometric_pairs(part)
                counts = capi.k3_list_counts(reset=True)
                check(f"{content}/{budget} {name}", got, sub(exp, part), sizes)
                line.append(f"{name} {counts[0]}+{counts[1]}")
                total = counts[0] + counts[1]
                totals.setdefault(content, {})[name] = total
                if name in REGISTER[group] and content in SURVIVING and total == 0:
                    failures.append(f"COUNTER {content} {name}: no list taken in a register form")
                if name in BLOCK_WIDE[group] and total != 0:
                    failures.append(f"COUNTER {content} {name}: {counts} lists taken in a register form, the block-wide filter "
                                    f"owns the range")
    text = f"{group} {content}/{budget}: {N} pairs, {time.time() - t0:.2f} s"
    if line:
        text += "; register-form lists (copied+rebuilt) " + ", ".join(line)
    print(text)
    if content == "clean" and budget == 25:
        t0 = time.time()
        with open_map(sc, budget, guided=1) as dm:
            got = dm.geometric_pairs(sc.matches)
        check("clean/25 guided", got, sets["clean_25_gm"], sizes)
        print(f"{group} clean/25 guided: {len(got)} pairs, {sum(len(v[0]) for v in got.values())} guided matches, "
              f"{time.time() - t0:.2f} s")


def pairs_raw(dm, pairs, lists):
    """sfmloc_geometric_pairs on a pair list as given (capi.Map.geometric_pairs takes a dict: no pair twice)"""
    arr = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    off = np.zeros(len(arr) + 1, np.uint64)
    off[1:] = np.cumsum([len(v[0]) for v in lists])
    mi = np.ascontiguousarray(np.concatenate([np.asarray(v[0], np.uint32) for v in lists]), np.uint32)
    mj = np.ascontiguousarray(np.concatenate([np.asarray(v[1], np.uint32) for v in lists]), np.uint32)
    h = C.c_void_p()
    capi._check(capi._L().sfmloc_geometric_pairs(dm._h, capi._ptr(arr, C.c_uint32), len(arr), capi._ptr(off, C.c_uint64),
                                                 capi._ptr(mi, C.c_uint32), capi._ptr(mj, C.c_uint32), C.byref(h)))
    return dm._take_matches(h)


def same_bytes(label, a, b):
    ok = list(a) == list(b) and all(a[k][s].tobytes() == b[k][s].tobytes() for k in a for s in (0, 1))
    if not ok:
        print(f"MISMATCH {label}")
        failures.append(label)


def further(group, sets):
    t0 = time.time()
    for name, sc in (("many_256", KC.many_pairs(256)), ("many_257", KC.many_pairs(257)), ("large10", KC.large_views()),
                     ("row65534", KC.last_query_row())):
        sizes = {k: len(v[0]) for k, v in sc.matches.items()}
        capi.k3_list_counts(reset=True)
        with open_map(sc, 25) as dm:
            got = dm.geometric_pairs(sc.matches)
        counts = capi.k3_list_counts(reset=True)
        check(name, got, sets[name], sizes)
        print(f"{group} {name}: {len(sc.matches)} pairs, {len(got)} survive, register-form lists {counts[0]}+{counts[1]}")
        if name == "large10" and sum(counts):
            failures.append(f"COUNTER large10: {counts}")
        if name.startswith("many") and not sum(counts):
            failures.append(f"COUNTER {name}: no list taken in a register form")
    # reuse of the map's one context: the ranges in another order, then a pair twice, then lists that do not run
    sc = KC.scene("clean", 25)
    N = len(sc.sizes)
    sizes = {(k, N): m for k, m in enumerate(sc.sizes)}
    exp = sets["clean_25"]
    parts = {name: part for name, lo, hi, part in KC.ranges(sc)}
    with open_map(sc, 25) as dm:
        first = dm.geometric_pairs(parts["le2048"])
        small = dm.geometric_pairs(parts["le512"])
        third = dm.geometric_pairs(parts["le2048"])
        check("reuse le2048", first, sub(exp, parts["le2048"]), sizes)
        check("reuse le512", small, sub(exp, parts["le512"]), sizes)
        same_bytes("reuse: le2048 after le512 differs from le2048 before it", first, third)
        k18, k64 = sc.sizes.index(18), sc.sizes.index(64)
        a, b = sc.matches[(k18, N)], sc.matches[(k64, N)]
        short = (a[0][:8], a[1][:8])            # the pair of 18 named twice: first with 8 of its matches, then with all
        got = pairs_raw(dm, [(k18, N), (k64, N), (k18, N)], [short, b, a])
        check("a pair twice keeps its last list", got, sub(exp, {(k18, N), (k64, N)}), sizes)
        got = pairs_raw(dm, [(k18, N), (k18, N)], [a, short])
        check("a pair twice keeps its last list (the short one: dropped)", got, {}, sizes)
        k7, k8 = sc.sizes.index(7), sc.sizes.index(8)
        none = np.zeros(0, np.uint32)
        got = dm.geometric_pairs({(k8, N): (none, none), (k7, N): sc.matches[(k7, N)], (k18, N): (a[0][:7], a[1][:7])})
        check("empty and 7-match lists", got, {}, sizes)
        check("after them", dm.geometric_pairs(parts["le512"]), sub(exp, parts["le512"]), sizes)
    # a localised query between two pair calls on one map
    import synthdata as synth
    m = synth.make_map(43, n_views=8, desc_per_view=260, views_per_place=8, landmarks_per_place=220, obs_per_view=150,
                       map_flips=6)
    q = synth.make_query(m, 44, n_feat=300, n_copies=120)
    p = S.default_params(ransac_round=25, geom_precision=KC.GEOM_PRECISION)
    with S.Map(m.view_id, m.view_off, m.desc, params=p, view_wh=m.view_wh, kpt_xy=m.kpt_xy, row_landmark=m.row_landmark,
               landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic) as dm:
        put = {k: v for k, v in dm.track(3).items() if len(v[0]) >= 20}
        before = dm.geometric_pairs(put)
        dq = dm.query(q.desc, q.kpt_xy, q.width, q.height)
        pose, _, _ = dm.localize(dq)
        dq.close()
        after = dm.geometric_pairs(put)
    off = m.view_off.astype(np.int64)
    from oracle import pipeline as opipe
    want = opipe.geometric_match([m.kpt_xy[off[v]:off[v + 1]] for v in range(8)], m.view_wh, m.view_id, put, ransac_round=25)
    sz = {k: len(v[0]) for k, v in put.items()}
    check("pairs before a query", before, want, sz)
    same_bytes("a localised query in between changes the next pair call", before, after)
    print(f"{group} further: {len(put)} tracked pairs, {len(want)} survive, query localised: {bool(pose.ok)}; "
          f"{time.time() - t0:.2f} s")
    if len(want) < 4:
        failures.append("the tracked scene has fewer than 4 surviving pairs")


def main():
    group, path = sys.argv[1], sys.argv[2]
    sets = KC.load_expectations(path)
    t0 = time.time()
    for content, budget in KC.all_scenes():
        run_scene(group, content, budget, sets)
    if group in FURTHER:
        further(group, sets)
    if group == "plain_ref":
        with open(sys.argv[3], "w") as f:
            json.dump(totals, f)
    if group == "plain_big":
        with open(sys.argv[3]) as f:
            ref = json.load(f)
        for content, t in totals.items():
            if t["le512"] != ref[content]["le512"]:
                failures.append(f"COUNTER {content} le512: {t['le512']} lists taken, {ref[content]['le512']} without the "
                                f"1 024-match instance: it took lists of the plain launch's range")
    print(f"{group}: {time.time() - t0:.2f} s in all")
    for f in failures:
        print("FAILED", f)
    if failures:
        return 1
    print("OK")
    return 0


if __name__ == "__main__":
    sys.exit(main())
