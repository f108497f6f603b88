"""Writes tests/golden/pairscales_parity.json: what the two solvers of tests/pairscales_np.global_poses_scaled leave
between them on the scenes of tests/pairscales_scene.py (the largest difference of a baseline and of a centre
coordinate), which times four is the bound of the device tests, as profiles/globalposes_parity.json is for the unscaled
call; and the restatement's own figures on the corridor: the centre errors of both calls and the largest relative error
of a baseline other than the planted wrong pair's.  CPU only:  python tests/golden/make_pairscales_fixtures.py"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import globalposes_np as gp  # noqa: E402
import globalposes_scene as gs  # noqa: E402
import pairscales_np as tw  # noqa: E402
import pairscales_scene as sc  # noqa: E402

MAKERS = dict(triplet=sc.scene_triplet, corridor=sc.scene_corridor, boundaries=sc.scene_boundaries)
INTS = ("n_component_views", "root", "n_translation_pairs", "scale_n_wedges_used", "scale_n_scaled_pairs",
        "scale_n_scaled_views", "scale_first_pair", "scale_steps_tried", "scale_steps_accepted", "scale_stop",
        "trans_steps_tried", "trans_steps_accepted", "trans_stop")


def wedges_of(ref):
    rec = ref["records"]
    return (np.array([[r[1], r[2]] for r in rec], np.uint32).reshape(-1, 2), np.array([r[4] for r in rec], np.float64))


def wedges_for(name, s, ref):
    """the wedges of the scaled call on a scene: the measured records; on the boundary scene also a planted star, the
    hub's first pair with every other pair of the hub at the ratio of the planted baselines (the hub's pairs share few
    features with one another, so the measured wedges give no node of more than 64: the star's centre is one, and the
    wave gathers it).  Every eighth ratio of the star is off by half, so that the scale averaging has weights to
    iterate on and ends by its tolerance, not by a last step at rounding level whose acceptance either solver may see
    differently"""
    kl, ratio = wedges_of(ref)
    if name != "boundaries":
        return kl, ratio
    have = set(map(tuple, kl.tolist()))
    hub = [k for k, p in enumerate(s["pairs"].tolist()) if s["hub"] in p]
    star = [(hub[0], l) for l in hub[1:] if (hub[0], l) not in have]
    return (np.concatenate([kl, np.array(star, np.uint32)]),
            np.concatenate([ratio, [s["b_true"][l] / s["b_true"][k] * (1.5 if q % 8 == 3 else 1.0) for q, (k, l) in enumerate(star)]]))


def main():
    out = {}
    for name, make in MAKERS.items():
        s = make()
        kl, ratio = wedges_for(name, s, tw.wedge_scales(**s["call"]))
        n = len(s["R_true"])
        a, b = (tw.global_poses_scaled(n, s["pairs"], s["rel_R"], s["rel_t"], kl, ratio, solver=v) for v in ("pcg", "dense"))
        assert all(a[k] == b[k] for k in INTS), name
        e = dict(twin_baseline=float(np.max(np.abs(a["baselines"] - b["baselines"]))),
                 twin_centre=float(np.max(np.abs(a["C"] - b["C"]))), **{k: int(a[k]) for k in INTS})
        if name == "corridor":
            u = gp.global_poses(n, s["pairs"], s["rel_R"], s["rel_t"])
            bt = s["b_true"] / tw.lower_median(s["b_true"])
            rel = np.abs(a["baselines"] / bt - 1.0)
            e.update(centre_error_scaled=gs.errors(s, a["in_component"], u["root"], a["R"], a["C"])[1],
                     centre_error_unscaled=gs.errors(s, u["in_component"], u["root"], u["R"], u["C"])[1],
                     wrong_pair_baseline_error=float(rel[s["wrong_pair"]]),
                     other_baseline_error=float(np.max(np.delete(rel, s["wrong_pair"]))))
        out[name] = e
    with open(os.path.join(HERE, "pairscales_parity.json"), "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
