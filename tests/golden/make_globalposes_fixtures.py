"""Writes tests/golden/globalposes/expected.json, tests/golden/globalposes/scene_large.npz and the "twin" sections of
profiles/globalposes_parity.json from the NumPy restatement (tests/globalposes_np.py) on the planted scenes of
tests/globalposes_scene.py.  No device.  Run from the repository root: python tests/golden/make_globalposes_fixtures.py

expected.json, per scene: the restatement's own errors against the planted truth (largest rotation error in degrees in
the root's gauge; largest centre error after the one similarity the gauge allows, as a fraction of the extent), its
integer results, and the two-solver distances below.  How each bound was measured:
    rotation_deg, centre    the restatement run with solver="pcg" on the scene; nothing is added to the figure.
    parity                  the restatement run twice, solver="pcg" (the header's rule) and solver="dense"
                            (numpy.linalg.solve), and per quantity the largest distance between the two: R (entries),
                            C (norm per view, over the largest planted |C - mean|), rot_residual and trans_residual (per
                            pair), cost (the five costs of the report, relative).  Each scene has its own figures; the
                            device tests hold the device on a scene within bound(): four times that scene's figure.
                            On the scenes of a few views conjugate gradients end exactly within their few unknowns and
                            the figure is itself a rounding figure, so bound() does not go below four times FLOOR =
                            16 eps (3.6e-15; every quantity is relative or of magnitude 1 at most).  The floor is a
                            count by reasoning, not a measurement: the device adds a view's pair terms and a
                            workgroup's partials in another order than NumPy (a few roundings per sum of a few terms)
                            and projects with a fixed-sweep Jacobi where NumPy uses eigh (a few more), each of eps / 2.
    chain                   the end-to-end scene of globalposes_scene.scene_files through the restatements of both stages
                            on the CPU (tests/relpose_np.py, whose bits the device's relative poses are, then
                            globalposes_np): the errors of the poses that chain ends with, before any triangulation or
                            adjustment, and the same two-solver distances ("parity") for that scene.
scene_large.npz keeps the restatement's outputs on scene (c), which take it half a minute: the device tests read them."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(HERE))

import globalposes_np as tw  # noqa: E402
import globalposes_scene as sc  # noqa: E402

OUT = os.path.join(HERE, "globalposes")
PARITY = os.path.join(ROOT, "profiles", "globalposes_parity.json")
SCENES = {"triplet": sc.scene_triplet, "ring": sc.scene_ring, "large": sc.scene_large}
FLOOR = 16.0 * float(np.finfo(np.float64).eps)
COSTS = ("chordal_cost", "rot_cost_initial", "rot_cost_final", "trans_cost_initial", "trans_cost_final")
KEEP = ("in_component", "root", "R", "C", "n_triplets", "n_triplets_ok", "kept", "used_t", "rot_residual",
        "trans_residual") + COSTS


def run(s, solver):
    return tw.global_poses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"], solver=solver)


def distances(s, a, b):
    """per quantity the distance between two results on scene s (what "parity" above lists)"""
    Ct = s["C_true"][a["in_component"]]
    extent = float(np.max(np.linalg.norm(Ct - Ct.mean(0), axis=1)))
    return {"R": float(np.max(np.abs(a["R"] - b["R"]))),
            "C": float(np.max(np.linalg.norm(a["C"] - b["C"], axis=1))) / extent,
            "rot_residual": float(np.max(np.abs(a["rot_residual"] - b["rot_residual"]))),
            "trans_residual": float(np.max(np.abs(a["trans_residual"] - b["trans_residual"]))),
            "cost": max(abs(float(a[k]) - float(b[k])) / abs(float(b[k])) for k in COSTS)}


def bound(twin):
    """the device's bound per quantity from a scene's two-solver distances (see the module's text)"""
    return {q: 4.0 * max(float(v), FLOOR) for q, v in twin.items()}


def chain():
    """-> the "chain" figures above"""
    import relpose_np as rp
    s = sc.scene_files()
    res = [r for r in zip(sc.relpose_call(s)["pairs"].tolist(), rp.relative_poses(**sc.relpose_call(s))) if int(r[1]["ok"])]
    pairs = np.array([p for p, _ in res], np.uint32)
    use = np.array([int(r["front"][int(r["choice"])]) == int(r["n_inliers"]) for _, r in res], np.uint8)
    args = (len(s["feats"]), pairs, np.array([r["R"] for _, r in res]).reshape(-1, 3, 3),
            np.array([r["t"] for _, r in res]).reshape(-1, 3), use)
    o, dense = tw.global_poses(*args), tw.global_poses(*args, solver="dense")
    rot, cen = sc.errors(s, o["in_component"], o["root"], o["R"], o["C"])
    return {"rotation_deg": rot, "centre": cen, "parity": distances(s, o, dense), "n_component_views": o["n_component_views"], "n_pairs": len(pairs),
            "n_translation_pairs": o["n_translation_pairs"]}


def main():
    os.makedirs(OUT, exist_ok=True)
    expected, parity = {}, {}
    expected["chain"] = chain()
    print("chain", expected["chain"])
    for name, make in SCENES.items():
        s = make()
        a, b = run(s, "pcg"), run(s, "dense")
        rot, cen = sc.errors(s, a["in_component"], a["root"], a["R"], a["C"])
        parity[name] = distances(s, a, b)
        expected[name] = {"rotation_deg": rot, "centre": cen, "n_component_views": a["n_component_views"],
                          "root": a["root"], "n_pairs_kept": a["n_pairs_kept"], "n_triplets": a["n_triplets_total"],
                          "n_triplets_ok": a["n_triplets_ok_total"], "parity": parity[name],
                          "steps": [a["rot_steps_tried"], a["trans_steps_tried"]]}
        if name == "large":
            np.savez_compressed(os.path.join(OUT, "scene_large.npz"), **{k: np.asarray(a[k]) for k in KEEP})
        print(name, expected[name])
    with open(os.path.join(OUT, "expected.json"), "w") as fh:
        json.dump(expected, fh, indent=1, sort_keys=True)
        fh.write("\n")
    try:
        with open(PARITY) as fh:
            doc = json.load(fh)
    except (OSError, ValueError):
        doc = {}
    doc.update({"twin_" + n: parity[n] for n in parity})
    doc.pop("bound", None)
    doc["floor"] = FLOOR
    doc["note"] = ("twin_*: the distance between the restatement's two solvers (pcg, dense) per scene and quantity; "
                   "device_*: the distance of the device from the restatement (pcg) on that scene, recorded by "
                   "tests/test_gpu_globalposes.py, to be at most 4 x max(twin, floor)")
    with open(PARITY, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
