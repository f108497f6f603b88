#!/usr/bin/env python3
"""Build-container script (needs the reference tree, as make_ref_fixtures.py does; never runs on the GPU box): what
the reference's own map-merge functions (PyVisionLocalizeCommon/src/hulo_sfm/mergeSfM.py) return on the small documents of tests/merge_scene.py,
recorded as data under tests/golden/merge_ref/expected.json.  The module is Python 2 text: it is converted in memory
with lib2to3 (make_ref_fixtures.import_py2) and executed; nothing of it is written anywhere.  np.float is set to float
in this process because NumPy 2 removed the alias the module uses.

Recorded: getConsistent3DMatch, getInliersByAffineTransform, merge_sfm_data, transform_sfm_data, findMedianThres,
findMedianStructurePointsThres, ransacAffineTransform (five seeds of `random`, n x 100 rounds) and modelMergeCheckLocal.

    python tests/golden/make_merge_fixtures.py
"""
import contextlib
import copy
import io
import json
import os
import random
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "merge_ref")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_ref_fixtures as ref  # noqa: E402
import merge_scene as MS  # noqa: E402

KMED = 2.5
CHECK_THRES = 1.0


def main():
    if not hasattr(np, "float"):
        np.float = float
    ref.import_py2("hulo_file/FileUtils.py", "hulo_file.FileUtils", package_modules=("hulo_file",))
    m = ref.import_py2("hulo_sfm/mergeSfM.py", "hulo_sfm.mergeSfM", package_modules=("hulo_sfm",))
    scene = MS.make_docs()
    exp = {}
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        pa, pb, loc = MS.write_docs(scene, tmp)
        docA, docB = copy.deepcopy(scene["docA"]), copy.deepcopy(scene["docB"])
        names, pairs = m.readMatch(loc)
        view_id = m.imgnameToViewID(names, docB)
        match = m.getConsistent3DMatch(view_id, pairs, m.getViewFeatTo3DMap(docB))
        exp["viewID"] = view_id
        exp["getConsistent3DMatch"] = sorted([int(b), int(a)] for b, a in match)
        match = exp["getConsistent3DMatch"]
        A = np.asarray(m.get3DPointloc(docA, [x[1] for x in match]), dtype=float).T
        B = np.asarray(m.get3DPointloc(docB, [x[0] for x in match]), dtype=float).T
        M = scene["M"]
        inl = m.getInliersByAffineTransform(A, B, M, MS.THRES)
        exp["getInliersByAffineTransform"] = [int(i) for i in inl]
        exp["findMedianThres"] = {"A": float(m.findMedianThres(docA, KMED)), "B": float(m.findMedianThres(docB, KMED))}
        exp["findMedianStructurePointsThres"] = {"A": float(m.findMedianStructurePointsThres(docA, KMED)),
                                                 "B": float(m.findMedianStructurePointsThres(docB, KMED))}
        moved = copy.deepcopy(docB)
        m.transform_sfm_data(moved, M)
        exp["transform_sfm_data"] = {"extrinsics": moved["extrinsics"],
                                     "X": [s["value"]["X"] for s in moved["structure"]]}
        runs = []
        for seed in range(5):
            random.seed(seed)
            Mr, ir = m.ransacAffineTransform(A, B, MS.THRES, A.shape[1] * 100, 1.75)
            runs.append({"seed": seed, "M": np.asarray(Mr).tolist(), "inliers": [int(i) for i in ir]})
        exp["ransacAffineTransform"] = runs
        m.merge_sfm_data(docA, docB, M, {match[x][0]: match[x][1] for x in inl})
        exp["merge_sfm_data"] = docA
        merged = os.path.join(tmp, "merged.json")
        with open(merged, "w") as fh:
            json.dump(docA, fh)
        exp["modelMergeCheckLocal"] = [int(x) for x in m.modelMergeCheckLocal(merged, loc, CHECK_THRES)]
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "expected.json"), "w") as fh:
        json.dump(exp, fh, indent=None, sort_keys=True, default=float)
        fh.write("\n")
    print({k: (len(v) if hasattr(v, "__len__") else v) for k, v in exp.items()})
    print("ransacAffineTransform inliers:", [len(r["inliers"]) for r in exp["ransacAffineTransform"]])


if __name__ == "__main__":
    main()
