#!/usr/bin/env python3
"""Build-container script (needs the reference tree and scipy, as make_merge_fixtures.py needs the tree; never runs on
the GPU box): what the reference's own world-coordinate functions return on the small documents of
tests/globalcoord_scene.py, recorded as data under tests/golden/globalcoord_ref/expected.json.  The modules
(PyEvaluateAccuracy/src/localizeGlobalCoordinateRefPoint.py, hulo_file/SfmDataUtils.py, hulo_file/FileUtils.py) are
Python 2 text: they are converted in memory with lib2to3 (make_ref_fixtures.import_py2) and executed; nothing of them is
written anywhere.  The iBeacon parameter modules the script imports are not in that tree: two empty stand-ins.

Recorded: reduceClosePointsKDTree on every scene and reduceClosePoints on those where knn does not bind (keeper keys and
observation lists), saveGlobalSfM, the bytes of Amat.txt / convertNumpyMatTxt2OpenCvMatYml, and the loc_global
arithmetic (:358-362) on tests/golden/ref_consumers/loc_cli/q00*.json.

    python tests/golden/make_globalcoord_fixtures.py
"""
import contextlib
import copy
import io
import json
import os
import sys
import tempfile
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "globalcoord_ref")
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import make_ref_fixtures as ref  # noqa: E402
import globalcoord_scene as GS  # noqa: E402

SCRIPT = "../../PyEvaluateAccuracy/src/localizeGlobalCoordinateRefPoint.py"
LOC_CLI = os.path.join(HERE, "ref_consumers", "loc_cli")


def summary(doc):
    return [[s["key"], [[ob["key"], ob["value"]["id_feat"]] for ob in s["value"]["observations"]]] for s in doc["structure"]]


def load_modules():
    if not hasattr(np, "float"):
        np.float = float
    for name in ("hulo_ibeacon.LocalizeIBeaconParam", "hulo_ibeacon.ReconstructIBeaconParam"):
        sys.modules.setdefault("hulo_ibeacon", types.ModuleType("hulo_ibeacon"))
        mod = types.ModuleType(name)
        setattr(mod, name.rsplit(".", 1)[1], type(name.rsplit(".", 1)[1], (), {}))
        sys.modules[name] = mod
        setattr(sys.modules["hulo_ibeacon"], name.rsplit(".", 1)[1], mod)
    for rel, name, pkg in (("hulo_file/FileUtils.py", "hulo_file.FileUtils", "hulo_file"),
                           ("hulo_file/PlyUtils.py", "hulo_file.PlyUtils", "hulo_file"),
                           ("hulo_file/SfmDataUtils.py", "hulo_file.SfmDataUtils", "hulo_file"),
                           ("hulo_sfm/mergeSfM.py", "hulo_sfm.mergeSfM", "hulo_sfm"),
                           ("hulo_param/ReconstructParam.py", "hulo_param.ReconstructParam", "hulo_param"),
                           ("hulo_param/LocalizeParam.py", "hulo_param.LocalizeParam", "hulo_param"),
                           ("hulo_bow/LocalizeBOWParam.py", "hulo_bow.LocalizeBOWParam", "hulo_bow")):
        ref.import_py2(rel, name, package_modules=(pkg,))
    return ref.import_py2(SCRIPT, "ref_localizeGlobalCoordinateRefPoint"), sys.modules["hulo_file.SfmDataUtils"], \
        sys.modules["hulo_file.FileUtils"]


def main():
    with contextlib.redirect_stdout(io.StringIO()):
        script, sfmutils, futils = load_modules()
    exp = {"reduce": {}}
    scenes = GS.reduce_scenes()
    with tempfile.TemporaryDirectory() as tmp, contextlib.redirect_stdout(io.StringIO()):
        for name, (doc, A, thres, knn, binds) in scenes.items():
            d = copy.deepcopy(doc)
            script.reduceClosePointsKDTree(d, A, thres, knn)
            exp["reduce"][name] = {"kdtree": summary(d)}
            if not binds:
                d = copy.deepcopy(doc)
                script.reduceClosePoints(d, A, thres)
                exp["reduce"][name]["brute"] = summary(d)
        doc, A = scenes["clusters"][0], scenes["clusters"][1]
        src, txt, yml, dst = (os.path.join(tmp, n) for n in ("sfm_data.json", "Amat.txt", "Amat.yml", "global.json"))
        with open(src, "w") as fh:
            json.dump(doc, fh)
        with open(txt, "w") as fh:
            np.savetxt(fh, A)
        futils.convertNumpyMatTxt2OpenCvMatYml(txt, yml, "A")
        sfmutils.saveGlobalSfM(src, txt, dst)
        with open(dst) as fh:
            moved = json.load(fh)
        exp["Amat"] = A.tolist()
        exp["Amat.txt"] = open(txt).read()
        exp["Amat.yml"] = open(yml).read()
        exp["saveGlobalSfM"] = {"extrinsics": moved["extrinsics"], "X": [s["value"]["X"] for s in moved["structure"]]}
        with open(script.__file__) as fh:                       # the script's own lines :358-362, executed, not copied
            block = compile(textwrap.dedent("\n".join(fh.read().split("\n")[357:362])), script.__file__, "exec")
        glob = []
        for name in sorted(os.listdir(LOC_CLI)):
            with open(os.path.join(LOC_CLI, name)) as fh:
                scope = {"np": np, "Amat": A, "jsonLoc": json.load(fh)}
            exec(block, scope)
            glob.append({k: scope["jsonLoc"][k] for k in ("t", "R", "t_relative", "R_relative") if k in scope["jsonLoc"]})
        exp["loc_global"] = glob
    os.makedirs(OUT, exist_ok=True)
    with open(os.path.join(OUT, "expected.json"), "w") as fh:
        json.dump(exp, fh, indent=None, sort_keys=True, default=float)
        fh.write("\n")
    print({k: [len(doc["structure"]), len(exp["reduce"][k]["kdtree"])] for k, (doc, *_) in scenes.items()})


if __name__ == "__main__":
    main()
