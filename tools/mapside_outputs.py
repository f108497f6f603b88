"""A SHA-256 of everything the map-side stages give on the test suites' scenes, one line per array or file, so that two
builds of the library can be compared output for output:

    python tools/mapside_outputs.py [--bin sfmlocalization_amd/bin] > listing.txt      # once per build, then diff

The library is the one sfmlocalization_amd loads (SFMLOC_LIB_PATH names another build); --bin is the folder of that
build's C++ tools.  Nothing is asserted and no time is in the listing: two listings are equal or they are not.

  chain    register_scene.make_scene_a on ONE handle: triangulate, clean, adjust (structure), adjust_joint (rst),
           register, color_plan -- after every stage its report and the handle's state (poses, masks, X, intrinsics).
  sparse   adjust_scene.sparse_views_case(257): resect (every view's result and inlier list), adjust (rotations and
           translations), color_plan.
  tools    OpenMVG_BA on adjust_ba_scene's document (-r=1; -c=s; -c=rt,sc -r=1; -c=rst,rstic -r=1 -j=1),
           openMVG_main_ComputeStructureFromKnownPoses on scene A (plain and --register) and ComputeRelativePoses on
           relpose_scene: every file they write, and their standard output without the lines that carry a time."""
import argparse
import ctypes
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adjust_ba_scene as BS  # noqa: E402
import adjust_scene as AS  # noqa: E402
import register_scene as RS  # noqa: E402
import relpose_scene as PS  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

TIMED = re.compile(r"\b(ms|seconds?|sec|s\))\b|\d s\b")


def sha(name, data):
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data).tobytes()
    print(hashlib.sha256(data).hexdigest(), name, flush=True)


def fields(r):
    """a report structure without its time, or the list / tuple of arrays a call returned, as bytes"""
    if isinstance(r, ctypes.Structure):
        return json.dumps([[f, getattr(r, f)] for f, _ in r._fields_ if f != "device_ms"]).encode()
    return b"".join(np.ascontiguousarray(x).tobytes() for x in r)


def state(tag, h, masks=True):
    p = h.read(masks=masks)
    for f in sorted(p):
        sha(f"{tag} {f}", p[f])
    sha(f"{tag} X", h.read_structure())
    sha(f"{tag} intrinsics", h.read_intrinsics())


def view_results(tag, results, inliers):
    for k, r in enumerate(results):
        sha(f"{tag} view {k} result", bytes(r))
        sha(f"{tag} view {k} inliers", inliers(k))


def chain():
    h = S.Sfm(**RS.make_scene_a()["arrays"])
    for name, stage in (("triangulate", lambda: h.triangulate()), ("clean", lambda: h.clean(4.0, 2.0, False)),
                        ("adjust_s", lambda: h.adjust(S.BA_STRUCTURE)),
                        ("adjust_joint_rst", lambda: h.adjust_joint(S.BA_ROTATION | S.BA_TRANSLATION | S.BA_STRUCTURE)),
                        ("register", lambda: h.register()), ("color_plan", lambda: h.color_plan())):
        sha(f"chain {name} report", fields(stage()))
        state(f"chain {name}", h)
    res, rnd = h.register_read()
    sha("chain register rounds", rnd)
    view_results("chain register", res, h.register_inliers)
    h.close()


def sparse():
    h = S.Sfm(**AS.sparse_views_case(257))
    sha("sparse resect counts", np.array(h.resect()))
    view_results("sparse resect", h.resect_read(), h.resect_inliers)
    state("sparse resect", h, masks=False)
    sha("sparse adjust_rt report", fields(h.adjust(S.BA_ROTATION | S.BA_TRANSLATION)))
    state("sparse adjust_rt", h, masks=False)
    sha("sparse color_plan", fields(h.color_plan()))
    h.close()


def run_tool(tag, cmd, folder, work):
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    sha(f"{tag} status", str(r.returncode).encode())
    lines = [l.replace(work, "<work>") for l in r.stdout.splitlines() if not TIMED.search(l)]   # (a temporary folder's name)
    sha(f"{tag} stdout", "\n".join(lines).encode())
    for f in sorted(os.listdir(folder)):
        with open(os.path.join(folder, f), "rb") as fh:
            sha(f"{tag} {f}", fh.read())


def tools(bin_dir, work):
    doc = BS.make_doc()[0]
    for tag, args in (("r1", ["-r=1"]), ("c_s", ["-c=s"]), ("c_rt_sc", ["-c=rt,sc", "-r=1"]),
                      ("joint", ["-c=rst,rstic", "-r=1", "-j=1"])):
        d = os.path.join(work, "ba_" + tag)
        os.makedirs(d)
        with open(os.path.join(d, "sfm_data.json"), "w") as fh:
            json.dump(doc, fh)
        run_tool("OpenMVG_BA " + tag, [os.path.join(bin_dir, "OpenMVG_BA"), os.path.join(d, "sfm_data.json"),
                                      os.path.join(d, "out.json")] + args, d, work)
    scene = RS.make_scene_a()
    for tag, args in (("plain", []), ("register", ["--register"])):
        d = os.path.join(work, "structure_" + tag)
        os.makedirs(d)
        path = RS.write_files(scene, d)
        run_tool("ComputeStructureFromKnownPoses " + tag,
                 [os.path.join(bin_dir, "openMVG_main_ComputeStructureFromKnownPoses"), "-i", path, "-m", d, "-o",
                  os.path.join(d, "out.json")] + args, d, work)
    d = os.path.join(work, "relpose")
    os.makedirs(d)
    path = PS.write_files(PS.make_scene(), d)
    run_tool("ComputeRelativePoses", [os.path.join(bin_dir, "ComputeRelativePoses"), "-i", path, "-m", d], d, work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin", default=os.path.join(ROOT, "sfmlocalization_amd", "bin"))
    args = ap.parse_args()
    chain()
    sparse()
    with tempfile.TemporaryDirectory() as work:
        tools(os.path.abspath(args.bin), work)


if __name__ == "__main__":
    main()
