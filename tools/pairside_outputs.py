"""A SHA-256 of everything the pair-side stages give on the test suites' scenes, one line per array or file, so that two
builds of the library can be compared output for output (the map side's counterpart is tools/mapside_outputs.py):

    python tools/pairside_outputs.py [--bin sfmlocalization_amd/bin] > listing.txt      # once per build, then diff

The library is the one sfmlocalization_amd loads (SFMLOC_LIB_PATH names another build); --bin is the folder of that
build's C++ tools.  Nothing is asserted and no time is in the listing: two listings are equal or they are not.

  calls    relpose_scene.make_scene(): RelPoses (results, inl_off, inl_idx), RelRefine fed from them, WedgeScales fed
           from the refined poses (records, report), once more each with every second pair left out, Tracks (counts,
           off, view, feat).
  global   GlobalPoses on globalposes_scene.scene_ring; with wedges on pairscales_scene.scene_corridor, the wedges
           being WedgeScales' records there (views, pair records, report; baselines, weights and scale report).
  tools    ComputeRelativePoses on globalposes_scene.scene_files (plain; --refine; -s; --refine -s) and on
           relpose_scene.make_scene() (--refine -s), ComputeGlobalPoses on the poses of the former's last run (with
           and without -s) and openMVG_main_ComputeStructureFromKnownPoses on
           register_scene.make_scene_a: every file they write (a JSON report without its *_ms fields), and their
           standard output without the lines that carry a time."""
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

import globalposes_scene as GS  # noqa: E402
import pairscales_scene as WS  # noqa: E402
import register_scene as RS  # noqa: E402
import relpose_scene as PS  # noqa: E402
import relrefine_cases  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

TIMED = re.compile(r"\b(ms|seconds?|sec|s\))\b|\d s\b")


def sha(name, data):
    if isinstance(data, np.ndarray):
        data = np.ascontiguousarray(data).tobytes()
    print(hashlib.sha256(data).hexdigest(), name, flush=True)


def fields(r):
    """a report structure without its times"""
    assert isinstance(r, ctypes.Structure)
    return json.dumps([[f, getattr(r, f)] for f, _ in r._fields_ if not f.endswith("_ms")]).encode()


def untimed(doc):
    """a JSON document without the members whose name ends in _ms"""
    if isinstance(doc, dict):
        return {k: untimed(v) for k, v in doc.items() if not k.endswith("_ms")}
    return [untimed(v) for v in doc] if isinstance(doc, list) else doc


def calls():
    args, _ = PS.call_arrays(PS.make_scene())
    rp = S.RelPoses(**args)
    sha("calls RelPoses results", rp.results)
    sha("calls RelPoses inl_off", rp.inl_off)
    sha("calls RelPoses inl_idx", rp.inl_idx)
    call = relrefine_cases.call_from_device(args, rp)
    half = dict(call, use_pair=np.asarray(call["use_pair"]) * (np.arange(len(call["pairs"])) % 2 == 0))
    for tag, c in (("all", call), ("every second", half)):
        fine = S.RelRefine(**c)
        sha(f"calls RelRefine {tag} results", fine.results)
        R, t = np.array(c["rel_R"], np.float64).reshape(-1, 9), np.array(c["rel_t"], np.float64).reshape(-1, 3)
        R[fine.refined], t[fine.refined] = fine.results["R"][fine.refined], fine.results["t"][fine.refined]
        w = S.WedgeScales(**dict(c, rel_R=R, rel_t=t))
        sha(f"calls WedgeScales {tag} records", w.records)
        sha(f"calls WedgeScales {tag} report", fields(w.report))
    trk = S.Tracks(args["view_off"], args["pairs"], args["offsets"], args["match_i"], args["match_j"])
    sha("calls Tracks counts", np.array(trk.counts, np.uint64))
    for f in ("off", "view", "feat"):
        sha(f"calls Tracks {f}", getattr(trk, f))


def gposes(tag, g, scaled):
    for f in ("in_component", "R", "C", "pairs"):
        sha(f"global {tag} {f}", getattr(g, f))
    sha(f"global {tag} report", fields(g.report))
    if scaled:
        sha(f"global {tag} baselines", g.baselines)
        sha(f"global {tag} wedge_weights", g.wedge_weights)
        sha(f"global {tag} scale_report", fields(g.scale_report))


def global_poses():
    s = GS.scene_ring()
    gposes("ring", S.GlobalPoses(s["n_views"], s["pairs"], s["rel_R"], s["rel_t"], s["use_t"]), False)
    s = WS.scene_corridor()
    w = S.WedgeScales(**s["call"])
    sha("global corridor wedges", w.records)
    gposes("corridor scaled", S.GlobalPoses(len(s["R_true"]), s["pairs"], s["rel_R"], s["rel_t"], wedges=w.records), True)


def run_tool(tag, cmd, folder, work, skip=()):
    """skip: the files that were in the folder before"""
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    sha(f"{tag} status", str(r.returncode).encode())
    lines = [l.replace(work, "<work>") for l in r.stdout.splitlines() if not TIMED.search(l)]   # (a temporary folder's name)
    sha(f"{tag} stdout", "\n".join(lines).encode())
    for f in sorted(set(os.listdir(folder)) - set(skip)):
        with open(os.path.join(folder, f), "rb") as fh:
            data = fh.read()
        if f.endswith("report.json"):
            data = json.dumps(untimed(json.loads(data))).encode()
        sha(f"{tag} {f}", data)


def tools(bin_dir, work):
    exe = lambda name: os.path.join(bin_dir, name)  # noqa: E731
    for tag, args in (("plain", []), ("refine", ["--refine"]), ("scales", ["-s", "pair_scales.json"]),
                      ("refine scales", ["--refine", "-s", "pair_scales.json"])):
        d = os.path.join(work, "relpose_" + tag.replace(" ", "_"))
        os.makedirs(d)
        path = GS.scene_files(d)["path"]
        before = os.listdir(d)
        run_tool("ComputeRelativePoses " + tag, [exe("ComputeRelativePoses"), "-i", path, "-m", d] + args, d, work, before)
    r = os.path.join(work, "relpose_scene")
    os.makedirs(r)
    rpath = PS.write_files(PS.make_scene(), r)
    run_tool("ComputeRelativePoses relpose_scene", [exe("ComputeRelativePoses"), "-i", rpath, "-m", r, "--refine", "-s",
                                                    "pair_scales.json"], r, work, os.listdir(r))
    for tag, args in (("plain", []), ("scales", ["-s", os.path.join(d, "pair_scales.json")])):
        g = os.path.join(work, "gposes_" + tag)
        os.makedirs(g)
        run_tool("ComputeGlobalPoses " + tag,
                 [exe("ComputeGlobalPoses"), "-i", path, "-p", os.path.join(d, "relative_poses.json"), "-o",
                  os.path.join(g, "out.json"), "-r", os.path.join(g, "report.json")] + args, g, work)
    d = os.path.join(work, "structure")
    os.makedirs(d)
    path = RS.write_files(RS.make_scene_a(), d)
    run_tool("ComputeStructureFromKnownPoses", [exe("openMVG_main_ComputeStructureFromKnownPoses"), "-i", path, "-m", d,
                                                "-o", os.path.join(d, "out.json")], d, work)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--bin", default=os.path.join(ROOT, "sfmlocalization_amd", "bin"))
    args = ap.parse_args()
    calls()
    global_poses()
    with tempfile.TemporaryDirectory() as work:
        tools(os.path.abspath(args.bin), work)


if __name__ == "__main__":
    main()
