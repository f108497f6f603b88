"""openMVG_main_GlobalSfM over the C ABI: a folder of features and matches becomes a posed, triangulated, adjusted map --
the step PyReconstruct/src/reconstructGraph.py:171 runs and whose <outDir>/sfm_data.json it waits for.

    python -m sfmlocalization_amd.globalsfm -i <sfm_data.json> -m <matchDir> -o <outDir> [--triplet-angle 5] [--device 0]
                                            [--pair-scales] [--refine] [--register]

Three stages, each the run() of its own tool, the files of one the input of the next:
    sfmlocalization_amd.relpose       matches.f.txt -> <outDir>/matches.e.txt, <outDir>/relative_poses.json
    sfmlocalization_amd.globalposes   relative_poses.json -> <outDir>/sfm_data_poses.json (the views in the component posed)
    sfmlocalization_amd.structure     sfm_data_poses.json + matches.e.txt -> <outDir>/sfm_data.json: tracks, the robust
                                      triangulation, the cleanup at 4.0 px / 2.0 degrees, then rotations, translations and
                                      structure adjusted jointly (rst) on the same resident handle and cleaned again
--pair-scales: relpose also writes <outDir>/pair_scales.json (its -s) and globalposes reads it (its -s), so that the
spacing of cameras along a line comes from the depths of shared features; without it the chain is what it was.
--refine: relpose adjusts every ok pair's pose on its inliers (its --refine) before the averaging sees it.
--register: structure grows the map to the views the averaging left without a pose (its --register): they are resected
against the triangulated structure and the structure is extended, before the joint adjustment.
The first stage that fails ends the run with its message and its exit code.  Python only: there is no C++ program for
the chain (the stages' own C++ programs can be run one after the other).
"""
import os
import sys

from . import globalposes, relpose, structure

NAME = "openMVG_main_GlobalSfM"
USAGE = (f"Usage: {NAME}\n"
         "[-i|--input_file] path to a SfM_Data scene\n"
         "[-m|--matchdir] path to the features and matches that correspond to the provided SfM_Data scene\n"
         "[-o|--outdir] path where the output data will be stored\n"
         "\n[Optional]\n"
         "[--triplet-angle] largest angle of a triplet's cycle rotation in degrees (5)\n"
         "[--device] HIP device (0)\n"
         "[--pair-scales] fix the pair baselines from shared features (relpose -s, globalposes -s)\n"
         "[--refine] adjust every relative pose on its inliers before the averaging (relpose --refine)\n"
         "[--register] resect the views left without a pose against the structure and extend it (structure --register)\n")


def run(in_path, match_dir, out_dir, triplet_angle=5.0, device=0, log=print, pair_scales=False, refine=False,
        register=False):
    """The tool's body.  Returns 0, or the exit code of the stage that failed after its message on stderr."""
    os.makedirs(out_dir, exist_ok=True)
    essential = os.path.join(os.path.abspath(out_dir), "matches.e.txt")
    poses = os.path.join(os.path.abspath(out_dir), "relative_poses.json")
    posed = os.path.join(out_dir, "sfm_data_poses.json")
    scales = os.path.join(os.path.abspath(out_dir), "pair_scales.json") if pair_scales else None
    extra = dict(scales_file=scales) if pair_scales else {}
    if refine:
        extra["refine"] = True
    rc = relpose.run(in_path, match_dir, out_file=essential, poses_file=poses, device=device, log=log, **extra)
    if rc:
        return rc
    extra = dict(scales_path=scales) if pair_scales else {}
    rc = globalposes.run(in_path, poses, posed, triplet_angle=triplet_angle, device=device, log=log, **extra)
    if rc:
        return rc
    return structure.run(posed, match_dir, os.path.join(out_dir, "sfm_data.json"), match_file=essential, residual_px=4.0,
                         angle_deg=2.0, device=device, log=log, joint=True, **({"register": True} if register else {}))


def parse_args(argv):
    """-> the keyword arguments of run(), or None for a bad command line"""
    opt = {"-i": "", "-m": "", "-o": "", "--triplet-angle": "5", "--device": "0"}
    long_names = {"--input_file": "-i", "--matchdir": "-m", "--outdir": "-o"}
    i = 0
    flag = refine = register = False
    while i < len(argv):
        a = argv[i]
        if a in ("--pair-scales", "--refine", "--register"):
            flag, refine = flag or a == "--pair-scales", refine or a == "--refine"
            register = register or a == "--register"
            i += 1
            continue
        if "=" in a and a.split("=", 1)[0] in ("--triplet-angle", "--device"):
            a, val = a.split("=", 1)
        else:
            a = long_names.get(a, a)
            if a not in opt or i + 1 >= len(argv):
                return None
            val = argv[i + 1]
            i += 1
        opt[a] = val
        i += 1
    try:
        kw = dict(in_path=opt["-i"], match_dir=opt["-m"], out_dir=opt["-o"], triplet_angle=float(opt["--triplet-angle"]),
                  device=int(opt["--device"]))
        if flag:
            kw["pair_scales"] = True
        if refine:
            kw["refine"] = True
        if register:
            kw["register"] = True
    except ValueError:
        return None
    if not kw["in_path"] or not kw["match_dir"] or not kw["out_dir"] or not 0.0 < kw["triplet_angle"] < 180.0:
        return None
    return kw


def main(argv=None):
    kw = parse_args(sys.argv[1:] if argv is None else list(argv))
    if kw is None:
        sys.stderr.write(USAGE)
        return 1

    def log(s):
        print(s, flush=True)
    return run(log=log, **kw)


if __name__ == "__main__":
    sys.exit(main())
