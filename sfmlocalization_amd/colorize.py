"""openMVG_main_ComputeSfM_DataColor over the C ABI: the landmark colouring the reference runs after every
reconstruction and accepted merge (PyReconstruct/src/reconstructGraph.py:182,209, hulo_sfm/sfmMergeGraph.py:396-397), in
its world-coordinate scripts (localizeGlobalCoordinate.py:229-231) and inside hulo_file/PlyUtils.py; its output,
colorized.ply, goes into the finished map (SfmDataUtils.py:119).

    python -m sfmlocalization_amd.colorize -i <sfm_data.json> -o <out.ply> [--device=0]

The colouring plan -- which view every landmark takes its colour from, ColorizeTracks' greedy cover -- is computed on the
device (sfmloc_sfm_color_plan; include/sfmloc.h states the semantics).  The host then reads the chosen views' images in
plan order (sfmloc_image_read, colour; a gray file gives three equal channels) and samples the pixel at ((int)y, (int)x)
of the landmark's observation in that view: a few hundred pixels per frame, so no frame is uploaded.
bin/openMVG_main_ComputeSfM_DataColor (csrc/colorize_cli.cpp) is the same program and writes the same bytes.

Divergences from OpenMVG 1.1: a coordinate outside the image is clamped to the border (the reference reads out of bounds;
a NaN reads column or row 0); an image that cannot be read ends the run with status 1 and the file's name, and nothing
is written; a landmark without observations is written black.  The PLY is plyHelper::exportToPly's -- the landmarks in
ascending id with their colours, then the centre of every view that has a pose, in ascending view id, in green -- with
numbers as %g separated by single spaces (Eigen pads the columns of a row to a common width; every consumer in the
reference splits on whitespace, PlyUtils.py:67,90).

save_structure_ply, save_camera_ply and save_global_ply are PlyUtils.saveStructurePly, saveCameraPly and saveGlobalPly.
"""
import json
import os
import sys

import numpy as np

from . import adjust

NAME = "openMVG_main_ComputeSfM_DataColor"
USAGE = (f"Usage: {NAME}\n"
         "[-i|--input_file] path to the input SfM_Data scene\n"
         "[-o|--output_file] path to the output PLY file\n")
PLY_HEADER = ("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")


def pixel(c, n):
    """(int)c clamped to [0, n - 1], element-wise: the cast truncates toward zero; a NaN gives 0"""
    c = np.asarray(c, np.float64)
    inside = np.where(c >= n, n - 1, np.trunc(c))
    return np.where(c > 0.0, inside, 0).astype(np.int64)


def device_plan(arrays, device=0):
    """the colouring plan of the structure in `arrays` (adjust.sfm_arrays) -> (order, lm_iter, lm_obs)"""
    from . import capi as S
    h = S.Sfm(**arrays, params=S.sfm_default_params(device=int(device)))
    try:
        return h.color_plan()
    finally:
        h.close()


def _read_bgr(path):
    from . import capi as S
    return S.image_read(path, color=True)


def sample(doc, arrays, plan, read_bgr=_read_bgr):
    """colours [n_landmarks, 3] (r, g, b) of a plan: the images are read in plan order, one at a time.  Raises OSError
    naming the file when an image cannot be read."""
    order, lm_iter, lm_obs = plan
    rgb = np.zeros((len(arrays["landmark_id"]), 3), np.uint8)
    by_iter = np.argsort(lm_iter, kind="stable")
    first = np.searchsorted(lm_iter[by_iter], np.arange(len(order) + 1))
    root = doc.get("root_path", "")
    obs_x = arrays["obs_x"]
    for k, v in enumerate(order):
        path = os.path.join(root, doc["views"][int(v)]["value"]["ptr_wrapper"]["data"].get("filename", ""))
        try:
            img = read_bgr(path)
        except Exception as e:
            raise OSError(path) from e
        h, w = img.shape[:2]
        ls = by_iter[first[k]:first[k + 1]]
        xy = obs_x[lm_obs[ls].astype(np.int64)]
        rgb[ls] = img[pixel(xy[:, 1], h), pixel(xy[:, 0], w), ::-1]
    return rgb


def ply_text(X, rgb, centres):
    """plyHelper::exportToPly: points with their colours, then the camera centres in green"""
    out = [PLY_HEADER % (len(X) + len(centres))]
    for p, c in zip(X, rgb):
        out.append("%g %g %g %d %d %d\n" % (p[0], p[1], p[2], c[0], c[1], c[2]))
    for p in centres:
        out.append("%g %g %g 0 255 0\n" % (p[0], p[1], p[2]))
    return "".join(out)


def camera_centres(arrays):
    """the centre of every view whose pose is defined, in ascending view id"""
    vp = arrays["view_pose"]
    return [arrays["pose_C"][p] for p in vp if arrays["pose_valid"][p]]


def colorize_doc(doc, out_ply, device=0, plan_fn=device_plan):
    """the tool's body on a parsed document.  Returns 0, or 1 after an error message on stderr."""
    from . import capi as S
    arrays, _, _ = adjust.sfm_arrays(doc)
    n_lm = len(arrays["landmark_id"])
    plan = (np.zeros(0, np.uint32), np.full(n_lm, S.COLOR_UNSET, np.uint32), np.zeros(n_lm, np.uint64))
    try:
        if len(arrays["obs_view"]):                # (no observations: nothing to plan, no device call)
            plan = plan_fn(arrays, device)
        rgb = sample(doc, arrays, plan)
    except S.SfmlocError as e:
        print(f"{NAME}: {e.message}", file=sys.stderr)
        return 1
    except OSError as e:
        print(f"{NAME}: cannot read the image {e}", file=sys.stderr)
        return 1
    text = ply_text(arrays["landmark_X"], rgb, camera_centres(arrays))
    with open(out_ply, "w") as fh:
        fh.write(text)
    return 0


def run(in_sfm, out_ply, device=0, edit=None, plan_fn=device_plan):
    try:
        with open(in_sfm) as fh:
            doc = json.load(fh)
        if edit:
            edit(doc)
        adjust.sfm_arrays(doc)
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nThe input SfM_Data file \"{in_sfm}\" cannot be read. ({e})", file=sys.stderr)
        return 1
    return colorize_doc(doc, out_ply, device, plan_fn)


def save_structure_ply(in_sfm, out_ply, device=0):
    """PlyUtils.saveStructurePly (PlyUtils.py:28-36): the run with extrinsics = [] -- the landmarks alone"""
    return run(in_sfm, out_ply, device, edit=lambda doc: doc.__setitem__("extrinsics", []))


def save_camera_ply(in_sfm, out_ply, device=0):
    """PlyUtils.saveCameraPly (PlyUtils.py:38-46): the run with structure = [] -- the camera centres alone"""
    return run(in_sfm, out_ply, device, edit=lambda doc: doc.__setitem__("structure", []))


def save_global_ply(in_ply, Amat, out_ply):
    """PlyUtils.saveGlobalPly (PlyUtils.py:48-76): the header copied stripped; of every other non-empty line the first
    three values become A [.; 1] and are written as str(float), the last three values as int, each followed by a
    space"""
    Amat = np.asarray(Amat, np.float64)
    header = True
    with open(in_ply) as src, open(out_ply, "w") as fh:
        for line in src:
            line = line.strip()
            if header:
                fh.write(line + "\n")
                header = line.lower() != "end_header"
                continue
            if not line:
                continue
            val = np.array([float(t) for t in line.split()], np.float64)
            val[0:3] = np.dot(Amat[:, 0:3], val[0:3]) + Amat[:, 3]
            n = len(val)
            fh.write("".join((str(float(v)) if i < n - 3 else str(int(v))) + " " for i, v in enumerate(val)) + "\n")


def parse_args(argv):
    """-> (input, output, device), or None for a malformed command line"""
    a_in = a_out = None
    device = 0
    it = iter(argv)
    for a in it:
        if a in ("-i", "--input_file", "-o", "--output_file"):
            v = next(it, None)
            if v is None:
                return None
        elif a.startswith("--input_file=") or a.startswith("--output_file="):
            a, v = a.split("=", 1)
        elif a.startswith("--device="):
            try:
                device = int(a.split("=", 1)[1])
            except ValueError:
                return None
            continue
        else:
            return None
        if a in ("-i", "--input_file"):
            a_in = v
        else:
            a_out = v
    if not a_in or not a_out:
        return None
    return a_in, a_out, device


def main(argv=None):
    args = parse_args(sys.argv[1:] if argv is None else list(argv))
    if args is None:
        sys.stderr.write(USAGE)
        return 1
    return run(*args)


if __name__ == "__main__":
    sys.exit(main())
