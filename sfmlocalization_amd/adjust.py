"""OpenMVG_BA (OpenMVG_BA/src/adjust_sfm_data.cpp) over the C ABI: the call the reference's merge loop makes once per
candidate merge (hulo_sfm/sfmMergeGraph.py:297, hulo_bow/sfmMergeGraphBOW.py:226,
hulo_ibeacon/sfmMergeGraphIBeacon.py:322), and the separable commands of its -c switch.

    python -m sfmlocalization_amd.adjust <sfm_data> <sfm_data_out> [-c=...] [-r=0|1] [-j=0|1] [--device=0]

Every view with more than 10 observations is re-resected on the device, <folder of sfm_data>/sfm_data_b4bd.json is
written with the new poses and the structure untouched, the structure is cleaned (residual 4 px, angle 2 degrees, the
unstable poses with -r=1) and the result goes to sfm_data_out (in place works).  Both files are json.dump of the
document: views, intrinsics, root_path and key order as in the input, extrinsics in ascending pose id, control_points
[].  bin/OpenMVG_BA (csrc/adjust_cli.cpp) is the same program and writes the same bytes.

-c=item,item,... (adjust_sfm_data.cpp:158-244): after the re-resection and sfm_data_b4bd.json every item is run in
order: s adjusts the structure alone, r / t / rt the rotations / translations / both alone (sfmloc_sfm_adjust: every
landmark or pose is a problem of its own), and a c in the item cleans afterwards (4 px, 2 degrees, -r) and prints the
four counts.  An item with none of r t i s adjusts nothing.  With a non-empty -c there is no final cleanup of its own
(the reference cleans in the else branch only), and the output holds the adjusted poses (C = -R^T t) and X.  The joint
commands -- structure together with a pose part (rs, rst, ...) and anything with i -- are not supported yet: every item
is checked before anything is opened, and one refused item ends the run with status 1 and nothing written.  The
semantics are stated in include/sfmloc.h.

-j=1 (--joint=1, in any position) opts in to the joint adjustment: no item is refused, an item that would be goes to
sfmloc_sfm_adjust_joint with the default options (one Levenberg-Marquardt problem over everything the item names), a
separable item still goes to sfmloc_sfm_adjust (-c=rt,sc -j=1 gives the bytes of -c=rt,sc).  An intrinsic whose bits
changed is written from the arrays (focal_length, principal_point, disto_k3); sfm_data_b4bd.json keeps the input's.
"""
import json
import os
import sys

import numpy as np

RESIDUAL_PX, ANGLE_DEG = 4.0, 2.0          # STRUCTURE_CLEANUP_RESIDUAL_ERROR / _ANGLE_ERROR (adjust_sfm_data.cpp:40-41)
INTRINSIC_TYPES = {"pinhole": 0, "pinhole_radial_k3": 3}
UNSUPPORTED_TYPE = 0xFFFFFFFF                # any other intrinsic type (sfmloc_sfm_create refuses it)

USAGE = ("Execute bundle adjustment for sfm_data.json\n"
         "Usage: OpenMVG_BA [params] sfm_data sfm_data_out\n"
         "\t-c, --command\n\t\tCommand for order of bundle adjustment (BD) [default=no BD] [options:r = rotation, "
         "t = translation, s = structure, c = clean]. Usage example: c=r,tc,s means BD with rotation only, then BD with "
         "translation follow by cleaning, then BD with structure. Not supported yet: i (intrinsic), and s together "
         "with r or t.\n"
         "\t-r, --rm_unstable (value:0)\n\t\tRemove unstable pose and observation\n"
         "\t-j, --joint (value:0)\n\t\tWith 1, run the items that are not supported yet (i, and s together with r or t) as "
         "one joint bundle adjustment\n")


def _u32(v):
    if not isinstance(v, int) or isinstance(v, bool) or not 0 <= v <= 0xFFFFFFFF:
        raise ValueError("malformed id")
    return v


def sfm_arrays(doc):
    """sfm_data document -> the arrays of sfmloc_sfm_desc, the pose ids of the pose table and the input's extrinsic
    values (None for a pose id only a view names).  Raises ValueError on what the tool refuses."""
    views, intrs = doc["views"], doc["intrinsics"]
    exts, st = doc.get("extrinsics", []), doc.get("structure", [])
    type_names, intr_index, intr_type, intr = {}, {}, [], []
    for e in intrs:                        # cereal names a polymorphic type at its first occurrence only
        val = e["value"]
        pid = _u32(val["polymorphic_id"]) & 0x7FFFFFFF
        if "polymorphic_name" in val:
            type_names[pid] = val["polymorphic_name"]
        t = type_names.get(pid, "")
        k = [0.0] * 6
        if t in INTRINSIC_TYPES:        # (any other type goes to sfmloc_sfm_create, which refuses it: SFMLOC_EIO)
            data = val["ptr_wrapper"]["data"]
            pin = data["value0"] if t == "pinhole_radial_k3" else data
            k = [float(pin["focal_length"]), float(pin["principal_point"][0]), float(pin["principal_point"][1]), 0.0, 0.0,
                 0.0]
            if t == "pinhole_radial_k3":
                k[3:] = [float(x) for x in data["disto_k3"]]
        intr_index[_u32(e["key"])] = len(intr_type)
        intr_type.append(INTRINSIC_TYPES.get(t, UNSUPPORTED_TYPE))
        intr.append(k)
    ext_by_id = {_u32(e["key"]): e["value"] for e in exts}
    view_id, view_intr, view_pose_id, view_index = [], [], [], {}
    for e in views:
        data = e["value"]["ptr_wrapper"]["data"]
        vid = _u32(data["id_view"])
        if view_id and vid <= view_id[-1]:
            raise ValueError("views are not in ascending id_view")
        ii = _u32(data["id_intrinsic"])
        if ii not in intr_index:
            raise ValueError(f"view {vid}: no intrinsic {ii}")
        view_index[vid] = len(view_id)
        view_id.append(vid)
        view_intr.append(intr_index[ii])
        view_pose_id.append(_u32(data["id_pose"]))
    pose_id = sorted(set(ext_by_id) | set(view_pose_id))
    pose_index = {p: i for i, p in enumerate(pose_id)}
    pose_valid = np.zeros(len(pose_id), np.uint8)
    pose_R = np.zeros((len(pose_id), 9))
    pose_C = np.zeros((len(pose_id), 3))
    pose_src = []
    for i, p in enumerate(pose_id):
        src = ext_by_id.get(p)
        pose_src.append(src)
        if src is not None:
            pose_valid[i] = 1
            pose_R[i] = np.array(src["rotation"], np.float64).reshape(9)
            pose_C[i] = np.array(src["center"], np.float64).reshape(3)
    lm_id, lm_X, obs_off, obs_view, obs_x = [], [], [0], [], []
    for e in st:
        lid = _u32(e["key"])
        if lm_id and lid <= lm_id[-1]:
            raise ValueError("structure is not in ascending landmark id")
        lm_id.append(lid)
        lm_X.append([float(x) for x in e["value"]["X"]])
        for o in e["value"]["observations"]:
            vid = _u32(o["key"])
            if vid not in view_index:
                raise ValueError(f"landmark {lid}: observation of unknown view {vid}")
            obs_view.append(view_index[vid])
            obs_x.append([float(x) for x in o["value"]["x"]])
        obs_off.append(len(obs_view))
    arrays = dict(view_id=np.array(view_id, np.uint32), view_intrinsic=np.array(view_intr, np.uint32),
                  view_pose=np.array([pose_index[p] for p in view_pose_id], np.uint32),
                  intrinsic_type=np.array(intr_type, np.uint32), intrinsic=np.array(intr, np.float64).reshape(-1, 6),
                  pose_valid=pose_valid, pose_R=pose_R, pose_C=pose_C, landmark_id=np.array(lm_id, np.uint32),
                  landmark_X=np.array(lm_X, np.float64).reshape(-1, 3), obs_off=np.array(obs_off, np.uint64),
                  obs_view=np.array(obs_view, np.uint32), obs_x=np.array(obs_x, np.float64).reshape(-1, 2))
    return arrays, pose_id, pose_src


def _extrinsics(pose_id, pose_src, valid, R, C, replaced):
    out = []
    for i, p in enumerate(pose_id):
        if not valid[i]:
            continue
        if pose_src[i] is not None and not replaced[i]:
            out.append({"key": p, "value": pose_src[i]})
        else:
            out.append({"key": p, "value": {"rotation": [[float(x) for x in row] for row in np.asarray(R[i]).reshape(3, 3)],
                                            "center": [float(x) for x in C[i]]}})
    return out


def _with(doc, **items):
    out = dict(doc)
    for k, v in items.items():
        out[k] = v
    return out


def _write(path, doc):
    with open(path, "w") as fh:
        json.dump(doc, fh)


def command_items(command):
    """-c split on commas as the reference's getline loop splits it (no item after a trailing comma)"""
    items = command.split(",") if command else []
    if items and items[-1] == "":
        items.pop()
    return items


def refused_item(items):
    """the first item that is not separable (structure with a pose part, or intrinsics), or None"""
    for item in items:
        if "i" in item or ("s" in item and ("r" in item or "t" in item)):
            return item
    return None


def _bits_differ(a, b):
    return (np.ascontiguousarray(a, np.float64).view(np.uint64) != np.ascontiguousarray(b, np.float64).view(np.uint64))


def _intrinsics(doc, arrays, K):
    """the document's intrinsics with every entry whose bits changed written from K (f, ppx, ppy, k1, k2, k3)"""
    out = []
    for i, e in enumerate(doc["intrinsics"]):
        if _bits_differ(K[i], arrays["intrinsic"][i]).any():
            radial = int(arrays["intrinsic_type"][i]) == 3
            val = e["value"]
            data = val["ptr_wrapper"]["data"]
            pin = data["value0"] if radial else data
            pin = _with(pin, focal_length=float(K[i][0]), principal_point=[float(K[i][1]), float(K[i][2])])
            data = _with(data, value0=pin, disto_k3=[float(x) for x in K[i][3:]]) if radial else pin
            e = _with(e, value=_with(val, ptr_wrapper=_with(val["ptr_wrapper"], data=data)))
        out.append(e)
    return out


def run(in_path, out_path, rm_unstable=False, device=0, log=print, command="", joint=False):
    """The tool's body.  Returns 0, or 1 after an error message on stderr."""
    from . import capi as S
    items = command_items(command)
    log("Start bundle adjustment over sfm_data.json.")
    log(f"Reading sfm_data.json file : {in_path}")
    try:
        with open(in_path) as fh:
            doc = json.load(fh)
        arrays, pose_id, pose_src = sfm_arrays(doc)
    except (OSError, ValueError, KeyError, TypeError, IndexError) as e:
        print(f"\nThe input sfm_data.json file \"{in_path}\" cannot be read. ({e})", file=sys.stderr)
        return 1
    try:
        h = S.Sfm(**arrays, params=S.sfm_default_params(device=int(device)))
    except S.SfmlocError as e:
        print(f"OpenMVG_BA: {e.message}", file=sys.stderr)
        return 1
    try:
        h.resect()
        res = h.resect_read()
        replaced = np.zeros(len(pose_id), bool)
        for k, r in enumerate(res):
            if r.ok:
                replaced[arrays["view_pose"][k]] = True
        if any(not r.ran for r in res):
            log("Warning: there is/are frames with too few matches.")
        p = h.read(masks=False)
        b4 = _with(doc, extrinsics=_extrinsics(pose_id, pose_src, p["pose_valid"], p["pose_R"], p["pose_C"], replaced),
                   control_points=[])
        _write(os.path.join(os.path.dirname(in_path), "sfm_data_b4bd.json"), b4)

        def clean():
            counts = h.clean(RESIDUAL_PX, ANGLE_DEG, rm_unstable)
            log(f"Number of points before cleanup : {counts[0]}")
            log(f"Number of points residual error : {counts[1]}")
            log(f"Number of points angle error : {counts[2]}")
            log(f"Number of points after cleanup : {counts[3]}")
        cleaned = False
        for item in items:
            rot, trn, intr, stru = "r" in item, "t" in item, joint and "i" in item, "s" in item
            log("\nBundle adjustment over " + ("rotations, " if rot else "") + ("translations, " if trn else "")
                + ("intrinsic params, " if intr else "") + ("structure, " if stru else ""))
            what = (S.BA_ROTATION if rot else 0) | (S.BA_TRANSLATION if trn else 0) | \
                (S.BA_INTRINSICS if intr else 0) | (S.BA_STRUCTURE if stru else 0)
            if joint and refused_item([item]) is not None:
                h.adjust_joint(what)
            else:
                h.adjust(what)
            if "c" in item:
                clean()
                cleaned = True
        if not items:
            clean()
            cleaned = True
        q = h.read(masks=cleaned)
        X = h.read_structure() if items else None
        K = h.read_intrinsics() if items and joint else None
    except S.SfmlocError as e:
        print(f"OpenMVG_BA: {e.message}", file=sys.stderr)
        return 1
    finally:
        h.close()
    if items:          # a pose or a landmark the adjustment moved is written from the arrays, the others as they were
        moved = _bits_differ(q["pose_R"].reshape(-1, 9), p["pose_R"].reshape(-1, 9)).any(1) | \
            _bits_differ(q["pose_C"], p["pose_C"]).any(1)
        replaced = replaced | moved
        p = q
    off = arrays["obs_off"]
    structure = []
    for l, e in enumerate(doc.get("structure", [])):
        if cleaned and not q["landmark_keep"][l]:
            continue
        val = e["value"]
        if cleaned:
            obs = [o for j, o in enumerate(val["observations"]) if q["obs_keep"][int(off[l]) + j]]
            val = _with(val, observations=obs)
        if X is not None and _bits_differ(X[l], arrays["landmark_X"][l]).any():
            val = _with(val, X=[float(x) for x in X[l]])
        structure.append(_with(e, value=val))
    out = _with(doc, extrinsics=_extrinsics(pose_id, pose_src, q["pose_valid"], p["pose_R"], p["pose_C"], replaced))
    if K is not None:
        out["intrinsics"] = _intrinsics(doc, arrays, K)
    if "structure" in doc:
        out["structure"] = structure
    out["control_points"] = []
    _write(out_path, out)
    return 0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    if len(argv) < 1:
        sys.stderr.write(USAGE)
        return 1
    pos, command, rm_unstable, device, joint = [], "", 0, 0, 0
    for a in argv:
        if a in ("-h", "--help"):
            sys.stderr.write(USAGE)
            return 1
        if a.startswith("-c=") or a.startswith("--command="):
            command = a.split("=", 1)[1]
        elif a.startswith("-r=") or a.startswith("--rm_unstable="):
            try:
                rm_unstable = int(a.split("=", 1)[1])
            except ValueError:
                rm_unstable = 0
        elif a.startswith("-j=") or a.startswith("--joint="):
            try:
                joint = int(a.split("=", 1)[1])
            except ValueError:
                joint = 0
        elif a.startswith("--device="):
            device = int(a.split("=", 1)[1])
        elif a.startswith("-"):
            sys.stderr.write(USAGE)
            return 1
        else:
            pos.append(a)
    if len(pos) < 2 or not pos[0] or not pos[1]:
        sys.stderr.write(USAGE)
        return 1
    bad = None if joint else refused_item(command_items(command))
    if bad is not None:
        print(f"OpenMVG_BA: -c={command}: item \"{bad}\" is not supported yet (-c adjusts the structure alone, or "
              "rotations / translations alone; no intrinsics); nothing was written", file=sys.stderr)
        return 1

    def log(s):
        print(s, flush=True)
    return run(pos[0], pos[1], rm_unstable=rm_unstable != 0, device=device, log=log, command=command, joint=joint != 0)


if __name__ == "__main__":
    sys.exit(main())
