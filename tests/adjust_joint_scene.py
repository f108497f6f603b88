"""The scenes of the joint bundle adjustment tests.

wide()   adjust_ba_scene's document (imported, not edited) with every view cloned N_CLONES times: a clone has its own
         id_view and id_pose (the pair that shares a pose shares one in every clone), starts from its original's pose,
         and observes its original's landmarks 0.3 px beside where the original saw them.  The planted block sizes of
         adjust_ba_scene cross the 8-lane group, the 64-lane wave and the 256-thread workgroup over observations; the
         clones cross the two remaining widths of ba_joint.hip with views and poses that observe: over 512 views per
         intrinsic (the per-intrinsic sum strides by 256: two full strides) and 1 030 poses with observations (the
         one-workgroup passes stride by 1024).
small()  a hand-made scene of 3 views and 8 landmarks, every view seeing every landmark: everything inside one wave;
         second_intrinsic=True adds an intrinsic no view uses.
"""
import copy
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adjust_ba_scene as BS  # noqa: E402

COMMANDS = (11, 15, 9, 7, 8, 3)    # rst, rsti, rs, rti, and two separable ones the joint call accepts as well: s, rt
NAMES = {11: "rst", 15: "rsti", 9: "rs", 7: "rti", 8: "s", 3: "rt"}
N_CLONES, CLONE_ID_STEP, CLONE_PIXEL_SIGMA = 4, 1000, 0.3


def wide_doc(seed=17):
    base, planted = BS.make_doc()
    doc = copy.deepcopy(base)
    rng = np.random.Generator(np.random.PCG64(seed))
    ext = {e["key"]: e["value"] for e in base["extrinsics"]}
    for c in range(1, N_CLONES + 1):
        step = c * CLONE_ID_STEP
        poses = set()
        for k, src in enumerate(base["views"]):
            v = copy.deepcopy(src)
            d = v["value"]["ptr_wrapper"]["data"]
            v["key"] = src["key"] + step
            v["value"]["ptr_wrapper"]["id"] = 2147483649 + c * BS.N_VIEWS + k
            d.update(filename=f"clone{c}_{k:06d}.jpg", id_view=d["id_view"] + step, id_pose=d["id_pose"] + step)
            doc["views"].append(v)
            if d["id_pose"] not in poses:
                poses.add(d["id_pose"])
                doc["extrinsics"].append({"key": d["id_pose"], "value": copy.deepcopy(ext[d["id_pose"] - step])})
        for e, src in zip(doc["structure"], base["structure"]):
            for o in src["value"]["observations"]:
                x = np.array(o["value"]["x"]) + rng.normal(0.0, CLONE_PIXEL_SIGMA, 2)
                e["value"]["observations"].append({"key": o["key"] + step, "value": {
                    "id_feat": o["value"]["id_feat"] + 100000 * c, "x": [float(x[0]), float(x[1])]}})
    doc["extrinsics"].sort(key=lambda e: e["key"])
    return doc, planted


def small(second_intrinsic=False, seed=3):
    """-> arrays as adjust.sfm_arrays returns them"""
    rng = np.random.Generator(np.random.PCG64(seed))
    K = np.array([[800.0, 320.0, 240.0, 0.0, 0.0, 0.0], [700.0, 300.0, 250.0, 0.05, -0.01, 0.002]])
    itype = np.array([0, 3], np.uint32)
    view_intr = np.array([0, 1, 0], np.uint32)
    C = np.array([[-1.0, 0.0, -6.0], [0.0, 0.5, -6.5], [1.2, -0.3, -6.0]])
    R = np.stack([BS._look_at(C[k], np.array([0.0, 0.0, 0.0]) + 0.1 * k) for k in range(3)])
    X = rng.uniform(-1.0, 1.0, (8, 3))
    obs_view, obs_x = [], []
    for l in range(8):
        for v in range(3):
            obs_view.append(v)
            obs_x.append(BS._project(K[view_intr[v]], itype[view_intr[v]] == 3, R[v], C[v], X[l]) + rng.normal(0, 0.5, 2))
    R0 = np.stack([BS._rodrigues(rng.normal(0, 1, 3) * 0.01) @ R[k] for k in range(3)])
    if second_intrinsic:
        K = np.concatenate([K, [[650.0, 310.0, 245.0, 0.01, 0.02, 0.03]]])
        itype = np.array([0, 3, 3], np.uint32)
    return dict(view_id=np.array([4, 9, 11], np.uint32), view_intrinsic=view_intr, view_pose=np.arange(3, dtype=np.uint32),
                intrinsic_type=itype, intrinsic=K * (1.0 + 1e-3 * np.array([1, -1, 1, 0, 0, 0])),
                pose_valid=np.ones(3, np.uint8), pose_R=R0.reshape(3, 9), pose_C=C + rng.normal(0, 0.03, (3, 3)),
                landmark_id=np.arange(8, dtype=np.uint32) * 2 + 1, landmark_X=X + rng.normal(0, 0.03, X.shape),
                obs_off=np.arange(9, dtype=np.uint64) * 3, obs_view=np.array(obs_view, np.uint32),
                obs_x=np.array(obs_x, np.float64))


def twins(a, what, obs_keep=None, landmark_keep=None):
    """both twin solutions of command `what` with what they leave between them: r_ref (largest distance of a residual
    component, pixels) and c_ref (relative distance of the total cost)"""
    import adjust_joint_np as JN
    sol = {k: JN.adjust(a, what, a["pose_R"], a["pose_C"], a["intrinsic"], a["landmark_X"], k, obs_keep, landmark_keep)
           for k in ("lm", "scipy")}
    r_ref = float(np.abs(sol["lm"]["residual"] - sol["scipy"]["residual"]).max())
    c_ref = abs(sol["lm"]["cost1"] - sol["scipy"]["cost1"]) / sol["scipy"]["cost1"]
    return dict(sol, r_ref=r_ref, c_ref=float(c_ref))


@functools.lru_cache(maxsize=None)
def reference():
    """wide() as arrays, the masks of the first cleanup (BS.FIRST_CLEAN) and the twins of every command from that state.
    Computed once per process; callers must not change it."""
    import adjust_np as AN
    from sfmlocalization_amd import adjust
    doc, planted = wide_doc()
    a, pose_id, _ = adjust.sfm_arrays(doc)
    first = AN.clean(a, a["pose_valid"], a["pose_R"], a["pose_C"], *BS.FIRST_CLEAN)
    out = {"doc": doc, "a": a, "pose_id": pose_id, "planted": planted, "obs_keep": first["obs_keep"],
           "landmark_keep": first["landmark_keep"], "first_counts": first["counts"], "cmd": {}}
    for what in COMMANDS:
        out["cmd"][what] = twins(a, what, first["obs_keep"], first["landmark_keep"])
    return out
