"""The sfm_data the OpenMVG_BA tests run on (synthdata.make_map, 60 views, obs.x from its structure) with the planted
cases of the issue, and the CPU expectation: the oracle's resection of every view (oracle_c.p3p_localize on the raw
obs.x in ascending landmark id, stream = id_view) followed by the NumPy cleanup restatement (adjust_np)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import synthdata  # noqa: E402

SEED = 0x5F3759DF12345678
RADIAL_K = (-0.08, 0.02, 0.0)
RADIAL_F, RADIAL_PP = 760.0, (331.5, 236.25)   # the second intrinsic has its own focal and principal point
FEW_VIEWS = (3, 24, 45)            # views left with 10 or fewer observations
FAIL_VIEW = 17                     # 12 observations, each a random pixel: the resection fails
WEAK_VIEW = 30                     # 5 observations (not resected), keeps its pose: -r=1 erases it
ORPHAN_POSE = 100000               # an extrinsic no view names: -r=1 erases it


def _disto(p, k):
    r2 = p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]
    r4 = r2 * r2
    r6 = r4 * r2
    rc = ((1.0 + k[0] * r2) + k[1] * r4) + k[2] * r6
    return p * rc[:, None]


def make_doc(seed=61, outlier_shift=(6.0, 25.0)):
    m = synthdata.make_map(seed, n_views=60, desc_per_view=300, views_per_place=20, landmarks_per_place=400,
                           obs_per_view=120)
    rng = np.random.Generator(np.random.PCG64(seed + 1))
    f, ppx, ppy = m.intrinsic
    radial_view = np.arange(60) >= 40                 # views 40..59 on a pinhole_radial_k3 intrinsic
    slot_view = np.searchsorted(m.view_off, np.arange(m.n_rows), side="right") - 1
    per_lm = {}
    for r in np.nonzero(m.row_landmark >= 0)[0]:
        k = int(slot_view[r])
        per_lm.setdefault(int(m.row_landmark[r]), []).append([k, int(r - m.view_off[k])])
    structure = []
    for s in sorted(per_lm):
        X = m.landmark_X[s]
        obs = []
        for k, feat in sorted(per_lm[s]):
            Xc = (X - m.view_C[k]) @ m.view_R[k].T
            p = (Xc[:2] / Xc[2])[None, :]
            if radial_view[k]:
                x = (RADIAL_F * _disto(p, RADIAL_K)[0] + np.array(RADIAL_PP)) + rng.normal(0, 0.3, 2)
            else:
                x = (f * p[0] + np.array([ppx, ppy])) + rng.normal(0, 0.3, 2)
            obs.append([k, feat, x])
        structure.append([int(m.landmark_id[s]), X.copy(), obs])
    # planted outliers: 4 % of the observations pushed 6..25 px away
    for lm in structure:
        for o in lm[2]:
            if rng.uniform() < 0.04:
                ang = rng.uniform(0, 2 * np.pi)
                o[2] = o[2] + rng.uniform(*outlier_shift) * np.array([np.cos(ang), np.sin(ang)])
    # near-degenerate tracks: far landmarks (rays under 2 degrees) seen exactly by three views of a place
    next_id = max(lm[0] for lm in structure) + 5
    for t in range(12):
        ks = [t % 20 + 1, (t + 5) % 20 + 1, (t + 11) % 20 + 1]
        d = m.place_center[0] - m.view_C[ks[0]]
        X = m.view_C[ks[0]] + d / np.linalg.norm(d) * 3000.0 + rng.uniform(-40, 40, 3)
        obs = []
        for k in ks:
            Xc = (X - m.view_C[k]) @ m.view_R[k].T
            obs.append([k, 1000 + t, f * (Xc[:2] / Xc[2]) + np.array([ppx, ppy])])
        structure.append([next_id, X, obs])
        next_id += 3
    # a view whose resection fails, views with too few observations, a weak view
    for lm in structure:
        for o in lm[2]:
            if o[0] == FAIL_VIEW:
                o[2] = np.array([rng.uniform(0, 640), rng.uniform(0, 480)])
    keep_n = {v: 8 + i for i, v in enumerate(FEW_VIEWS)}
    keep_n[WEAK_VIEW] = 5
    keep_n[FAIL_VIEW] = 12
    seen = {v: 0 for v in keep_n}
    for lm in structure:
        new = []
        for o in lm[2]:
            if o[0] in keep_n:
                seen[o[0]] += 1
                if seen[o[0]] > keep_n[o[0]]:
                    continue
            new.append(o)
        lm[2] = new
    structure.sort(key=lambda t: t[0])
    views = []
    for k in range(60):
        v = {"key": int(m.view_id[k]), "value": {"polymorphic_id": 1073741824 if k else 2147483649, "ptr_wrapper": {
            "id": 2147483649 + k, "data": {"local_path": "/", "filename": f"img{k:06d}.jpg", "width": 640, "height": 480,
                                           "id_view": int(m.view_id[k]), "id_intrinsic": 1 if radial_view[k] else 0,
                                           "id_pose": int(m.view_id[k])}}}}
        if k == 0:
            v["value"]["polymorphic_name"] = "view"
        views.append(v)
    intr = [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole", "ptr_wrapper": {
                "id": 2147483709, "data": {"width": 640, "height": 480, "focal_length": float(f),
                                           "principal_point": [float(ppx), float(ppy)]}}}},
            {"key": 1, "value": {"polymorphic_id": 2147483651, "polymorphic_name": "pinhole_radial_k3", "ptr_wrapper": {
                "id": 2147483710, "data": {"value0": {"width": 640, "height": 480, "focal_length": RADIAL_F,
                                                      "principal_point": list(RADIAL_PP)},
                                           "disto_k3": [float(x) for x in RADIAL_K]}}}}]
    ext = [{"key": int(m.view_id[k]), "value": {"rotation": m.view_R[k].tolist(), "center": m.view_C[k].tolist()}}
           for k in range(60)]
    ext.append({"key": ORPHAN_POSE, "value": {"rotation": np.eye(3).tolist(), "center": [0.0, 0.0, 0.0]}})
    st = [{"key": lid, "value": {"X": [float(x) for x in X], "observations": [
        {"key": int(m.view_id[k]), "value": {"id_feat": int(feat), "x": [float(x[0]), float(x[1])]}}
        for k, feat, x in obs]}} for lid, X, obs in structure]
    doc = {"sfm_data_version": "0.3", "root_path": "/data/images", "views": views, "intrinsics": intr,
           "extrinsics": ext, "structure": st, "control_points": []}
    return doc, m


def view_lists(a):
    """per view: (observation indices in ascending landmark id)"""
    order = np.argsort(a["obs_view"], kind="stable")
    bounds = np.searchsorted(a["obs_view"][order], np.arange(len(a["view_id"]) + 1))
    return [order[bounds[k]:bounds[k + 1]] for k in range(len(a["view_id"]))]


def p3p_raw(oracle_c, pt2d, pt3d, f, ppx, ppy, seed, stream, max_iteration=4096):
    """oracle_c.p3p_localize without the wrapper's cut: the wrapper keeps the inliers only when Localize's gate (more
    than 2.5 * 3) passes, but the C function fills the buffer with the best model's inliers, P and errmax regardless.
    -> dict(n (the gated count), inl_raw (the whole buffer: its first n_in entries are AC-RANSAC's inliers, n_in
    unknown below the gate), P, errmax, nfa, iters)"""
    import ctypes as C
    pt2d = np.ascontiguousarray(pt2d, np.float64)
    pt3d = np.ascontiguousarray(pt3d, np.float64)
    n = len(pt2d)
    inl = np.full(max(n, 1), -1, np.int32)
    P = np.zeros(12)
    nfa, em, it = C.c_double(), C.c_double(), C.c_int()
    dp = C.POINTER(C.c_double)
    k = oracle_c.lib().orc_p3p_localize(pt2d.ctypes.data_as(dp), pt3d.ctypes.data_as(dp), C.c_int(n), C.c_double(f),
                                        C.c_double(ppx), C.c_double(ppy), C.c_int(max_iteration), C.c_uint64(seed),
                                        C.c_uint32(stream), inl.ctypes.data_as(C.POINTER(C.c_int32)),
                                        P.ctypes.data_as(dp), C.byref(em), C.byref(nfa), C.byref(it))
    return {"n": k, "inl_raw": inl[:n].copy(), "inliers": inl[:k].copy(), "P": P.reshape(3, 4), "errmax": em.value,
            "nfa": nfa.value, "iters": it.value}


def oracle_resect(a, oracle_c, seed=SEED):
    """-> per view dict(ran, ok, n, inliers, inl_raw, iters, P, errmax, nfa, R, center) and the pose table after the
    re-resection"""
    off = a["obs_off"].astype(np.int64)
    obs_lm = np.repeat(np.arange(len(a["landmark_id"])), np.diff(off))
    out = []
    pv, R, C = a["pose_valid"].astype(bool).copy(), a["pose_R"].copy(), a["pose_C"].copy()
    for k, idx in enumerate(view_lists(a)):
        r = {"ran": len(idx) > 10, "ok": False, "n_obs": len(idx)}
        if r["ran"]:
            K = a["intrinsic"][a["view_intrinsic"][k]]
            o = p3p_raw(oracle_c, a["obs_x"][idx], a["landmark_X"][obs_lm[idx]], K[0], K[1], K[2], seed,
                        int(a["view_id"][k]))
            r.update(o)
            if o["n"] >= 8:
                _, Rr, _, c = oracle_c.krt_from_p(o["P"])
                r.update(ok=True, R=Rr, center=c)
                p = a["view_pose"][k]
                pv[p], R[p], C[p] = True, Rr.reshape(9), c
        out.append(r)
    return out, pv, R, C


def two_pass_case():
    """A small sfm_data (arrays) whose -r=1 fixed point needs two erasing passes, with exact projections and wide rays so
    that the residual and angle filters keep everything: pose 0 has 5 observations and goes in pass 1; its landmarks
    are left with one observation and go, which leaves pose 1 with 1 and it goes in pass 2; pose 3 is named by no view
    (0 observations) and goes in pass 1; poses 2 and 4 keep 21 and 20.  Callers clean without resecting: the input
    poses are the exact ones."""
    rng = np.random.Generator(np.random.PCG64(3))
    cams = [np.array([-2.0, 0, 0]), np.array([0.0, 0, 0]), np.array([2.0, 0, 0]), np.array([0.0, 2.0, 0])]
    f, ppx, ppy = 800.0, 320.0, 240.0
    groups = [([0, 1], 5), ([1, 2], 1), ([2, 3], 20)]
    lm_X, obs_off, obs_view, obs_x = [], [0], [], []
    for views, n in groups:
        for _ in range(n):
            X = rng.uniform([-1, -1, 8], [1, 1, 12])
            lm_X.append(X)
            for k in views:
                d = X - cams[k]
                obs_view.append(k)
                obs_x.append([f * d[0] / d[2] + ppx, f * d[1] / d[2] + ppy])
            obs_off.append(len(obs_view))
    pose_C = np.array([cams[0], cams[1], cams[2], [9.0, 9.0, 9.0], cams[3]])
    return dict(view_id=np.array([0, 1, 2, 3], np.uint32), view_intrinsic=np.zeros(4, np.uint32),
                view_pose=np.array([0, 1, 2, 4], np.uint32), intrinsic_type=np.zeros(1, np.uint32),
                intrinsic=np.array([[f, ppx, ppy, 0.0, 0.0, 0.0]]), pose_valid=np.ones(5, np.uint8),
                pose_R=np.tile(np.eye(3).reshape(1, 9), (5, 1)), pose_C=pose_C,
                landmark_id=np.arange(len(lm_X), dtype=np.uint32) * 4 + 2, landmark_X=np.array(lm_X),
                obs_off=np.array(obs_off, np.uint64), obs_view=np.array(obs_view, np.uint32),
                obs_x=np.array(obs_x, np.float64))


SPARSE_OBSERVED = (0, 1, 254, 255, 256)    # with the last view: the only views of sparse_views_case that see anything
SPARSE_FEW = {0: 12, 1: 10}                # view 0 is resected on 12 observations, view 1 (10) is not


def radix_key_bits(max_key):
    """csrc/radix_sort.h radix_key_bits: the key bits the transpose's sort looks at for view indices 0..max_key"""
    return int(max_key).bit_length()


def sparse_views_case(n_views, seed=7):
    """arrays (as two_pass_case) for the transpose's sort as adjust.hip compiles it: n_views views on one pinhole
    intrinsic, cameras on an arc looking at a cloud of landmarks, every view with a pose; only the views
    SPARSE_OBSERVED and n_views - 1 (those that exist) have observations, exact projections plus 0.3 px of noise.
    Views 0 and 1 see 12 and 10 landmarks; every other observed view sees q of 2 q landmarks, q = 200 or, where that
    leaves the total under 1025, the smallest q that reaches it (with four such views 251): the sort then runs over
    more than one block, with radix_key_bits(n_views - 1) = 8 or 9 key bits -- one pass, or two whose second one sorts on
    the bit that parts view 256 and later from the rest.  n_views = 1: a single view with 200 observations, zero key
    bits, no pass."""
    rng = np.random.Generator(np.random.PCG64(seed + n_views))
    f, ppx, ppy = 800.0, 320.0, 240.0
    observed = sorted({v for v in SPARSE_OBSERVED + (n_views - 1,) if v < n_views})
    full = [v for v in observed if v not in SPARSE_FEW or n_views == 1]
    q = 200 if n_views == 1 else max(200, -(-(1025 - sum(SPARSE_FEW.values())) // len(full)))
    X = rng.uniform([-2.0, -1.5, -2.0], [2.0, 1.5, 2.0], (2 * q, 3))
    ang = np.linspace(-0.6, 0.6, n_views) if n_views > 1 else np.zeros(1)
    pose_C = np.stack([12.0 * np.sin(ang), 0.3 * np.cos(5.0 * ang), -12.0 * np.cos(ang)], 1)
    pose_R = np.zeros((n_views, 3, 3))
    for k in range(n_views):                                    # rows: right, down, forward (towards the origin)
        fw = -pose_C[k] / np.linalg.norm(pose_C[k])
        right = np.cross([0.0, 1.0, 0.0], fw)
        right /= np.linalg.norm(right)
        pose_R[k] = np.stack([right, np.cross(fw, right), fw])
    sees = {v: set(rng.permutation(2 * q)[:(q if v in full else SPARSE_FEW[v])].tolist()) for v in observed}
    lm_X, obs_off, obs_view, obs_x = [], [0], [], []
    for l in range(2 * q):
        views = [v for v in observed if l in sees[v]]
        if not views:
            continue
        lm_X.append(X[l])
        for v in views:
            Xc = pose_R[v] @ (X[l] - pose_C[v])
            obs_view.append(v)
            obs_x.append(f * Xc[:2] / Xc[2] + np.array([ppx, ppy]) + rng.normal(0, 0.3, 2))
        obs_off.append(len(obs_view))
    return dict(view_id=np.arange(n_views, dtype=np.uint32), view_intrinsic=np.zeros(n_views, np.uint32),
                view_pose=np.arange(n_views, dtype=np.uint32), intrinsic_type=np.zeros(1, np.uint32),
                intrinsic=np.array([[f, ppx, ppy, 0.0, 0.0, 0.0]]), pose_valid=np.ones(n_views, np.uint8),
                pose_R=pose_R.reshape(n_views, 9), pose_C=pose_C,
                landmark_id=np.arange(len(lm_X), dtype=np.uint32) * 3 + 1, landmark_X=np.array(lm_X),
                obs_off=np.array(obs_off, np.uint64), obs_view=np.array(obs_view, np.uint32),
                obs_x=np.array(obs_x, np.float64))
