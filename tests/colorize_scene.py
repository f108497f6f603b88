"""Scenes of the landmark-colouring tests: sfm_data documents over given observation lists, small image writers (binary
PPM, PNG through zlib) and the seeded observation structures that each reach one part of the device code."""
import struct
import zlib

import numpy as np

W, H = 64, 48


def write_ppm(path, rgb):
    rgb = np.ascontiguousarray(rgb, np.uint8)
    with open(path, "wb") as fh:
        fh.write(b"P6\n%d %d\n255\n" % (rgb.shape[1], rgb.shape[0]) + rgb.tobytes())


def write_png(path, img):
    """8-bit gray [h, w] or RGB [h, w, 3], filter 0 on every row"""
    img = np.ascontiguousarray(img, np.uint8)
    h, w = img.shape[:2]
    raw = b"".join(b"\x00" + img[r].tobytes() for r in range(h))

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data))
    with open(path, "wb") as fh:
        fh.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2 if img.ndim == 3 else 0, 0, 0, 0))
                 + chunk(b"IDAT", zlib.compress(raw)) + chunk(b"IEND", b""))


def document(root_path, names, sizes, centres, landmarks, first_key=0, key_step=1):
    """names / sizes [(w, h)] per view (view k has id_view = id_pose = k); centres {view: [x, y, z]} (the views with a
    pose); landmarks [(X, [(view, x, y), ...])]"""
    views = []
    for k, (name, (w, h)) in enumerate(zip(names, sizes)):
        v = {"key": k, "value": {"polymorphic_id": 1073741824 if k else 2147483649, "ptr_wrapper": {
            "id": 2147483649 + k, "data": {"local_path": "/", "filename": name, "width": w, "height": h, "id_view": k,
                                           "id_intrinsic": 0, "id_pose": k}}}}
        if k == 0:
            v["value"]["polymorphic_name"] = "view"
        views.append(v)
    intr = [{"key": 0, "value": {"polymorphic_id": 2147483650, "polymorphic_name": "pinhole", "ptr_wrapper": {
        "id": 2147483700, "data": {"width": W, "height": H, "focal_length": 50.0, "principal_point": [W / 2, H / 2]}}}}]
    ext = [{"key": k, "value": {"rotation": np.eye(3).tolist(), "center": [float(t) for t in c]}}
           for k, c in sorted(centres.items())]
    st = [{"key": first_key + key_step * i, "value": {"X": [float(t) for t in X], "observations": [
        {"key": int(v), "value": {"id_feat": j, "x": [float(x), float(y)]}} for j, (v, x, y) in enumerate(obs)]}}
        for i, (X, obs) in enumerate(landmarks)]
    return {"sfm_data_version": "0.3", "root_path": root_path, "views": views, "intrinsics": intr, "extrinsics": ext,
            "structure": st, "control_points": []}


def csr(rows):
    """[[view, ...] per landmark] -> (obs_off u64, obs_view u32)"""
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    view = np.array([v for r in rows for v in r], np.uint32)
    return off, view


def sfm_arrays(n_views, rows, seed=0):
    """the arrays of capi.Sfm for an observation structure: one pinhole, every view with a pose, pixels inside 64 x 48"""
    rng = np.random.Generator(np.random.PCG64(seed))
    off, view = csr(rows)
    n_lm = len(rows)
    return dict(view_id=np.arange(n_views, dtype=np.uint32), view_intrinsic=np.zeros(n_views, np.uint32),
                view_pose=np.arange(n_views, dtype=np.uint32), intrinsic_type=np.zeros(1, np.uint32),
                intrinsic=np.array([[50.0, W / 2, H / 2, 0, 0, 0]]), pose_valid=np.ones(n_views, np.uint8),
                pose_R=np.tile(np.eye(3).reshape(9), (n_views, 1)), pose_C=rng.uniform(-1, 1, (n_views, 3)),
                landmark_id=np.arange(n_lm, dtype=np.uint32) * 2 + 5, landmark_X=rng.uniform(-5, 5, (n_lm, 3)),
                obs_off=off, obs_view=view, obs_x=rng.uniform(0, 1, (len(view), 2)) * [W - 1, H - 1])


def random_rows(rng, n_views, n_lm, lo, hi):
    """n_lm landmarks, each seen by lo..hi distinct views in ascending view order"""
    return [sorted(rng.permutation(n_views)[:rng.integers(lo, hi + 1)].tolist()) for _ in range(n_lm)]


def plan_scenes(chunk):
    """-> {name: (n_views, rows)}; `chunk` = the iterations the implementation enqueues per host read"""
    rng = np.random.Generator(np.random.PCG64(2024))
    out = {"small": (7, random_rows(rng, 7, 50, 2, 6))}
    # all ties: 300 views on a ring, landmark i seen by views i and i + 1 -- every view starts with 2 and the counts
    # stay equal over long runs of iterations
    out["all_ties"] = (300, [sorted([i, (i + 1) % 300]) for i in range(300)])
    # many iterations: chunk + 1 views must each be chosen (a private landmark each), one more than one host chunk
    n = chunk + 1
    out["many_iterations"] = (n, [[v] for v in range(n)] + random_rows(rng, n, 40, 2, 3))
    # long list: view 3 sees 5 000 landmarks (several workgroups of the update pass), among short lists
    rows = [sorted({3, int(rng.integers(0, 20))}) for _ in range(5000)] + random_rows(rng, 20, 300, 1, 3)
    out["long_list"] = (20, [rows[i] for i in rng.permutation(len(rows))])
    # stride: view 0 sees 66 000 landmarks, more than the update pass's whole grid (256 workgroups x 256 lanes)
    out["stride"] = (9, [[0, 1 + i % 8] for i in range(66000)])
    # hub: one landmark seen by 200 views (a long CSR row: 200 decrements from one lane)
    out["hub"] = (200, [list(range(200))] + random_rows(rng, 200, 400, 1, 4))
    # edges: view 4 without observations, landmarks 1 and 5 without any, and a landmark that names view 2 twice
    out["edges"] = (6, [[0, 1], [], [2, 3], [2, 2, 5], [1], [], [0, 5, 3]])
    out["no_landmarks"] = (3, [])
    return out
