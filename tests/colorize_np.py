"""NumPy restatement of the landmark colouring (include/sfmloc.h "colouring plan", sfmlocalization_amd/colorize.py): the
plain loop as OpenMVG's ColorizeTracks writes it -- every iteration recounts every view from scratch over the landmarks
that are left, takes the view with the most (np.argmax: the lowest index among equals) and colours the landmarks that
observe it.  Deliberately not the decremental form the device uses.  Also the sampler and the PLY writer, written from
the statement and not from the package's code; images are decoded by sfmloc_image_read (host code with tests of its own,
tests/test_image_io.py)."""
import os

import numpy as np

UNSET = 0xFFFFFFFF


def plan(n_views, obs_off, obs_view):
    """-> (order [n_order] u32, lm_iter [n_lm] u32, lm_obs [n_lm] u64)"""
    obs_off = np.asarray(obs_off, np.int64)
    obs_view = np.asarray(obs_view, np.int64)
    n_lm = len(obs_off) - 1
    obs_lm = np.repeat(np.arange(n_lm), np.diff(obs_off))
    lm_iter = np.full(n_lm, UNSET, np.uint32)
    lm_obs = np.zeros(n_lm, np.uint64)
    left = np.diff(obs_off) > 0                      # a landmark without observations is never coloured
    order = []
    while left.any():
        card = np.bincount(obs_view[left[obs_lm]], minlength=n_views)
        v = int(np.argmax(card))
        assert card[v] > 0
        hit = np.flatnonzero((obs_view == v) & left[obs_lm])      # the remaining landmarks' observations in v
        lms, first = np.unique(obs_lm[hit], return_index=True)     # (a landmark's first one, should it have two)
        lm_iter[lms] = len(order)
        lm_obs[lms] = hit[first]
        left[lms] = False
        order.append(v)
    return np.array(order, np.uint32), lm_iter, lm_obs


def pixel(c, n):
    """the C cast (int)c, truncating toward zero, then clamped to the image"""
    if c != c:
        return 0
    return min(max(int(c), 0), n - 1) if abs(c) < 1e18 else (0 if c < 0 else n - 1)


def colours(n_lm, order, lm_iter, lm_obs, obs_x, image_of_view):
    """rgb [n_lm, 3]; image_of_view(v) -> B G R array [h, w, 3]; unobserved landmarks stay black"""
    rgb = np.zeros((n_lm, 3), np.uint8)
    for k, v in enumerate(order):
        img = image_of_view(int(v))
        h, w = img.shape[:2]
        for l in np.flatnonzero(lm_iter == k):
            x, y = obs_x[int(lm_obs[l])]
            b, g, r = img[pixel(float(y), h), pixel(float(x), w)]
            rgb[l] = (r, g, b)
    return rgb


def ply(X, rgb, centres):
    lines = ["ply", "format ascii 1.0", "element vertex " + str(len(X) + len(centres)), "property float x",
             "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
             "end_header"]
    for p, c in zip(X, rgb):
        lines.append(" ".join(["%g" % float(t) for t in p] + [str(int(t)) for t in c]))
    for p in centres:
        lines.append(" ".join(["%g" % float(t) for t in p]) + " 0 255 0")
    return "\n".join(lines) + "\n"


def document_ply(doc, read_bgr):
    """the whole tool on a parsed sfm_data document -> the PLY text"""
    views = [e["value"]["ptr_wrapper"]["data"] for e in doc["views"]]
    index = {d["id_view"]: i for i, d in enumerate(views)}
    poses = {e["key"]: e["value"]["center"] for e in doc.get("extrinsics", [])}
    off, view, xs, X = [0], [], [], []
    for s in doc.get("structure", []):
        X.append(s["value"]["X"])
        for o in s["value"]["observations"]:
            view.append(index[o["key"]])
            xs.append(o["value"]["x"])
        off.append(len(view))
    order, it, ob = plan(len(views), off, view)
    rgb = colours(len(X), order, it, ob, xs,
                  lambda v: read_bgr(os.path.join(doc["root_path"], views[v]["filename"])))
    return ply(X, rgb, [poses[d["id_pose"]] for d in views if d["id_pose"] in poses])
