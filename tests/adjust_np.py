"""NumPy restatement of the structure cleanup of sfmloc_sfm (include/sfmloc.h, "residual", "angle", "unstable"): the
residual norm per observation, the bearing rays and the minimum clamped cosine per landmark, and the -r fixed point.
Only + - * / sqrt in f64, elementwise and in the stated order (NumPy does not fuse), so residual norms and cosines are
the device's bits; the final acos is compared through the decision only.  Arrays as adjust.sfm_arrays returns them."""
import math

import numpy as np

LO, HI = -1.0 + 1.e-8, 1.0 - 1.e-8


def ud_pixel_k3(f, ppx, ppy, k1, k2, k3, x, y):
    """Pinhole_Intrinsic_Radial_K3::get_ud_pixel as geom_device.h restates it (bisection to 1e-8, capped loops)"""
    def disto(r2):
        t = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        return r2 * (t * t)
    px, py = (x - ppx) / f, (y - ppy) / f
    r2 = px * px + py * py
    radius = 1.0
    if r2 != 0.0:
        lo = up = r2
        it = 0
        while it < 4096 and disto(lo) > r2:
            lo = lo / 1.05
            it += 1
        it = 0
        while it < 4096 and disto(up) < r2:
            up = up * 1.05
            it += 1
        it = 0
        while it < 4096 and 1e-8 < up - lo:
            mid = 0.5 * (lo + up)
            if disto(mid) > r2:
                up = mid
            else:
                lo = mid
            it += 1
        radius = math.sqrt((0.5 * (lo + up)) / r2)
    return f * (radius * px) + ppx, f * (radius * py) + ppy


def observation_terms(a, pose_R, pose_C):
    """-> (residual norm [n_obs], world ray [n_obs, 3], ray norm [n_obs]) of every observation"""
    off = a["obs_off"].astype(np.int64)
    n_lm = len(a["landmark_id"])
    obs_lm = np.repeat(np.arange(n_lm), np.diff(off))
    v = a["obs_view"].astype(np.int64)
    pi = a["view_pose"][v].astype(np.int64)
    ii = a["view_intrinsic"][v].astype(np.int64)
    R = np.asarray(pose_R, np.float64).reshape(-1, 9)[pi]
    C = np.asarray(pose_C, np.float64).reshape(-1, 3)[pi]
    K = a["intrinsic"][ii]
    radial = a["intrinsic_type"][ii] == 3
    X = a["landmark_X"][obs_lm]
    x, y = a["obs_x"][:, 0], a["obs_x"][:, 1]
    f, ppx, ppy = K[:, 0], K[:, 1], K[:, 2]
    d0, d1, d2 = X[:, 0] - C[:, 0], X[:, 1] - C[:, 1], X[:, 2] - C[:, 2]
    X0 = (R[:, 0] * d0 + R[:, 1] * d1) + R[:, 2] * d2
    X1 = (R[:, 3] * d0 + R[:, 4] * d1) + R[:, 5] * d2
    X2 = (R[:, 6] * d0 + R[:, 7] * d1) + R[:, 8] * d2
    with np.errstate(divide="ignore", invalid="ignore"):
        p0, p1 = X0 / X2, X1 / X2
        r2 = p0 * p0 + p1 * p1
        r4 = r2 * r2
        r6 = r4 * r2
        rc = ((1.0 + K[:, 3] * r2) + K[:, 4] * r4) + K[:, 5] * r6
        p0 = np.where(radial, p0 * rc, p0)
        p1 = np.where(radial, p1 * rc, p1)
        ex, ey = x - (f * p0 + ppx), y - (f * p1 + ppy)
        res = np.sqrt(ex * ex + ey * ey)
    ux, uy = x.copy(), y.copy()
    for o in np.nonzero(radial)[0]:
        ux[o], uy[o] = ud_pixel_k3(*[float(t) for t in K[o]], float(x[o]), float(y[o]))
    b0, b1 = (ux - ppx) / f, (uy - ppy) / f
    b2 = np.ones_like(b0)
    bn = np.sqrt((b0 * b0 + b1 * b1) + b2 * b2)
    c0, c1, c2 = b0 / bn, b1 / bn, b2 / bn
    r0 = (R[:, 0] * c0 + R[:, 3] * c1) + R[:, 6] * c2
    r1 = (R[:, 1] * c0 + R[:, 4] * c1) + R[:, 7] * c2
    r2_ = (R[:, 2] * c0 + R[:, 5] * c1) + R[:, 8] * c2
    ray = np.stack([r0, r1, r2_], 1)
    rn = np.sqrt((r0 * r0 + r1 * r1) + r2_ * r2_)
    return res, ray, rn


def pair_cosines(ray, rn, idx):
    """clamped cosine of every pair (i < j) of the observations idx, in the device's pair order"""
    i, j = np.triu_indices(len(idx), 1)
    a, b = idx[i], idx[j]
    dot = (ray[a, 0] * ray[b, 0] + ray[a, 1] * ray[b, 1]) + ray[a, 2] * ray[b, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        c = dot / (rn[a] * rn[b])
    m = np.where(HI < c, HI, c)                 # max(LO, min(c, HI)) as OpenMVG's clamp: NaN -> LO
    return np.where(LO < m, m, LO)


def angle_deg(c):
    return math.acos(c) * 180.0 / math.pi


def clean(a, pose_valid, pose_R, pose_C, residual_px=4.0, angle_limit=2.0, rm_unstable=False):
    """The whole cleanup -> dict(res, min_cos, obs_keep, landmark_keep, stage, pose_valid, counts, passes).
    stage per landmark: 0 residual filter, 1 angle filter, 2 -r loop, 3 kept."""
    off = a["obs_off"].astype(np.int64)
    n_lm = len(a["landmark_id"])
    res, ray, rn = observation_terms(a, pose_R, pose_C)
    keep = ~(res > residual_px)
    stage = np.zeros(n_lm, np.uint8)
    min_cos = np.full(n_lm, np.nan)
    for l in range(n_lm):
        idx = np.arange(off[l], off[l + 1])[keep[off[l]:off[l + 1]]]
        if len(idx) < 2:
            continue
        c = pair_cosines(ray, rn, idx)
        min_cos[l] = min(HI, float(c.min()))
        stage[l] = 1 if angle_deg(min_cos[l]) < angle_limit else 3
    pv = np.asarray(pose_valid, bool).copy()
    passes = 0
    if rm_unstable:
        pv, keep, stage, passes = unstable(a, pv, keep, stage)
    counts = [n_lm, int((stage >= 1).sum()), int((stage >= 2).sum()), int((stage == 3).sum())]
    return {"res": res, "min_cos": min_cos, "obs_keep": keep, "landmark_keep": stage == 3, "stage": stage,
            "pose_valid": pv, "counts": counts, "passes": passes}


def unstable(a, pose_valid, keep, stage, min_pose=6, min_lm=2):
    """eraseUnstablePosesAndObservations: eraseMissingPoses(6) then eraseObservationsWithMissingPoses(2) while
    observations are removed; counts per id_pose.  -> (pose_valid, keep, stage, passes)"""
    off = a["obs_off"].astype(np.int64)
    obs_pose = a["view_pose"][a["obs_view"].astype(np.int64)].astype(np.int64)
    pv, keep, stage = pose_valid.copy(), keep.copy(), stage.copy()
    n_lm = len(stage)
    lm_of = np.repeat(np.arange(n_lm), np.diff(off))
    passes = 0
    while True:
        passes += 1
        alive = keep & (stage[lm_of] == 3)
        cnt = np.bincount(obs_pose[alive], minlength=len(pv))
        erase = pv & (cnt < min_pose)
        if not erase.any():
            break
        pv &= ~erase
        drop = alive & ~pv[obs_pose]
        keep &= ~drop
        left = np.bincount(lm_of[keep & (stage[lm_of] == 3)], minlength=n_lm)
        stage[(stage == 3) & (left < min_lm)] = 2
        if not drop.any():
            break
    return pv, keep, stage, passes
