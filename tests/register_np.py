"""NumPy and oracle restatement of sfmloc_sfm_register (include/sfmloc.h "Growing a map", csrc/register.hip): the count,
the candidates, the compacted per-view lists, the oracle's P3P AC-RANSAC on the undistorted pixels (stream = id_view)
with the oracle's KRt_From_P, the extension of the kept landmarks by structure_np.inliers and structure_np.triangulate
restricted to the selected landmarks.  Every value is the device's bits.  Arrays as adjust.sfm_arrays returns them."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import structure_np as SN  # noqa: E402
from adjust_np import ud_pixel_k3  # noqa: E402
from adjust_scene import p3p_raw, view_lists  # noqa: E402

SEED = SN.SEED


def sub_landmarks(a, sel):
    """the arrays with the landmarks sel alone (ids kept: the sampling stream is the landmark's id) -> (arrays, the
    observation indices they came from)"""
    off = a["obs_off"].astype(np.int64)
    idx = np.concatenate([np.arange(off[l], off[l + 1]) for l in sel]) if len(sel) else np.zeros(0, np.int64)
    out = dict(a)
    out["landmark_id"] = a["landmark_id"][sel]
    out["landmark_X"] = a["landmark_X"][sel]
    out["obs_off"] = np.concatenate([[0], np.cumsum(off[sel + 1] - off[sel])]).astype(np.uint64)
    out["obs_view"] = a["obs_view"][idx]
    out["obs_x"] = a["obs_x"][idx]
    return out, idx


class State:
    """what a handle keeps between rounds and calls"""

    def __init__(self, n_views):
        self.res = [{"ran": False, "ok": False, "n_obs": 0} for _ in range(n_views)]
        self.round = np.full(n_views, -1, np.int64)
        self.last_cnt = np.zeros(n_views, np.int64)
        self.rounds_done = 0


def register(a, pose_valid, pose_R, pose_C, X, obs_keep, landmark_keep, oracle_c, max_rounds=16, min_points=10,
             min_inliers=0, tri_min_inliers=3, tri_allow_pairs=True, residual_px=4.0, seed=SEED, undistort=True,
             max_iteration=4096, state=None):
    """The whole call on copies of the pose table, X and the masks -> dict(report, res [per view: ran, ok, n_obs, and for
    a view that ran p3p_raw's fields, R and center when accepted], round, pose_valid, pose_R, pose_C, X, obs_keep,
    landmark_keep, rounds [per round: tried, registered (view indices), extended, lm_tried, lm_added (landmark
    indices)], state).  undistort=False feeds raw pixels (what sfmloc_sfm_resect's quirk would do): tests only."""
    n_views = len(a["view_id"])
    pv = np.asarray(pose_valid).astype(bool).copy()
    R, C = np.asarray(pose_R, np.float64).reshape(-1, 9).copy(), np.asarray(pose_C, np.float64).reshape(-1, 3).copy()
    X = np.asarray(X, np.float64).copy()
    ok_ = np.asarray(obs_keep).astype(bool).copy()
    lk = np.asarray(landmark_keep).astype(bool).copy()
    off = a["obs_off"].astype(np.int64)
    obs_lm = np.repeat(np.arange(len(a["landmark_id"])), np.diff(off))
    obs_v = a["obs_view"].astype(np.int64)
    vp = a["view_pose"].astype(np.int64)
    lists = view_lists(a)
    st = state if state is not None else State(n_views)
    rep = {"rounds": 0, "views_unposed_in": int((~pv[vp]).sum()), "views_tried": 0, "views_registered": 0,
           "obs_extended": 0, "landmarks_tried": 0, "landmarks_added": 0}
    log = []
    i = 0
    while max_rounds == 0 or i < max_rounds:
        i += 1
        unposed = [v for v in range(n_views) if not pv[vp[v]]]
        clist = {v: lists[v][lk[obs_lm[lists[v]]]] for v in unposed}       # "count", "list"
        todo = [v for v in unposed if len(clist[v]) > min_points and (st.round[v] < 0 or len(clist[v]) > st.last_cnt[v])]
        if not todo:
            break
        assert all(len(clist[v]) <= 65536 for v in todo)
        new = []
        Rn, Cn, pvn = R.copy(), C.copy(), pv.copy()
        for v in todo:                                                     # "resection" on the round's own state
            idx = clist[v]
            st.last_cnt[v] = len(idx)
            K = a["intrinsic"][a["view_intrinsic"][v]]
            px = a["obs_x"][idx]
            if undistort and a["intrinsic_type"][a["view_intrinsic"][v]] == 3:
                px = np.array([ud_pixel_k3(*[float(t) for t in K], float(x), float(y)) for x, y in px]).reshape(-1, 2)
            o = p3p_raw(oracle_c, px, X[obs_lm[idx]], K[0], K[1], K[2], seed, int(a["view_id"][v]), max_iteration)
            r = {"ran": True, "ok": False, "n_obs": len(idx)}
            r.update(o)
            if o["n"] >= 8 and (min_inliers == 0 or o["n"] >= min_inliers):
                _, Rr, _, c = oracle_c.krt_from_p(o["P"])
                r.update(ok=True, R=Rr, center=c)
                pvn[vp[v]], Rn[vp[v]], Cn[vp[v]] = True, Rr.reshape(9), c
                new.append(v)
            st.res[v] = r
            st.round[v] = st.rounds_done
        R, C, pv = Rn, Cn, pvn
        st.rounds_done += 1
        rep["rounds"] += 1
        rep["views_tried"] += len(todo)
        rep["views_registered"] += len(new)
        entry = {"tried": list(todo), "registered": list(new), "extended": 0, "lm_tried": [], "lm_added": []}
        log.append(entry)
        if not new:
            break
        for v in new:                                                      # "extend": X as the round began
            idx = clist[v]
            idx = idx[~ok_[idx]]
            for o in idx:
                inl, _ = SN.inliers(a, R, C, X[obs_lm[o]], np.array([o]), residual_px)
                if inl[0, 0]:
                    ok_[o] = True
                    entry["extended"] += 1
        is_new = np.zeros(n_views, bool)
        is_new[new] = True
        posed = pv[vp[obs_v]]
        sel = np.array([l for l in range(len(lk)) if not lk[l] and is_new[obs_v[off[l]:off[l + 1]]].any()
                        and posed[off[l]:off[l + 1]].sum() >= 2], np.int64)  # "landmarks"
        if len(sel):
            sub, idx = sub_landmarks(a, sel)
            t = SN.triangulate(sub, pv, R, C, SN.ROBUST, tri_min_inliers, bool(tri_allow_pairs), residual_px, seed)
            X[sel] = t["X"]
            lk[sel] = t["landmark_keep"]
            ok_[idx] = t["obs_keep"]
            entry["lm_tried"] = sel.tolist()
            entry["lm_added"] = sel[t["landmark_keep"]].tolist()
        rep["obs_extended"] += entry["extended"]
        rep["landmarks_tried"] += len(entry["lm_tried"])
        rep["landmarks_added"] += len(entry["lm_added"])
    return {"report": rep, "res": st.res, "round": st.round.copy(), "pose_valid": pv, "pose_R": R, "pose_C": C, "X": X,
            "obs_keep": ok_, "landmark_keep": lk, "rounds": log, "state": st}
