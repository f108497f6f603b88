"""Writes tests/golden/relpose/expected.json: the five-point samples the relative-pose tests solve, and the bounds of
their numeric comparisons.  Run from the repository root: python tests/golden/make_relpose_fixtures.py

Nobody has measured what two different elimination and root-finding routes may differ by, so the bounds are not
invented: the independent solver (tests/relpose_independent.py: SVD null space, action matrix, numpy.linalg.eig) runs on
each sample, then again with each of the 20 inputs moved by one ulp up and down, and the largest change of a model (sign
and norm aligned, max-norm) is the problem's own conditioning `cond`.  The bound is 1000 x cond: three decades for the
two routes, while a wrong model is O(1) away.  Samples are drawn from a seeded generator and kept only when the
independent solver's models are separated from each other by more than that bound (asserted below), so that "matches
one of its models" names one model.  One more sample repeats a point: it must give no model at all.

Pose against truth, per scene pair that has a baseline and ends ok: the restatement's winning sample[5] is solved by the
independent solver, its model nearest the planted E decomposed by numpy.linalg.svd, and the candidate nearest the planted
(R, t) compared with them: ref_dR, ref_dt, the error the sample's noise alone puts into a correct solver.  The device
(the restatement's bits) must be within ref_dR + 1000 x cond_R of the planted R, likewise t, cond_R and cond_t being the
change of that candidate under the same one-ulp perturbations of the sample.

The decomposition is bounded the same way: the planted E of every solver sample is decomposed by numpy.linalg.svd, again
with each of its nine entries moved by one ulp up and down; decompose_cond is the largest change of a candidate (max-norm
of R plus max-norm of t, a candidate matched with its nearest one) and decompose_bound 1000 x that.

The measured distances of the restatement are written beside each bound (twin_dist, twin_dR, twin_dt) for the record;
no bound is derived from them."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
sys.path.insert(0, TESTS)
sys.path.insert(0, os.path.dirname(TESTS))

import relpose_independent as ind  # noqa: E402
import relpose_np as twin  # noqa: E402
import relpose_scene as scene_mod  # noqa: E402

N_SAMPLES = 10
FACTOR = 1000.0


def _rot(w):
    return scene_mod._rot(w)


def _perturbed(x1, x2):
    base = np.concatenate([x1.ravel(), x2.ravel()])
    for i in range(20):
        for d in (-np.inf, np.inf):
            p = base.copy()
            p[i] = np.nextafter(p[i], d)
            yield p[:10].reshape(5, 2), p[10:].reshape(5, 2)


def solver_cond(x1, x2, ref):
    """the largest change of any model of `ref` when an input moves by one ulp"""
    c = 0.0
    for a, b in _perturbed(x1, x2):
        m = ind.five_point(a, b)
        for e in ref:
            c = max(c, ind.align_distance(e, m))
    return c


def separation(models):
    s = np.inf
    for i in range(len(models)):
        for j in range(i + 1, len(models)):
            s = min(s, ind.align_distance(models[i], models[j:j + 1]))
    return s


def pose_distance(Ra, ta, Rb, tb):
    return float(np.abs(np.asarray(Ra).reshape(3, 3) - Rb).max() + np.abs(np.asarray(ta) - tb).max())


def decomposition_cond(E):
    """the largest change of any of the four candidates of the independent decomposition (numpy.linalg.svd) when an entry
    of E moves by one ulp; a candidate is matched with its nearest one"""
    ref = ind.decompose(E)
    c = 0.0
    for i in range(9):
        for d in (-np.inf, np.inf):
            p = np.array(E, np.float64)
            p[i] = np.nextafter(p[i], d)
            cand = ind.decompose(p)
            for R, t in ref:
                c = max(c, min(pose_distance(Rc, tc, R, t) for Rc, tc in cand))
    return c


def essential_of(R, t):
    E = np.array([[0, -t[2], t[1]], [t[2], 0, -t[0]], [-t[1], t[0], 0]]) @ R
    return (E / np.linalg.norm(E)).ravel()


def nearest_pose(E, R, t):
    """the candidate of the independent decomposition of E nearest the planted (R, t) -> (R, t)"""
    best = None
    for Rc, tc in ind.decompose(E):
        d = np.abs(Rc - R).max() + np.abs(tc - t).max()
        if best is None or d < best[0]:
            best = (d, Rc, tc)
    return best[1], best[2]


def solver_samples():
    rng = np.random.Generator(np.random.PCG64(77))
    out = []
    while len(out) < N_SAMPLES:
        R = _rot(rng.normal(size=3) * 0.2)
        t = rng.normal(size=3)
        t /= np.linalg.norm(t)
        X = rng.uniform(-1, 1, (5, 3)) + [0, 0, 4]
        Y = X @ R.T + t
        x1, x2 = X[:, :2] / X[:, 2:], Y[:, :2] / Y[:, 2:]
        ref = ind.five_point(x1, x2)
        cond = solver_cond(x1, x2, ref)
        bound = FACTOR * cond
        if len(ref) == 0 or not separation(ref) > bound:      # (kept by the separation of the independent roots alone)
            continue
        assert separation(ref) > bound
        nm, E = twin.five_point(x1[None], x2[None])
        Ep = essential_of(R, t)
        dcond = decomposition_cond(Ep)
        R4, t4 = twin.decompose(Ep)
        dref = ind.decompose(Ep)
        out.append({"decompose_cond": dcond, "decompose_bound": FACTOR * dcond,
                    "twin_decompose_dist": max(min(pose_distance(R4[c], t4[c], Rr, tr) for Rr, tr in dref)
                                               for c in range(4)),
                    "x1": x1.ravel().tolist(), "x2": x2.ravel().tolist(), "E_planted": Ep.tolist(), "n_ref": len(ref),
                    "cond": cond, "bound": bound, "separation": separation(ref),
                    "planted_dist_ref": ind.align_distance(Ep, ref),
                    "twin_n": int(nm[0]),
                    "twin_dist": max([ind.align_distance(E[0, k], ref) for k in range(nm[0])] + [0.0]),
                    "twin_planted_dist": ind.align_distance(Ep, E[0, :nm[0]])})
    rep = dict(out[0])
    x1, x2 = np.array(rep["x1"]).reshape(5, 2), np.array(rep["x2"]).reshape(5, 2)
    x1[3], x2[3] = x1[1], x2[1]
    out.append({"x1": x1.ravel().tolist(), "x2": x2.ravel().tolist(), "E_planted": None, "n_ref": 0, "cond": 0.0,
                "bound": 0.0, "separation": 0.0, "planted_dist_ref": 0.0,
                "twin_n": int(twin.five_point(x1[None], x2[None])[0][0]), "twin_dist": 0.0, "twin_planted_dist": 0.0,
                "repeated_point": True})
    return out


def pose_bounds():
    sc = scene_mod.make_scene()
    args, names = scene_mod.call_arrays(sc)
    res = twin.relative_poses(**args)
    kpt = np.asarray(args["kpt_xy"], np.float32)
    off = args["offsets"].astype(np.int64)
    voff = args["view_off"].astype(np.int64)
    out = {}
    for k, (name, r) in enumerate(zip(names, res)):
        vi, vj = int(args["pairs"][k][0]), int(args["pairs"][k][1])
        R, t = scene_mod.planted_pose(sc, vi, vj)
        if not r["ok"] or np.abs(t).max() == 0.0:
            continue
        bi = twin.bearings(kpt[voff[vi]:voff[vi + 1]], args["intrinsics"][args["view_intrinsic"][vi]],
                           args["intrinsic_type"][args["view_intrinsic"][vi]])
        bj = twin.bearings(kpt[voff[vj]:voff[vj + 1]], args["intrinsics"][args["view_intrinsic"][vj]],
                           args["intrinsic_type"][args["view_intrinsic"][vj]])
        smp = np.asarray(r["sample"], np.int64)
        x1 = bi[args["match_i"][off[k]:off[k + 1]].astype(np.int64)[smp]]
        x2 = bj[args["match_j"][off[k]:off[k + 1]].astype(np.int64)[smp]]
        Ep = essential_of(R, t)

        def pose_of(a, b):
            m = ind.five_point(a, b)
            e = min(m, key=lambda q: ind.align_distance(Ep, q[None]))
            return nearest_pose(e, R, t)
        Rr, tr = pose_of(x1, x2)
        cR = ct = 0.0
        for a, b in _perturbed(x1, x2):
            Rp, tp = pose_of(a, b)
            cR, ct = max(cR, np.abs(Rp - Rr).max()), max(ct, np.abs(tp - tr).max())
        ref_dR, ref_dt = float(np.abs(Rr - R).max()), float(np.abs(tr - t).max())
        out[name] = {"sample": smp.tolist(), "ref_dR": ref_dR, "ref_dt": ref_dt, "cond_R": cR, "cond_t": ct,
                     "bound_R": ref_dR + FACTOR * cR, "bound_t": ref_dt + FACTOR * ct,
                     "twin_dR": float(np.abs(r["R"].reshape(3, 3) - R).max()), "twin_dt": float(np.abs(r["t"] - t).max())}
    return out


def main():
    doc = {"factor": FACTOR, "solver": solver_samples(), "pose": pose_bounds()}
    os.makedirs(os.path.join(HERE, "relpose"), exist_ok=True)
    with open(os.path.join(HERE, "relpose", "expected.json"), "w") as fh:
        json.dump(doc, fh, indent=1)
    for s in doc["solver"]:
        print("solver: n_ref %d twin_n %d cond %.2e bound %.2e twin_dist %.2e planted(ref) %.2e planted(twin) %.2e | "
              "decompose cond %.2e bound %.2e twin %.2e" % (
                  s["n_ref"], s["twin_n"], s["cond"], s["bound"], s["twin_dist"], s["planted_dist_ref"],
                  s["twin_planted_dist"], s.get("decompose_cond", 0.0), s.get("decompose_bound", 0.0),
                  s.get("twin_decompose_dist", 0.0)))
    for n, p in doc["pose"].items():
        print("pose %s: ref_dR %.2e twin_dR %.2e bound_R %.2e | ref_dt %.2e twin_dt %.2e bound_t %.2e" % (
            n, p["ref_dR"], p["twin_dR"], p["bound_R"], p["ref_dt"], p["twin_dt"], p["bound_t"]))


if __name__ == "__main__":
    main()
