"""The calls the two-view refinement tests make on tests/relpose_scene.py: the arguments of capi.RelRefine /
relrefine_np.refine_relative_poses from a set of relative-pose results, and the same call cut down to some pairs or to the
first inliers of one pair."""
import numpy as np


def call_from(args, R, t, inl_off, inl_idx, ok):
    """args: relpose_scene.call_arrays' dict -> the keyword arguments of the refinement, use_pair = ok"""
    call = {k: v for k, v in args.items() if k != "view_wh"}
    call.update(rel_R=np.ascontiguousarray(R, np.float64).reshape(-1, 9), rel_t=np.ascontiguousarray(t, np.float64).reshape(-1, 3),
                inl_off=np.asarray(inl_off, np.uint64), inl_idx=np.asarray(inl_idx, np.uint32),
                use_pair=np.asarray(ok, np.uint8))
    return call


def call_from_twin(args, res):
    """res: relpose_np.relative_poses' list"""
    n = [int(r["n_inliers"]) for r in res]
    idx = [np.asarray(r["inliers"], np.uint32) for r, m in zip(res, n) if m]
    return call_from(args, [np.asarray(r["R"]).reshape(9) if m else np.zeros(9) for r, m in zip(res, n)],
                     [np.asarray(r["t"]).reshape(3) if m else np.zeros(3) for r, m in zip(res, n)],
                     np.concatenate([[0], np.cumsum(n)]), np.concatenate(idx) if idx else np.zeros(0, np.uint32),
                     [int(r["ok"]) for r in res])


def call_from_device(args, rp):
    """rp: capi.RelPoses"""
    return call_from(args, rp.results["R"], rp.results["t"], rp.inl_off, rp.inl_idx, rp.results["ok"])


def sub_call(call, ks, first=None, use=None):
    """the same call restricted to the pairs ks (in that order); first[i] (or None): only that many of pair ks[i]'s
    inliers, from the front of its list; use: use_pair of the new call (default: the pairs' own)"""
    off, ioff = call["offsets"].astype(np.int64), call["inl_off"].astype(np.int64)
    ks = list(ks)
    first = [None] * len(ks) if first is None else list(first)
    n = [int(ioff[k + 1] - ioff[k]) if f is None else int(f) for k, f in zip(ks, first)]
    assert all(m <= ioff[k + 1] - ioff[k] for k, m in zip(ks, n))

    def cat(a, o, cnt, dtype):
        parts = [a[o[k]:o[k] + c] for k, c in zip(ks, cnt)]
        return np.concatenate(parts).astype(dtype) if parts else np.zeros(0, dtype)
    m = [int(off[k + 1] - off[k]) for k in ks]
    out = dict(call)
    out.update(pairs=call["pairs"][ks].reshape(-1, 2), offsets=np.concatenate([[0], np.cumsum(m)]).astype(np.uint64),
               match_i=cat(call["match_i"], off, m, np.uint32), match_j=cat(call["match_j"], off, m, np.uint32),
               rel_R=call["rel_R"][ks].reshape(-1, 9), rel_t=call["rel_t"][ks].reshape(-1, 3),
               inl_off=np.concatenate([[0], np.cumsum(n)]).astype(np.uint64), inl_idx=cat(call["inl_idx"], ioff, n, np.uint32),
               use_pair=np.asarray(call["use_pair"][ks] if use is None else use, np.uint8).reshape(-1))
    return out


def same_bits(dev, ref):
    """dev: RELREFINE_RESULT records; ref: the twin's list -> the (pair, field) that differ"""
    bad = []
    for k, r in enumerate(ref):
        for f in ("status", "n_used", "steps"):
            if int(dev[k][f]) != int(r[f]):
                bad.append((k, f))
        if int(dev[k]["reserved"]) != 0:
            bad.append((k, "reserved"))
        for f in ("R", "t", "E", "cost_initial", "cost"):
            a = np.ascontiguousarray(dev[k][f], np.float64).reshape(-1).view(np.uint64)
            b = np.ascontiguousarray(r[f], np.float64).reshape(-1).view(np.uint64)
            if not np.array_equal(a, b):
                bad.append((k, f))
    return bad
