"""GPU: one process works on device 0 and then on device 1 -- the kernels that ask for more dynamic LDS than the default
limit of a launch (K1, K3's fast form, K5's round, the gang forms of a session, the sharded shortlist's k_bow_merge_select,
AKAZE's k_suppress and k_octave_resident) have that limit raised per kernel AND per device (csrc/devmem.h "Dynamic-LDS
limits"), so the second device's launches must succeed in a process whose first device has already raised them, and
give the first device's results bit for bit.  One child process, so that no other test's launches have been made in it;
skipped where fewer than two devices are visible."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN, CAP = 20, 4096


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def answer(res):
    pose, pq, pl = res
    return {"ok": bool(pose.ok), "n_inliers": int(pose.n_inliers), "n_matches_2d3d": int(pose.n_matches_2d3d),
            "bits": digest(pq, pl, np.array(pose.P, np.float64), np.array(pose.center, np.float64))}


def on_device(device):
    """every call raises unless it answers SFMLOC_OK"""
    import torch
    import sfmlocalization_amd as S
    import synthdata as synth
    from sfmlocalization_amd import capi
    m = synth.make_map(1, n_views=50, desc_per_view=400, views_per_place=10, landmarks_per_place=300, obs_per_view=120)
    qs = [synth.make_query(m, 2 + k, n_feat=500, n_copies=150) for k in range(2)]
    rng = np.random.Generator(np.random.PCG64(5))
    place_bow = rng.uniform(0, 1, (len(m.place_center), 64)).astype(np.float32)
    bow = (place_bow[m.view_place] + rng.normal(0, 0.05, (m.n_views, 64))).astype(np.float32)
    out = {}
    dev = torch.device("cuda", device)
    keys = torch.zeros(KNN, dtype=torch.int64, device=dev)
    part = torch.zeros(capi.part_bytes(CAP), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(ransac_round=25, device=device), view_wh=m.view_wh,
               kpt_xy=m.kpt_xy, row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X,
               intrinsic=m.intrinsic, bow=bow) as dm:
        assert dm.info()["device"] == device
        dqs = [dm.query(q.desc, q.kpt_xy, q.width, q.height) for q in qs]
        for dq, q in zip(dqs, qs):
            dq.set_bow(place_bow[q.place])
        # the whole path on all views: K1, K3's fast form, K5's rounds
        out["localize"] = answer(dm.localize(dqs[0]))
        out["match_lists"] = digest(*dm.putative_read())
        # a gang session of two contexts
        ctxs = [dm.context(), dm.context()]
        with capi.gang(ctxs):
            for c, dq in zip(ctxs, dqs):
                c.begin_bow(dq, None, KNN)
        out["gang"] = [answer(c.end()) for c in ctxs]
        launches, ganged = capi.gang_counters(ctxs[0])
        assert ganged > 0, "the session issued no gang launch"
        # the sharded shortlist of a world of one shard: its keys, the merge (k_bow_merge_select), its part, the pose
        c = ctxs[0]
        c.shard_bow_keys(dqs[0], KNN, keys.data_ptr())
        c.shard_begin_bow(dqs[0], keys.data_ptr(), 1, KNN)
        c.shard_export(part.data_ptr(), CAP)
        c.sync()
        c.merge_begin(dqs[0], part.data_ptr(), 1, CAP)
        out["sharded"] = answer(c.end())
        out["sharded_views"] = digest(c.debug_views())
        for c in ctxs:
            c.close()
        for dq in dqs:
            dq.close()
    ak = S.Akaze(640, 480, device=device)
    kp, desc = ak.detect_and_compute(synth.texture_image(1, 480, 640))
    ak.close()
    out["akaze"] = {"n": int(len(kp)), "bits": digest(kp, desc)}
    return out


@pytest.mark.gpu
def test_second_device_in_one_process_equals_the_first():
    import sfmlocalization_amd as S
    if S.device_count() < 2:
        pytest.skip("needs two HIP devices")
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    first, second = json.loads(r.stdout.strip().splitlines()[-1])
    assert first["localize"]["ok"] and first["sharded"]["ok"] and all(g["ok"] for g in first["gang"])
    assert first["akaze"]["n"] > 10
    for what in first:
        assert second[what] == first[what], what


if __name__ == "__main__":
    sys.path[:0] = [ROOT]
    print(json.dumps([on_device(0), on_device(1)]))
