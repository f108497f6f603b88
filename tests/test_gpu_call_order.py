"""GPU: what one entry point decides for its query -- counters already cleared, block list and flag mask built by the
shortlist's workgroup, K2 left to K3 -- holds for that call alone.  Whole-query calls, staged calls, a refused call and
the sharded entry points interleaved on ONE context give, bit for bit, what each gives on a fresh map (a second map
created from the same arrays).

Sizes, from launch_hamming_top2 and ctx_match_putative: a query of NQ_SCREENED = 800 rows takes the screened scan
(>= 12 * 64 = 768 rows, unsplit) in slices ((800 - 64) / 2 >= 3 * 64), so the flag mask must be clear beforehand and K2
is left to K3 by the whole-query paths; NQ_EXACT = 500 rows stays below 768 and takes the exact scan.  24 of 40 views of
400 rows are more than half of the map's 250 blocks, which keeps the scan unsplit (split == 1)."""
import numpy as np
import pytest

import sfmlocalization_amd as S
import synthdata as synth
from sfmlocalization_amd import capi

pytestmark = pytest.mark.gpu

KNN = 24            # below the 40 views: the shortlist kernel's chain runs
NQ_SCREENED = 800   # >= 768: screened, sliced scan
NQ_EXACT = 500      # < 768: exact scan
CAP = 4096


class World:
    def __init__(self):
        self.m = synth.make_map(61, n_views=40, desc_per_view=400, views_per_place=10, landmarks_per_place=300,
                                obs_per_view=140)
        rng = np.random.Generator(np.random.PCG64(61))
        place_bow = rng.uniform(0, 1, (len(self.m.place_center), 64)).astype(np.float32)
        self.bow = (place_bow[self.m.view_place] + rng.normal(0, 0.05, (self.m.n_views, 64))).astype(np.float32)
        self.q = {n: synth.make_query(self.m, 610 + n, n_feat=n, n_copies=200, outlier_frac=0.3, place=1)
                  for n in (NQ_SCREENED, NQ_EXACT)}
        self.qbow = {n: (place_bow[q.place] + rng.normal(0, 0.05, 64)).astype(np.float32) for n, q in self.q.items()}
        # the references, each from a fresh map: the shortlist as a host list, the staged calls on it, the whole-query
        # calls with the host list and with the device-resident shortlist
        self.sel, self.staged, self.loc, self.loc_bow = {}, {}, {}, {}
        for n in self.q:
            with self.fresh() as dm:
                self.sel[n] = dm.bow_select(self.qbow[n], KNN)
            with self.fresh() as dm:
                self.staged[n] = staged(dm, self.query(dm, n), self.sel[n])
            with self.fresh() as dm:
                self.loc[n] = whole(dm.localize(self.query(dm, n), self.sel[n]))
            with self.fresh() as dm:
                self.loc_bow[n] = whole(dm.localize_bow(self.query(dm, n), self.qbow[n], KNN))
        assert len(self.sel[NQ_SCREENED]) == KNN and self.loc_bow[NQ_SCREENED][0]

    def fresh(self):
        m = self.m
        return S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(ransac_round=25), view_wh=m.view_wh,
                     kpt_xy=m.kpt_xy, row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X,
                     intrinsic=m.intrinsic, bow=self.bow)

    def query(self, dm, n):
        q = self.q[n]
        return dm.query(q.desc, q.kpt_xy, q.width, q.height)


@pytest.fixture(scope="module")
def world():
    return World()


def raw(x):
    return [np.ascontiguousarray(a).tobytes() for a in x]


def staged(dm, dq, sel):
    """the four staged calls on the map's own context -> putative lists, geometric lists, match set, pose: as bytes"""
    dm.match_putative(dq, sel)
    put = dm.putative_read()
    dm.geometric_filter(dq)
    geo = dm.geometric_read()
    dm.match_set(dq)
    ms = dm.match_set_read()
    dm.resection(dq)
    pose, pq, pl, ii = dm.pose_read()
    assert put[0].sum() > 0 and geo[0].sum() > 0 and len(ms[0]) > 0
    # (the views' counts are filled in by the whole-query calls only)
    return raw(put), raw(geo), raw(ms), [capi.result_fingerprint(pose, pq, pl, view_counts=False)] + raw([ii])


def whole(res):
    pose, pq, pl = res
    return bool(pose.ok), capi.result_fingerprint(pose, pq, pl)


def scan_was_screened(dm):
    """(only the screening kernels count finished pairs: sfmloc_stats_read)"""
    s = dm.stats()
    dm.stats_reset()
    return s.hamming_pairs_finished > 0


@pytest.mark.parametrize("n", [NQ_SCREENED, NQ_EXACT])
def test_bow_query_then_staged_calls_on_the_same_context(world, n):
    with world.fresh() as dm:
        dq = world.query(dm, n)
        assert whole(dm.localize_bow(dq, world.qbow[n], KNN)) == world.loc_bow[n]
        assert scan_was_screened(dm) == (n == NQ_SCREENED)
        assert staged(dm, dq, world.sel[n]) == world.staged[n]
        assert scan_was_screened(dm) == (n == NQ_SCREENED)


@pytest.mark.parametrize("n", [NQ_SCREENED, NQ_EXACT])
def test_staged_calls_then_bow_query_on_the_same_context(world, n):
    with world.fresh() as dm:
        dq = world.query(dm, n)
        assert staged(dm, dq, world.sel[n]) == world.staged[n]
        assert whole(dm.localize_bow(dq, world.qbow[n], KNN)) == world.loc_bow[n]
        assert staged(dm, dq, world.sel[n]) == world.staged[n]


@pytest.mark.parametrize("n", [NQ_SCREENED, NQ_EXACT])
def test_a_refused_query_leaves_nothing_behind(world, n):
    """sfmloc_localize with a view index out of range is refused after the query's reset kernel was queued"""
    bad = np.append(world.sel[n][:5], world.m.n_views).astype(np.uint32)
    with world.fresh() as dm:
        dq = world.query(dm, n)
        for after in ("whole", "staged", "whole"):
            with pytest.raises(S.SfmlocError) as e:
                dm.localize(dq, bad)
            assert e.value.code == capi.EINVAL and "out of range" in e.value.message
            if after == "whole":
                assert whole(dm.localize(dq, world.sel[n])) == world.loc[n]
            else:
                assert staged(dm, dq, world.sel[n]) == world.staged[n]


@pytest.mark.parametrize("first", ["sharded", "plain"])
def test_one_context_alternates_between_the_sharded_and_the_plain_bow_path(world, first):
    """a world of one shard: the context's own keys, its own part, sfmloc_merge_begin -- the pose of sfmloc_localize_bow"""
    import torch
    n = NQ_SCREENED
    with world.fresh() as ref_map:
        pose, pq, pl = ref_map.localize_bow(world.query(ref_map, n), world.qbow[n], KNN)
        ref = (bool(pose.ok), pose.n_inliers, pose.n_matches_2d3d, raw([pq, pl, np.array(pose.P), np.array(pose.center)]))
        assert ref[0]
    keys = torch.zeros(KNN, dtype=torch.int64, device="cuda")
    part = torch.zeros(capi.part_bytes(CAP), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with world.fresh() as dm:
        dq = world.query(dm, n)
        dq.set_bow(world.qbow[n])
        c = dm.context()

        def sharded():
            c.shard_bow_keys(dq, KNN, keys.data_ptr())
            c.shard_begin_bow(dq, keys.data_ptr(), 1, KNN)
            c.shard_export(part.data_ptr(), CAP)
            c.sync()
            c.merge_begin(dq, part.data_ptr(), 1, CAP)
            return c.end()

        def plain():
            c.begin_bow(dq, None, KNN)
            return c.end()

        order = [sharded, plain] if first == "sharded" else [plain, sharded]
        for run in order + order:
            pose, pq, pl = run()
            got = (bool(pose.ok), pose.n_inliers, pose.n_matches_2d3d, raw([pq, pl, np.array(pose.P), np.array(pose.center)]))
            assert got == ref, run.__name__
            assert scan_was_screened(dm)
        c.close()
