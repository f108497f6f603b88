"""GPU: a failed device allocation anywhere in a handle's creation or in a call (injected: sfmloc_debug_fail_next_alloc(k),
the calling thread's k-th allocation from now fails once) returns SFMLOC_ENOMEM, leaves no half-made state behind, and
the same call succeeds afterwards with the result of a call that never failed.  Every case walks k = 0, 1, 2, ... until
the call succeeds; the number of failing k must reach the number of typed buffers (csrc/devmem.h DevBuf) the call
allocates, counted from the code and written here as a literal, so a path that swallows the injected error cannot pass."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)

import adjust_scene as AS  # noqa: E402
import merge_scene as MS  # noqa: E402
from undistort_cameras import CAMERAS  # noqa: E402
from sfmlocalization_amd import capi as S  # noqa: E402

pytestmark = pytest.mark.gpu
MAX_K = 64


def walk(call, at_least, limit=MAX_K):
    """call() with allocation k = 0, 1, ... failing, until it succeeds -> its result then.  Every failure is ENOMEM; at
    least `at_least` values of k fail; more than `limit` iterations is a failure."""
    try:
        for k in range(limit):
            S.debug_fail_next_alloc(k)
            try:
                out = call()
            except S.SfmlocError as e:
                assert e.code == S.ENOMEM, (k, e)
                continue
            print("allocations that failed before the call succeeded:", k, "(at least", at_least, "expected)")
            assert k >= at_least, "only %d allocations failed, the call makes at least %d" % (k, at_least)
            return out
        pytest.fail("still failing after %d injected failures" % limit)
    finally:
        S.debug_fail_next_alloc(-1)


def same(a, b):
    """bit for bit: arrays, or tuples / dicts of them (None and scalars compare equal)"""
    if isinstance(a, dict):
        assert a.keys() == b.keys()
        for k in a:
            same(a[k], b[k])
    elif isinstance(a, (tuple, list)):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            same(x, y)
    elif a is None or b is None:
        assert a is None and b is None
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def test_undistorter_first_image_on_one_handle():
    """ONE handle takes every failed first apply and then the good one; a map pair that came up half would show in its
    output.  The first image allocates the map pair (one group of 2), the source and the target image, and what a call
    completed stays on the handle: k = 0 and k = 1 fail in the group (nothing kept), k = 2 fails at the source image
    after the pair is committed, and the call armed with k = 3 allocates the source and the target only and succeeds: 3"""
    K, dist, _ = CAMERAS[0]
    w, h = 64, 48
    K = K.copy()
    K[:2] *= 0.1                                        # the 640 x 480 camera at a tenth of its size
    img = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    with S.Undistorter(K, dist, w, h) as fresh:
        ref = fresh.apply(img)
    assert ref.size > 0
    with S.Undistorter(K, dist, w, h) as u:
        got = walk(lambda: u.apply(img), 3)
        same(got, ref)
        same(u.apply(img), ref)


def test_akaze_keypoint_regrowth():
    """Akaze.compute with more keypoints than the extractor's per-keypoint arrays hold (65 536 after create) regrows the
    seven of them as one group: 7.  Every failure leaves the old set and its capacity; the same call then gives what a
    fresh extractor gives"""
    rng = np.random.default_rng(9)
    gray = rng.integers(0, 256, (64, 64), dtype=np.uint8)
    n = 65536 + 1
    kin = np.stack([rng.uniform(0, 63, n), rng.uniform(0, 63, n), np.full(n, 4.0), rng.integers(0, 4, n)], 1).astype(np.float32)
    fresh = S.Akaze(64, 64)
    ref = fresh.compute(gray, kin)
    fresh.close()
    ak = S.Akaze(64, 64)
    small = ak.compute(gray, kin[:100])                 # within the capacity: no allocation
    got = walk(lambda: ak.compute(gray, kin), 7)
    same(got, ref)
    same(ak.compute(gray, kin[:100]), small)
    same(small, (ref[0][:100], ref[1][:100]))
    ak.close()


def test_sfm_create_then_clean_and_read():
    """sfmloc_sfm_create uploads 13 arrays and allocates 19 more (adjust.hip sfm_create_impl): 32.  Then it makes the map
    that K5's contexts hang off, without descriptors (capi.hip sfmloc_map_create: the two view tables, the log10 and the
    ratio table: 4) and that map's own context (make_ctx with no bank rows: 26 arrays and the P3P group of 7: 33): 69
    in all.  That is more than the 64 iterations the other walks allow, so this one is bounded by its own count: the
    create armed with k = 69 must be the first that succeeds, which makes 70 iterations"""
    a = AS.two_pass_case()

    def run(h):
        counts = h.clean(rm_unstable=True)
        out = h.read()
        h.close()
        return counts, out

    ref = run(S.Sfm(**a))
    h = walk(lambda: S.Sfm(**a), 69, limit=70)
    got = run(h)
    assert got[0] == ref[0]
    same(got[1], ref[1])


def test_merge_ransac():
    """two uploads and seven arrays (merge.hip ransac_impl): 9"""
    A, B, _, _ = MS.planted(seed=7, n=64, n_in=40)
    ref = S.merge_ransac(A, B, MS.THRES, 256)
    got = walk(lambda: S.merge_ransac(A, B, MS.THRES, 256), 9)
    assert (got["round"], got["count"]) == (ref["round"], ref["count"])
    same(got["M"], ref["M"])
    same(got["inliers"], ref["inliers"])


def test_reduce_points():
    """23 arrays and the partial sums of four scans, one array each at least (reduce.hip reduce_impl): 27.  The
    caller's arrays are written by a call that succeeds only"""
    rng = np.random.default_rng(3)
    X = rng.uniform(-1.0, 1.0, (200, 3))
    X[100:150] = X[:50] + rng.uniform(-0.004, 0.004, (50, 3))
    ref = S.reduce_points(X, thres=0.01, knn=8)
    assert ref["n_absorbed"] > 0
    out = (np.full(200, 7, np.uint32), np.full(200, 7, np.uint32), np.full(200, 7.0))

    def call():
        try:
            return S.reduce_points(X, thres=0.01, knn=8, out=out)
        except S.SfmlocError:
            assert (out[0] == 7).all() and (out[1] == 7).all() and (out[2] == 7.0).all()
            raise

    got = walk(call, 27)
    for k in ("n_keep", "n_absorbed", "n_pairs", "rounds"):
        assert got[k] == ref[k], k
    for k in ("owner", "order", "dist"):
        same(got[k], ref[k])


def test_bowtrainer_kmeans():
    """KmWork (trainbow.hip): 3 + 3 distance and partial-sum arrays and 14 more: 20"""
    x = np.random.default_rng(11).integers(0, 256, (500, 61)).astype(np.float32)
    with S.BowTrainer(61, 500) as tr:
        tr.add_rows(x)
        ref = tr.kmeans(8, attempts=1)
        got = walk(lambda: tr.kmeans(8, attempts=1), 20)
        same(got[0], ref[0])
        same(got[1], ref[1])
        assert got[2] == ref[2]


def _create_walk(create, at_least, limit=MAX_K, start=None):
    """a C create call with allocation k failing -> the handle of the first that succeeds; every failure: ENOMEM, no handle
    and, with `start`, the device's free memory at that figure again (nothing of the refused create is left)"""
    try:
        for k in range(limit):
            h = C.c_void_p()
            S.debug_fail_next_alloc(k)
            rc = create(C.byref(h))
            S.debug_fail_next_alloc(-1)
            if rc == 0:
                assert h.value
                print("allocations that failed before the create succeeded:", k, "(at least", at_least, "expected)")
                assert k >= at_least, "only %d allocations failed, the create makes at least %d" % (k, at_least)
                return h
            assert rc == S.ENOMEM and not h.value, (k, rc, S._L().sfmloc_last_error())
            if start is not None:
                assert free_device_bytes() == start, (k, free_device_bytes() - start)
        pytest.fail("still failing after %d injected failures" % limit)
    finally:
        S.debug_fail_next_alloc(-1)


def free_device_bytes():
    """hipMemGetInfo's free figure, asked of the HIP runtime the library itself is linked to"""
    free, total = C.c_size_t(0), C.c_size_t(0)
    assert S._L().hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def walk_pair_call(call, at_least):
    """walk() for a one-shot call that hands out a handle: every refused call leaves the device's free memory where it was
    before it (measured after one good call, so that what the runtime keeps for itself is there already), which it could
    not with a handle or an array of the failed call still alive; -> (the good call's result, the walked call's)"""
    ref = call()
    start = free_device_bytes()

    def checked():
        try:
            return call()
        except S.SfmlocError:
            assert free_device_bytes() == start
            raise

    got = walk(checked, at_least)
    assert free_device_bytes() == start
    return ref, got


def test_pair_side_calls_leave_nothing_behind():
    """The five one-shot calls of the pair side on pairscales_scene.scene_triplet (three views, three pairs of 40 matches,
    every array non-empty), counted from the code:
    sfmloc_relative_poses    the scene's ten arrays (twoview_device.h PairSceneBufs, view_wh among them), the bearings,
                             the inlier positions, the log10 table and the records: 14
    sfmloc_refine_relative_poses   nine arrays of the scene, five of the poses (PairPosesBufs), the bearings, two point
                             slabs and the records: 18
    sfmloc_wedge_scales      those fourteen, the four per-view lists, twelve arrays of the lists and candidates, two of
                             the choice and six of the order and the ratios (pairscales.hip wscales_device): 38
    sfmloc_tracks_build      7 + 6 + 4 + 3 arrays (tracks.hip tracks_device): 20
    sfmloc_global_poses      eight uploads, nine arrays of the graph and twenty of the two solves (globalposes.hip
                             gposes_device): 37"""
    import pairscales_scene
    s = pairscales_scene.scene_triplet()
    c = s["call"]
    scene = {k: c[k] for k in ("view_off", "kpt_xy", "view_intrinsic", "intrinsics", "intrinsic_type", "pairs", "offsets",
                               "match_i", "match_j")}
    wh = np.tile(np.array([640, 480], np.uint32), (3, 1))
    ref, got = walk_pair_call(lambda: S.RelPoses(view_wh=wh, **scene), 14)
    assert got.results.tobytes() == ref.results.tobytes() and np.array_equal(got.inl_idx, ref.inl_idx)
    assert np.array_equal(got.inl_off, ref.inl_off) and ref.results["ok"].all()
    ref, got = walk_pair_call(lambda: S.RelRefine(**c), 18)
    assert got.results.tobytes() == ref.results.tobytes() and ref.refined.all()
    ref, got = walk_pair_call(lambda: S.WedgeScales(**c), 38)
    assert got.records.tobytes() == ref.records.tobytes() and len(ref.records) == 3
    pl = (c["pairs"], c["offsets"], c["match_i"], c["match_j"])
    ref, got = walk_pair_call(lambda: S.Tracks(c["view_off"], *pl), 20)
    assert got.counts == ref.counts and ref.n_tracks > 0
    same((got.off, got.view, got.feat), (ref.off, ref.view, ref.feat))
    ref, got = walk_pair_call(lambda: S.GlobalPoses(3, s["pairs"], s["rel_R"], s["rel_t"]), 37)
    assert ref.in_component.all()
    same((got.in_component, got.R, got.C, got.pairs), (ref.in_component, ref.R, ref.C, ref.pairs))


def test_akaze_create_leaves_no_handle():
    """sfmloc_akaze_create at 64 x 64: 32 arrays and the seven per-keypoint ones (akaze.hip): 39"""
    L = S._L()
    gray = np.random.default_rng(2).integers(0, 256, (64, 64), dtype=np.uint8)
    gray[16:48, 16:48] //= 4
    fresh = S.Akaze(64, 64)
    ref = fresh.detect_and_compute(gray)
    fresh.close()
    h = _create_walk(lambda out: L.sfmloc_akaze_create(0, 64, 64, 4, 4, C.c_float(0.001), out), 39)
    ak = S.Akaze.__new__(S.Akaze)
    ak._h, ak.width, ak.height = h, 64, 64
    same(ak.detect_and_compute(gray), ref)
    ak.close()


def test_imgbow_create_leaves_no_handle():
    """sfmloc_imgbow_create at 64 x 64 without a PCA: the model's 3 arrays, the extractor's 39, the resize plan's 5 and
    its own 6: 53"""
    L = S._L()
    rng = np.random.default_rng(4)
    centers = rng.uniform(0, 255, (8, 61)).astype(np.float32)
    img = rng.integers(0, 256, (64, 64, 3), dtype=np.uint8)
    fresh = S.ImgBow(64, 64, 3, centers=centers, in_dim=61)
    ref = fresh.compute(img)
    fresh.close()
    d, keep = S._bof_desc(centers, 61)
    h = _create_walk(lambda out: L.sfmloc_imgbow_create(C.byref(d), 0, 64, 64, 3, out), 53)
    ib = S.ImgBow.__new__(S.ImgBow)
    ib._h, ib.width, ib.height, ib.channels = h, 64, 64, 3
    ib.dim = int(L.sfmloc_imgbow_dim(h))
    same(ib.compute(img), ref)
    ib.close()


# ---- the handles a query runs on: sfmloc_map_create, the three context creates, sfmloc_query_create ----

class _QuerySide:
    """Six views of 100 rows (600 rows: nine full 64-row blocks and one of 24, so the padded paths run) with every
    optional array of a map and 4-entry BoW vectors; one query of 150 rows that localises on it.  `ref`: the query's
    fingerprint on a map and a context that no injected failure ever touched, `ref_merged`: the same through one exported
    candidate part and a merge-only context; computed once, never changed."""
    CAP = 4096                                          # candidates a part holds (the query has 150 features)

    def __init__(self):
        import torch
        import synthdata as synth
        self.m = m = synth.make_map(61, n_views=6, desc_per_view=100, views_per_place=6, landmarks_per_place=150,
                                    obs_per_view=90)
        assert m.n_rows == 600
        self.bow = np.random.default_rng(61).uniform(0, 1, (6, 4)).astype(np.float32)
        self.q = synth.make_query(m, 62, n_feat=150, n_copies=110, outlier_frac=0.2)
        self.params = S.default_params(ransac_round=25)
        self.part = torch.zeros(S.part_bytes(self.CAP), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with self.fresh_map() as dm:
            dq = self.query(dm)
            c = dm.context()
            self.ref = self.localise(c, dq)
            pose = dm.localize(dq)[0]
            assert pose.ok and pose.n_inliers >= 10      # the map is small, not degenerate
            assert S.result_fingerprint(*dm.localize(dq)) == self.ref
            mc = dm.context(merge_only=True)
            self.ref_merged = self.localise_merged(c, mc, dq)
            for h in (mc, c, dq):
                h.close()
        print("query-side reference fingerprints:", self.ref.hex(), self.ref_merged.hex())

    def map_arrays(self):
        m = self.m
        return dict(view_id=m.view_id, view_off=m.view_off, desc=m.desc, view_wh=m.view_wh, kpt_xy=m.kpt_xy,
                    row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic,
                    bow=self.bow)

    def fresh_map(self):
        return S.Map(params=self.params, **self.map_arrays())

    def map_desc(self):
        """-> (sfmloc_map_desc of map_arrays(), the arrays it points into), as capi.Map fills it"""
        a = self.map_arrays()
        keep = [np.ascontiguousarray(a["view_id"], np.uint32), np.ascontiguousarray(a["view_off"], np.uint32),
                np.ascontiguousarray(a["desc"], np.uint8).reshape(-1, 64), np.ascontiguousarray(a["view_wh"], np.uint32),
                np.ascontiguousarray(a["kpt_xy"], np.float32), np.ascontiguousarray(a["row_landmark"], np.int32),
                np.ascontiguousarray(a["landmark_id"], np.uint32), np.ascontiguousarray(a["landmark_X"], np.float64),
                np.ascontiguousarray(a["bow"], np.float32)]
        d = S.MapDesc()
        d.n_views, d.n_rows, d.n_landmarks, d.bow_dim = 6, 600, keep[6].shape[0], 4
        d.view_id, d.view_off = S._ptr(keep[0], C.c_uint32), S._ptr(keep[1], C.c_uint32)
        d.desc, d.view_wh = S._ptr(keep[2], C.c_uint8), S._ptr(keep[3], C.c_uint32)
        d.kpt_xy, d.row_landmark = S._ptr(keep[4], C.c_float), S._ptr(keep[5], C.c_int32)
        d.landmark_id, d.landmark_X = S._ptr(keep[6], C.c_uint32), S._ptr(keep[7], C.c_double)
        d.bow = S._ptr(keep[8], C.c_float)
        d.focal, d.ppx, d.ppy = a["intrinsic"][:3]
        return d, keep

    def query(self, dm):
        return dm.query(self.q.desc, self.q.kpt_xy, self.q.width, self.q.height)

    @staticmethod
    def localise(c, dq):
        c.begin(dq)
        return S.result_fingerprint(*c.end())

    def localise_merged(self, c, mc, dq):
        """K1 .. K3 and the candidates on `c`, the merge and the resection on the merge-only context `mc`"""
        c.shard_begin(dq)
        c.shard_export(self.part.data_ptr(), self.CAP)
        c.sync()
        mc.merge_begin(dq, self.part.data_ptr(), 1, self.CAP)
        return S.result_fingerprint(*mc.end())


@pytest.fixture(scope="module")
def query_side():
    return _QuerySide()


def _adopt(cls, m, h):
    """the capi object of a handle that a C create call handed out"""
    o = cls.__new__(cls)
    o._h, o.map = h, m
    m._children.add(o)
    return o


def test_map_create_leaves_nothing_behind(query_side):
    """(Free memory is compared after refusals only: a first localisation on a new stream makes the runtime keep scratch
    memory for its hardware queue, which is no array of the library's.)  sfmloc_map_create with every optional array: the bank and its staging copy, the three view tables, the keypoints,
    the three landmark arrays, the BoW vectors, the log10 and the ratio table (capi.hip map_fill): 12; then the map's own
    context as in test_context_creates_leave_nothing_behind: 44; fifty-six in all: 56"""
    import weakref
    w = query_side
    L = S._L()
    w.fresh_map().close()                               # (what the runtime keeps for itself is there after one good create)
    start = free_device_bytes()
    d, keep = w.map_desc()
    h = _create_walk(lambda out: L.sfmloc_map_create(C.byref(d), C.byref(w.params), out), 56, start=start)
    dm = S.Map.__new__(S.Map)
    dm._h, dm._children, dm.params = h, weakref.WeakSet(), w.params
    dm.view_id, dm.view_off, dm.n_rows, dm.n_views = keep[0], keep[1], 600, 6
    dq = w.query(dm)
    assert S.result_fingerprint(*dm.localize(dq)) == w.ref
    dq.close()
    dm.close()


def test_context_creates_leave_nothing_behind(query_side):
    """make_ctx (capi.hip) on a map with bank rows and BoW vectors: 33 arrays, the P3P group of seven and the four of the
    shortlist: 44, for sfmloc_context_create and for sfmloc_context_create_sharing alike (a borrowed stream changes no
    array).  sfmloc_context_create_merge leaves out the eleven per-bank-row arrays of the matching stages: 33"""
    w = query_side
    L = S._L()
    with w.fresh_map() as dm:
        dq = w.query(dm)
        lead = dm.context()
        for c in (dm.context(), dm.context(share=lead), dm.context(share=lead, merge_only=True)):
            c.close()                                   # one good create / destroy of each kind
        start = free_device_bytes()
        h = _create_walk(lambda out: L.sfmloc_context_create(dm._h, out), 44, start=start)
        plain = _adopt(S.Context, dm, h)
        assert w.localise(plain, dq) == w.ref
        plain.close()
        start = free_device_bytes()                     # (again: see test_map_create_leaves_nothing_behind)
        h = _create_walk(lambda out: L.sfmloc_context_create_sharing(dm._h, lead._h, out), 44, start=start)
        sharing = _adopt(S.Context, dm, h)
        assert w.localise(sharing, dq) == w.ref
        sharing.close()
        start = free_device_bytes()
        h = _create_walk(lambda out: L.sfmloc_context_create_merge(dm._h, lead._h, out), 33, start=start)
        merging = _adopt(S.Context, dm, h)
        assert w.localise_merged(lead, merging, dq) == w.ref_merged
        merging.close()
        lead.close()
        dq.close()


def test_query_create_leaves_nothing_behind(query_side):
    """sfmloc_query_create with keypoints: the descriptors and the keypoints before and after the .feat round trip: 3"""
    w = query_side
    L = S._L()
    desc = np.ascontiguousarray(w.q.desc, np.uint8).reshape(-1, 64)
    kpt = np.ascontiguousarray(w.q.kpt_xy, np.float32).reshape(-1, 2)
    assert desc.shape[0] == 150                         # (not a multiple of 64: the descriptors are padded to 192 rows)
    with w.fresh_map() as dm:
        w.query(dm).close()
        start = free_device_bytes()
        h = _create_walk(lambda out: L.sfmloc_query_create(dm._h, S._ptr(desc, C.c_uint8), S._ptr(kpt, C.c_float), 150,
                                                           w.q.width, w.q.height, out), 3, start=start)
        dq = _adopt(S.Query, dm, h)
        dq.n = 150
        assert S.result_fingerprint(*dm.localize(dq)) == w.ref
        dq.close()


def test_lender_destroyed_before_its_borrower(query_side):
    """A lends its stream to B and is destroyed first: B still localises, bit for bit as a plain context does, and when B
    goes the lender's arrays and stream go with it -- the device's free memory is back where it started.
    (tests/test_gpu_gang.py destroys a lender before its borrowers too, but looks at neither the bits nor the memory.)"""
    w = query_side
    with w.fresh_map() as dm:
        dq = w.query(dm)

        def round_trip():
            a = dm.context()
            b = dm.context(share=a)
            a.close()
            held = free_device_bytes()                  # (the lender is kept while its stream is lent out)
            got = w.localise(b, dq)
            b.close()
            return held, got

        # one good round first: what the runtime keeps for itself from then on (the scratch memory of the hardware queue
        # the lender's stream runs on comes with the first resection there) is in the starting figure
        assert round_trip()[1] == w.ref
        start = free_device_bytes()
        held, got = round_trip()
        assert got == w.ref and held < start
        assert free_device_bytes() == start
        dq.close()
