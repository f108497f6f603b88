"""GPU: the BoW view shortlist (K8) on the cases of tests/bow_cases.py, against references computed on the CPU (R1 exact
integers, R2 one float32 subtract and multiply, R3 a float64 band) and against the C oracle bit for bit.

k_bow_topk has two forms: up to 16 384 candidates its distances stay in registers, above that every radix pass re-reads
global memory.  Which sizes run which: candidate counts 2 .. 16 384 (views or a candidate list) the register form;
16 385, 20 000 and 40 000 the global-memory form -- every pattern, the tie runs, R1 at dim 24 and 500, the shard keys,
the chained shortlist and the gang session run both."""
import numpy as np
import pytest

import bow_cases as BC
import sfmlocalization_amd as S
import synthdata as synth
from sfmlocalization_amd import capi
from sfmlocalization_amd import dist as D

pytestmark = pytest.mark.gpu


def open_map(case, **kw):
    _, view_off, desc = BC.map_arrays(case.n)
    return S.Map(BC.map_ids(case.n), view_off, desc, bow=case.bow, **kw)


def tiny_query(dm, seed=0, n=64):
    rng = np.random.Generator(np.random.PCG64(seed))
    return dm.query(rng.integers(0, 256, (n, 64)).astype(np.uint8), rng.uniform(0, 480, (n, 2)).astype(np.float32), 640, 480)


def check_select(oracle_c, dm, case):
    for k, cand in case.picks:
        got = dm.bow_select(case.query, k, cand)
        tag = f"{case.name} k {k} cand {None if cand is None else len(cand)}"
        if case.ref == "R3":
            case.check_r3(got, k, cand)
        else:
            np.testing.assert_array_equal(got, case.expected(k, cand), err_msg=tag)
        np.testing.assert_array_equal(got, oracle_c.bow_select(case.bow, case.query, k, cand), err_msg=tag)


@pytest.mark.parametrize("case", BC.pattern_cases(), ids=repr)
def test_select_distance_patterns(oracle_c, case):
    """uniform at every size and k; shared top 11 / top 22 bits, all equal, zero / subnormal / infinite distances at
    16 384, 16 385 and 40 000 views, the last also through candidate lists of 16 384, 16 385 and 3 views"""
    with open_map(case) as dm:
        np.testing.assert_array_equal(BC.bits_of(dm.bow_distances(case.query)), BC.bits_of(case.dist))
        check_select(oracle_c, dm, case)


@pytest.mark.parametrize("n", BC.SIZES)
def test_select_tie_runs(oracle_c, n):
    """runs of 40 equal distances across a thread's chunk boundary, a wave boundary and at the end of the list, cut by
    every k at the first, a middle and the last element of a run"""
    for case in BC.tie_runs_cases(n):
        with open_map(case) as dm:
            np.testing.assert_array_equal(BC.bits_of(dm.bow_distances(case.query)), BC.bits_of(case.dist))
            check_select(oracle_c, dm, case)


@pytest.mark.parametrize("case", BC.dim_cases(), ids=repr)
def test_select_dimensions(oracle_c, case):
    """dim 1 .. 1 000 (below one wave, at 63 / 64 / 65, two and more rounds per lane): distances equal the oracle's in
    bits for every dim, and R1's exact integers; the selection its reference"""
    with open_map(case) as dm:
        d = dm.bow_distances(case.query)
        exp = np.array([oracle_c.bow_dist(row, case.query) for row in case.bow], np.float32)
        np.testing.assert_array_equal(BC.bits_of(d), BC.bits_of(exp))
        if case.ref == "R1":
            np.testing.assert_array_equal(BC.bits_of(d), BC.bits_of(case.dist_f32))
        check_select(oracle_c, dm, case)


def read_keys(torch, buf):
    return buf.cpu().numpy().view(np.uint64)


def check_keys(got, exp):
    """the shard's best as keys, in view order, then the padding: sorted, they are the reference's"""
    n_real = int((exp != BC.PAD).sum())
    assert (got[n_real:] == BC.PAD).all() and (got[:n_real] != BC.PAD).all()
    np.testing.assert_array_equal(np.sort(got[:n_real]), exp[:n_real])


@pytest.mark.parametrize("case", [BC.tie_runs_case(16385, 1024, 1), BC.pattern_case("edge_values", 16385),
                                  BC.tie_runs_case(40000, 1024, 0), BC.r1_case(24), BC.five_view_case()], ids=repr)
def test_shard_keys(case):
    import torch
    ids = BC.map_ids(case.n)
    with open_map(case) as dm:
        dq, ctx = tiny_query(dm), dm.context()
        buf = torch.zeros(1025, dtype=torch.int64, device="cuda")
        for knn in (1024,) if case.n == 5 else (1, 100, 1024):
            buf.fill_(7)
            ctx.shard_bow_keys(dq, knn, buf.data_ptr(), bow=case.query)
            ctx.sync()
            got = read_keys(torch, buf)
            exp = BC.expected_keys(case, ids, knn)
            np.testing.assert_array_equal(exp[exp != BC.PAD], np.sort(D.bow_key(case.dist_f32, ids))[:knn])
            check_keys(got[:knn], exp)
            assert (got[knn:] == 7).all()                               # nothing written past knn keys
        with pytest.raises(S.SfmlocError) as e:
            ctx.shard_bow_keys(dq, 1025, buf.data_ptr(), bow=case.query)
        assert e.value.code == capi.EINVAL
        knn = 5 if case.n == 5 else 100                                 # the context still works
        ctx.shard_bow_keys(dq, knn, buf.data_ptr(), bow=case.query)
        ctx.sync()
        check_keys(read_keys(torch, buf)[:knn], BC.expected_keys(case, ids, knn))
        ctx.close()
        dq.close()


def merge_map(local_id):
    n = len(local_id)
    return S.Map(local_id, np.arange(n + 1, dtype=np.uint32), np.zeros((n, 64), np.uint8), bow=np.zeros((n, 2), np.float32),
                 **BC.geometry_kwargs(n))


@pytest.mark.parametrize("case", BC.merge_cases(), ids=repr)
def test_merge_select(case):
    """sfmloc_shard_begin_bow on crafted key lists: the context's view list is the brute-force reference's, phantom
    padding included; a shard that owns no winner scans nothing"""
    import torch
    keys = torch.from_numpy(case.keys.view(np.int64)).cuda()
    with merge_map(case.local_id) as dm:
        dq, ctx = tiny_query(dm), dm.context()
        before = dm.stats().hamming_pairs
        ctx.shard_begin_bow(dq, keys.data_ptr(), case.n_parts, case.k, 0 if case.part_stride == case.k else case.part_stride)
        got = ctx.debug_views()
        ctx.sync()
        np.testing.assert_array_equal(got, case.expected())
        moved = dm.stats().hamming_pairs - before
        print(f"{case.name}: hamming_pairs moved by {moved}")
        exp = case.expected()
        owned_blocks = len(np.unique(exp[exp != case.n_views] // 64))          # (one bank row per view, 64-row blocks)
        assert moved == owned_blocks * 64 * dq.n
        if case.n_owned() == 0:
            assert moved == 0
        # the read-back itself: too small a buffer is SFMLOC_ECAP with the count set
        n = capi.C.c_uint32()
        small = np.zeros(1, np.uint32)
        rc = capi._L().sfmloc_debug_context_views(ctx._h, capi._ptr(small, capi.C.c_uint32), 1, capi.C.byref(n))
        assert len(got) > 1 and (rc, n.value) == (capi.ECAP, len(got))
        ctx.close()
        dq.close()


def test_merge_refuses_more_than_its_capacity():
    import torch
    case = BC.merge_cases()[0]
    keys = torch.from_numpy(np.concatenate([case.keys, case.keys[:1]]).view(np.int64)).cuda()      # 9 x 1024
    with merge_map(case.local_id) as dm:
        dq, ctx = tiny_query(dm), dm.context()
        for n_parts, k in ((9, 1024), (1, 1025)):
            with pytest.raises(S.SfmlocError) as e:
                ctx.shard_begin_bow(dq, keys.data_ptr(), n_parts, k)
            assert e.value.code == capi.EINVAL
            ctx.sync()
        ctx.shard_begin_bow(dq, keys.data_ptr(), 8, 1024)               # the context still works
        np.testing.assert_array_equal(ctx.debug_views(), case.expected())
        ctx.sync()
        ctx.close()
        dq.close()


@pytest.fixture(scope="module")
def chain_scene():
    """20 000 views x 40 rows (neighbouring views share 64-row blocks), BoW vectors from place prototypes"""
    m = synth.make_map(35, n_views=20000, desc_per_view=40, views_per_place=20, landmarks_per_place=60, obs_per_view=30)
    rng = np.random.Generator(np.random.PCG64(78))
    proto = rng.uniform(0, 1, (len(m.place_center), 500)).astype(np.float32)
    bow = proto[m.view_place] + rng.normal(0, 0.05, (m.n_views, 500)).astype(np.float32)
    dm = S.Map(m.view_id, m.view_off, m.desc, params=S.default_params(ransac_round=25), view_wh=m.view_wh, kpt_xy=m.kpt_xy,
               row_landmark=m.row_landmark, landmark_id=m.landmark_id, landmark_X=m.landmark_X, intrinsic=m.intrinsic, bow=bow)
    qs = []
    for trial in range(4):
        q = synth.make_query(m, 500 + trial, n_feat=800, place=37 * trial + 5)
        qb = (proto[q.place] + rng.normal(0, 0.05, 500)).astype(np.float32)
        dq = dm.query(q.desc, q.kpt_xy, q.width, q.height)
        dq.set_bow(qb)
        qs.append((dq, qb))
    cand = np.sort(rng.choice(m.n_views, BC.REG_LIMIT + 1, replace=False)).astype(np.uint32)
    yield dm, bow, qs, cand
    for dq, _ in qs:
        dq.close()
    dm.close()


def same_result(got, ref, tag):
    assert got[0].ok == ref[0].ok and got[0].n_inliers == ref[0].n_inliers, tag
    assert got[0].n_putative_views == ref[0].n_putative_views and got[0].n_matches_2d3d == ref[0].n_matches_2d3d, tag
    np.testing.assert_array_equal(got[1], ref[1], err_msg=tag)
    np.testing.assert_array_equal(got[2], ref[2], err_msg=tag)
    np.testing.assert_array_equal(np.array(got[0].P).view(np.uint64), np.array(ref[0].P).view(np.uint64), err_msg=tag)


def test_chain_selection_is_the_oracles(oracle_c, chain_scene):
    """sfmloc_localize_bow_begin over 20 000 views and over 16 385 candidates (the global-memory form both times), knn
    100 .. 3 000 (the block list of more than 1 024 views): the selection the context worked on is the oracle's, and
    pose, inliers and pairs are those of sfmloc_bow_select + sfmloc_localize_begin, bit for bit"""
    dm, bow, qs, cand16385 = chain_scene
    ctx = dm.context()
    n_ok = n_runs = 0
    for knn in (100, 1024, 1025, 3000):
        for cand in (None, cand16385):
            dq, qb = qs[n_runs % len(qs)]
            tag = f"knn {knn} cand {None if cand is None else len(cand)}"
            exp = oracle_c.bow_select(bow, qb, knn, cand)
            ctx.begin_bow(dq, qb, knn, cand)
            np.testing.assert_array_equal(ctx.debug_views(), exp, err_msg=tag)
            got = ctx.end()
            sel = dm.bow_select(qb, knn, cand)
            np.testing.assert_array_equal(sel, exp, err_msg=tag)
            ctx.begin(dq, sel)
            np.testing.assert_array_equal(ctx.debug_views(), exp, err_msg=tag)
            same_result(got, ctx.end(), tag)
            n_ok += int(got[0].ok)
            n_runs += 1
    ctx.close()
    assert n_runs == 8 and n_ok >= 4, n_ok          # the comparison is not between two failures


def test_gang_keys_and_session(oracle_c, chain_scene):
    """sfmloc_shard_batch_bow_keys with a gang of 2 contexts and 3 queries on 40 000 views: the single calls' keys, and
    the reference's; one gang session through sfmloc_localize_bow_begin: every member's selection is the oracle's"""
    import torch
    case = BC.r1_case(24)
    ids = BC.map_ids(case.n)
    rng = np.random.Generator(np.random.PCG64(79))
    cases = [case] + [BC.Case(f"{case.name}-q{i}", "R1", case.bow, rng.integers(0, 4, case.dim), []) for i in (1, 2)]
    with open_map(case) as dm:
        ctxs = [dm.context(), dm.context()]
        dqs = [tiny_query(dm, seed=i) for i in range(3)]
        for dq, c in zip(dqs, cases):
            dq.set_bow(c.query)
        for knn in (100, 1024):
            batch = torch.zeros((3, knn), dtype=torch.int64, device="cuda")
            single = torch.zeros((3, knn), dtype=torch.int64, device="cuda")
            capi.shard_batch_bow_keys(ctxs, 2, dqs, knn, batch.data_ptr())
            for c in ctxs:
                c.sync()
            for i, dq in enumerate(dqs):
                ctxs[0].shard_bow_keys(dq, knn, single.data_ptr() + i * knn * 8)
            ctxs[0].sync()
            got, one = read_keys(torch, batch), read_keys(torch, single)
            np.testing.assert_array_equal(got, one)
            for i, c in enumerate(cases):
                check_keys(got[i], BC.expected_keys(c, ids, knn))
        for o in ctxs + dqs:
            o.close()
    dm, bow, qs, cand = chain_scene
    ctxs = [dm.context(), dm.context()]
    for knn in (100, 1025):
        exp = [oracle_c.bow_select(bow, qb, knn) for _, qb in qs[:2]]
        with capi.gang(ctxs):
            for c, (dq, _) in zip(ctxs, qs):
                c.begin_bow(dq, None, knn)
        in_gang = [(c.debug_views(), c.end()) for c in ctxs]
        for c, (dq, _), e, (views, res) in zip(ctxs, qs, exp, in_gang):
            np.testing.assert_array_equal(views, e)
            c.begin_bow(dq, None, knn)                                   # single flight
            np.testing.assert_array_equal(c.debug_views(), e)
            same_result(res, c.end(), f"gang knn {knn}")
    for c in ctxs:
        c.close()
