"""bench.py's host-side pieces on the CPU: the module imports, the CPU-baseline legs (the only place outside tests/ and
smoke() that may use the oracle) run on a small map and report the contract's fields, and the committed evidence
bench.py reads (PMC traffic, the HBM-bound sweep) parses."""
import os

import numpy as np

import bench
import synthdata as synth


def test_cpu_baseline_legs_report_the_contract_fields():
    m = synth.make_map(2, n_views=60, desc_per_view=300, views_per_place=10, landmarks_per_place=200, obs_per_view=90)
    queries = [synth.make_query(m, 1000 + i, n_feat=300) for i in range(2)]
    cb = bench.cpu_baseline(m, queries, 1.0)
    assert cb["unit"] == "queries/s" and cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0
    assert cb["single_core_value"] > 0 and cb["with_per_query_desc_reread_value"] <= cb["value"]
    assert "views" in cb["sample"]
    rng = np.random.Generator(np.random.PCG64(33))
    proto = rng.uniform(0, 1, (len(m.place_center), 500)).astype(np.float32)
    bow = (proto[m.view_place] + rng.normal(0, 0.05, (60, 500))).astype(np.float32)
    qbow = [(proto[q.place] + rng.normal(0, 0.05, 500)).astype(np.float32) for q in queries]
    cs = bench.cpu_baseline_shortlist(m, queries, bow, qbow, 10, 1.0)
    assert cs["unit"] == "queries/s" and cs["value"] > 0 and "shortlist k=10" in cs["sample"]
    assert cs["single_core_value"] > 0 and 0 < cs["with_per_query_bow_and_desc_reread_value"] <= cs["value"]


def test_committed_evidence_parses():
    """The one field bench.py cannot measure in-process (PMC traffic of the roofline kernel) comes from a committed
    summary of separate rocprofv3 --pmc passes; when the file is present it must parse and be plausible for the
    20 M-row bank (1.28 GB read once)."""
    import os
    traffic, src = bench.pmc_traffic(True)
    if os.path.exists(bench.PMC_SUMMARY):
        assert traffic is not None and 1.2e9 < traffic < 2.0e9 and src.startswith("profiles/")
    else:
        assert traffic is None and src is None
    assert bench.pmc_traffic(False) == (None, None)


def test_gpus_flag_is_honoured(monkeypatch):
    """--gpus N without a launcher starts N ranks (a child torch.distributed.run, never an exec from this process);
    under a launcher a rank refuses a world size that differs from --gpus."""
    import subprocess
    import sys
    calls = []
    monkeypatch.setattr(subprocess, "call", lambda cmd, env=None: calls.append(cmd) or 0)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "4", "--steps", "3"])
    assert bench.spawn_ranks(bench.parse(["--gpus", "4", "--steps", "3"])) == 0
    cmd = calls[0]
    assert cmd[1:3] == ["-m", "torch.distributed.run"] and "--nproc-per-node=4" in cmd and cmd[-4:] == ["--gpus", "4", "--steps", "3"]
    assert "127.0.0.1" in cmd
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(bench.__file__), "bench.py"), "--gpus", "4"],
                       env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "WORLD_SIZE=2" in r.stderr


def test_plan_of_a_run():
    """plan(): the default single-GPU shortlist run keeps 20 queries in flight on 4 host threads and asks for a hardware
    queue per context + 2 (the 24-queue limit is why 22 contexts are slower); N ranks run gangs of 32 on 96 contexts per
    slot; --replicas makes every rank a single-GPU run; the image-in leg's defaults are 10 workers, a worker's BoW
    chains on one stream."""
    a = bench.parse([])
    shortlist, forced, sharded, gang, nctx, hwq = bench.plan(a, 1, False)
    assert shortlist and not sharded and gang == 1 and nctx == 20 and a.threads == 4 and hwq == 22
    assert a.image_workers == 10 and a.image_bow_worker_stream and a.image_bow_own_stream
    a = bench.parse(["--gpus", "8"])
    _, _, sharded, gang, nctx, hwq = bench.plan(a, 8, False)
    assert sharded and gang == 32 and nctx == 96 and hwq == 16
    a = bench.parse(["--gpus", "8", "--replicas"])
    _, _, sharded, gang, nctx, _ = bench.plan(a, 8, True)
    assert not sharded and gang == 1 and nctx == 20
    a = bench.parse(["--bow-knn", "0", "--views", "1000"])
    shortlist, _, _, _, nctx, _ = bench.plan(a, 1, False)
    assert not shortlist and nctx == 4


def test_plain_run_and_full_options():
    """A plain run measures the headline only; --full turns the side measurements on, --dump-outputs names a folder."""
    a = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert a.steps == 7 and a.warmup == 2 and not a.full and a.dump_outputs is None
    a = bench.parse(["--full", "--dump-outputs", "out"])
    assert a.full and a.dump_outputs == "out"


def test_dump_outputs_writes_the_last_step(tmp_path):
    """--dump-outputs: one float64 row per query of the last step in step order, the inlier pairs concatenated with
    offsets, the stage timings left out; a step too large for the limit is written as the same seeded sample of rows."""
    from sfmlocalization_amd import capi
    res = {}
    for i in range(8, 16):          # the last step of --steps 2 --batch 8 (queries 8 .. 15) among 5 distinct queries
        p = capi.Pose()
        p.ok, p.n_inliers, p.status, p.nfa = i % 2, i - 7, 3, -1.5 * i
        p.R[:] = [float(i)] * 9
        p.center[:] = [i, -i, 0.5]
        p.stage_seconds[:] = [9.0] * 7
        res[i] = (p, np.arange(i - 7, dtype=np.uint32), np.arange(i - 7, dtype=np.uint32) + 100 * i)
    res[3] = res[8]                 # an earlier query's result is not part of the step
    bench.dump_outputs(str(tmp_path / "d"), res, 8, 8, 5, 300)
    got = {f[:-4]: np.load(tmp_path / "d" / f) for f in os.listdir(tmp_path / "d")}
    assert all(f.endswith(".npy") for f in os.listdir(tmp_path / "d"))
    assert all(v.dtype == np.float64 for v in got.values())
    assert "stage_seconds" not in got
    np.testing.assert_array_equal(got["step_position"], np.arange(8))
    np.testing.assert_array_equal(got["query"], np.arange(8, 16) % 5)
    np.testing.assert_array_equal(got["ok"], np.arange(8, 16) % 2)
    assert got["R"].shape == (8, 3, 3) and got["P"].shape == (8, 3, 4) and got["center"].shape == (8, 3)
    np.testing.assert_array_equal(got["center"][:, 1], -np.arange(8, 16))
    off = got["pair_offsets"].astype(int)
    assert off[0] == 0 and off[-1] == len(got["pair_qfeat"]) == len(got["pair_landmark"]) == sum(range(1, 9))
    np.testing.assert_array_equal(got["pair_landmark"][off[3]:off[4]], np.arange(4) + 100 * 11)
    # a small limit: a seeded sample of the rows, the same on every call
    bench.dump_outputs(str(tmp_path / "s1"), res, 8, 8, 5, 300, limit=3 * 8 * (16 + 300 * 2))
    bench.dump_outputs(str(tmp_path / "s2"), res, 8, 8, 5, 300, limit=3 * 8 * (16 + 300 * 2))
    s1, s2 = np.load(tmp_path / "s1" / "step_position.npy"), np.load(tmp_path / "s2" / "step_position.npy")
    assert 0 < len(s1) < 8 and np.array_equal(s1, s2) and np.all(np.diff(s1) > 0)
