"""bench.py's host logic, no GPU: presets and the metric's config, the sharding of reads over ranks (weak for C2 / C3,
strong for C4), the index cache (built once on the host, path cover included, loaded by the other ranks), and the command
the parent of `bench.py --gpus N` starts its ranks with."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_presets_and_sharding():
    b = _bench()
    a = b.parse([])
    assert (a.genome, a.reads, a.read_len, a.k, a.find, a.scaling, a.gpus) == (5_000_000, 1_000_000, 150, 31, False, "weak", 1)
    a = b.parse(["--config", "C3"])
    assert (a.genome, a.reads, a.find, a.scaling) == (100_000_000, 10_000_000, True, "weak")
    a = b.parse(["--config", "C4", "--gpus", "8"])
    assert (a.genome, a.reads, a.find, a.scaling) == (250_000_000, 100_000_000, False, "strong")
    for world in (1, 2, 3, 4, 8):  # strong scaling: the shards tile the 100 M reads exactly
        parts = [b.shard(a, r, world) for r in range(world)]
        assert sum(n for n, _ in parts) == a.reads
        assert all(parts[r][1] == sum(n for n, _ in parts[:r]) for r in range(world))
    a = b.parse(["--gpus", "4"])
    assert [b.shard(a, r, 4) for r in range(4)] == [(1_000_000, r * 1_000_000) for r in range(4)]  # weak: fixed per rank
    # the launch the driver makes on an 8-GPU node, at the size tests/test_gpu_bench.py runs it with fewer ranks: contiguous shards of
    # ceil(reads / 8), the last one short
    a = b.parse(["--config", "C4", "--gpus", "8", "--genome", "300000", "--reads", "240003"])
    assert [b.shard(a, r, 8) for r in range(8)] == [(30001, r * 30001) for r in range(7)] + [(29996, 7 * 30001)]


def test_steps_is_the_number_of_timed_steps():
    b = _bench()
    assert b.parse([]).steps == 200 and b.parse(["--steps", "7"]).steps == 7
    assert b.parse(["--config", "C5"]).steps == 3
    for n in ("200", "1", "9"):  # (an explicit count is kept, the default's value included)
        assert b.parse(["--config", "C5", "--steps", n]).steps == int(n)
    try:
        b.parse(["--steps", "0"])
        raise AssertionError("--steps 0 accepted")
    except SystemExit:
        pass


def test_full_is_off_by_default():
    b = _bench()
    assert b.parse([]).full is False and b.parse(["--steps", "20", "--warmup", "5"]).full is False
    assert b.parse(["--full"]).full is True and b.parse(["--config", "C3", "--full"]).full is True


def test_a_run_reads_no_index_file_an_earlier_run_left(tmp_path, monkeypatch):
    """without --index-cache a run builds its index: a file under the cache's name is neither read nor written by one process; the
    parent of --gpus N (share) builds afresh too and leaves the file for its own ranks"""
    b = _bench()
    monkeypatch.setenv("KBO_BENCH_CACHE_DIR", str(tmp_path))
    monkeypatch.delenv("KBO_BENCH_NO_CACHE", raising=False)
    a = b.parse(["--genome", "50000", "--reads", "500"])
    other = b.parse(["--genome", "60000", "--reads", "500", "--index-cache", b.cache_path(a)])
    b.build_or_load_index(other, 2)                  # an earlier run's file, of another index, under this run's cache name
    before = os.stat(b.cache_path(a)).st_mtime_ns
    _, s = b.build_or_load_index(a, 2)
    assert s.n_sets() == 50_001 and os.stat(b.cache_path(a)).st_mtime_ns == before
    _, s = b.build_or_load_index(a, 2, share=True)
    assert s.n_sets() == 50_001
    _, s2 = b.build_or_load_index(a, 2, may_build=False)  # a rank of the same run
    assert s2.n_sets() == 50_001


def test_dump_outputs_types_budget_and_sample(tmp_path):
    b = _bench()
    rng = np.random.default_rng(1)
    chars = rng.integers(0, 256, 3_000_000, dtype=np.uint8)
    recs = rng.integers(0, 2**32, (1000, 7), dtype=np.uint64).astype(np.uint32)
    ms = rng.integers(0, 64, 5000, dtype=np.uint8)
    budget = 4 << 20
    info = b.dump_outputs(str(tmp_path / "a"), {"chars": chars, "run_records": recs, "ms": ms}, budget=budget)
    got = {n: np.load(str(tmp_path / "a" / (n + ".npy"))) for n in ("chars", "run_records", "ms")}
    # narrow values as float32, 32-bit ones as float64, every value exact
    assert got["chars"].dtype == np.float32 and got["ms"].dtype == np.float32 and got["run_records"].dtype == np.float64
    assert np.array_equal(got["run_records"], recs) and np.array_equal(got["ms"], ms)
    assert not info["arrays"]["ms"]["sampled"] and not (tmp_path / "a" / "ms_rows.npy").exists()
    # the larger output: a sample of its rows, ascending, named by <name>_rows.npy, within the budget
    rows = np.load(str(tmp_path / "a" / "chars_rows.npy"))
    assert info["arrays"]["chars"]["sampled"] and info["arrays"]["chars"]["rows_of"] == len(chars)
    assert rows.dtype == np.float64 and len(rows) == len(got["chars"]) > 100_000 and (np.diff(rows) > 0).all()
    assert np.array_equal(got["chars"], chars[rows.astype(np.int64)])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= budget + 4096
    # the same rows in every run; the default budget stays within 64 MB
    b.dump_outputs(str(tmp_path / "b"), {"chars": chars, "run_records": recs, "ms": ms}, budget=budget)
    assert np.array_equal(np.load(str(tmp_path / "b" / "chars_rows.npy")), rows)
    assert b.DUMP_BYTES + 64 * 1024 <= 64_000_000


def test_index_cache_round_trip_and_spawn_command(tmp_path):
    b = _bench()
    cache = str(tmp_path / "idx.kbohip")
    argv = ["--gpus", "2", "--genome", "60000", "--reads", "500", "--index-cache", cache]
    a = b.parse(argv)
    g1, s1 = b.build_or_load_index(a, 2)            # builds and writes the cache (with the path cover)
    assert os.path.exists(cache) and s1.n_sets() == 60_001
    g2, s2 = b.build_or_load_index(a, 2, may_build=False)  # what the other ranks do
    assert np.array_equal(g1, g2)
    p1, p2 = s1.export_parts(), s2.export_parts()
    assert all((x == y).all() for x, y in zip(p1[0], p2[0])) and p1[1] == p2[1] and (p1[2] == p2[2]).all()
    assert all((x == y).all() for x, y in zip(s1.path_cover(), s2.path_cover()))
    cmd = b.spawn_command(a, argv, 29512)
    assert cmd[:3] == [sys.executable, "-m", "torch.distributed.run"] and "--nproc-per-node=2" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29512"
    assert cmd[-len(argv):] == argv                 # (the cache is already named: nothing appended)
    a2 = b.parse(["--gpus", "2"])
    cmd2 = b.spawn_command(a2, ["--gpus", "2"], 1)
    assert cmd2[-2] == "--index-cache" and cmd2[-1].endswith("kbo_bench_iid_5000000_k31.kbohip")
