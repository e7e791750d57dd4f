"""bench.py's launch contract: `--gpus N` without a
launcher runs N ranks itself (torch.distributed.run, one process per GPU,
rendezvous on 127.0.0.1) and a WORLD_SIZE that disagrees with --gpus fails
loudly.  The ranks of --launch-check join a gloo group and all-reduce on
the CPU, so the spawn path is covered without a GPU."""
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(REPO, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_gpus_2_spawns_two_ranks():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=240, env=_env())
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, p.stdout  # rank 0 only
    rec = json.loads(lines[0])
    assert rec == {"world": 2, "rank_sum": 1.0}


def test_world_size_mismatch_fails_loudly():
    p = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--launch-check"],
                       capture_output=True, text=True, timeout=120,
                       env=_env(WORLD_SIZE="1", RANK="0", LOCAL_RANK="0"))
    assert p.returncode != 0
    assert "WORLD_SIZE" in p.stderr


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", BENCH)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plain_run_options():
    """--full (off by default) gates the CPU baseline and the selection step;
    --dump-outputs names the directory of the last timed step's arrays."""
    b = _bench_module()
    argv = sys.argv
    try:
        sys.argv = ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"]
        a = b.parse()
        assert (a.full, a.dump_outputs, a.steps, a.warmup) == (False, None, 7, 2)
        sys.argv += ["--full", "--dump-outputs", "d"]
        a = b.parse()
        assert (a.full, a.dump_outputs) == (True, "d")
    finally:
        sys.argv = argv
    # --steps K is K timed steps, in one graph up to the cap and in graphs of
    # the cap (one capture, replayed) and one remainder above it
    assert b.graph_chunks(7, 0, 0) == [7] and b.graph_chunks(7, 2, 3) == [2, 3, 2]
    assert b.graph_chunks(200, 0, 0) == [200]
    cap = b.MAX_GRAPH_STEPS
    assert b.graph_chunks(cap, 0, 0) == [cap]
    big = b.graph_chunks(400000, 0, 0)
    assert sum(big) == 400000 and max(big) == cap and len(set(big)) == 2
    assert b.graph_chunks(0, 0, 0) == []


def test_dump_outputs(tmp_path):
    """Every array goes out as <name>.npy in float64 with its values; above
    the byte budget each keeps the same seeded sample of its elements from
    call to call."""
    import numpy as np
    import torch
    b = _bench_module()
    arrays = {"coeffs": torch.arange(240, dtype=torch.float64).reshape(2, 4, 3, 10) / 7,
              "cost": torch.tensor([1.5, float("nan")], dtype=torch.float64),
              "status": torch.tensor([0, -5], dtype=torch.int32)}
    d = tmp_path / "whole"
    b.dump_outputs(str(d), arrays)
    assert sorted(os.listdir(d)) == ["coeffs.npy", "cost.npy", "status.npy"]
    for name, t in arrays.items():
        a = np.load(d / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == tuple(t.shape)
        np.testing.assert_array_equal(a, t.to(torch.float64).numpy())

    budget = b.DUMP_BUDGET_BYTES
    b.DUMP_BUDGET_BYTES = 488  # a quarter of the 244 x 8 bytes
    try:
        b.dump_outputs(str(tmp_path / "s1"), arrays)
        b.dump_outputs(str(tmp_path / "s2"), arrays)
    finally:
        b.DUMP_BUDGET_BYTES = budget
    total = 0
    for name, t in arrays.items():
        s1, s2 = np.load(tmp_path / "s1" / f"{name}.npy"), np.load(tmp_path / "s2" / f"{name}.npy")
        np.testing.assert_array_equal(s1, s2)
        assert s1.ndim == 1 and 1 <= s1.size <= max(1, t.numel() // 4)
        flat = t.to(torch.float64).numpy().ravel()
        assert np.isin(s1[~np.isnan(s1)], flat).all()
        total += s1.nbytes
    assert total <= 488 + 8 * len(arrays)
    assert np.load(tmp_path / "s1" / "coeffs.npy").size == 60


def test_profiled_entry_guard():
    """Committed PMC / SQ entries are used only when their profiled kernel
    time can come from this build: within 15 % of the run's, plus the
    profiler's per-dispatch cost above it."""
    b = _bench_module()
    assert b.same_build_time(0.0057, 0.0046)       # C2 under the kernel trace
    assert not b.same_build_time(0.0080, 0.0046)   # another build
    assert not b.same_build_time(0.0030, 0.0046)
    assert b.same_build_time(7.63, 7.47)           # tube: the slack is negligible
    assert not b.same_build_time(9.0, 7.47)
