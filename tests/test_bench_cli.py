"""bench.py contract on the CPU: ``--gpus N`` without a torchrun environment launches N ranks as a
child torch.distributed.run job and prints ONE JSON line with n_gpus = N (the driver's scaling
runs rely on this)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench_small(tmp_path, tag, *extra, cwd=None, env_extra=None):
    """A 2-client tiny-BERT bench run on the CPU (1 warm-up + 2 timed rounds); returns the record.
    ``cwd``: run from there and leave ``--out`` to the bench."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "2"
    env.update(env_extra or {})
    out = [] if cwd is not None else ["--out", str(tmp_path / f"run_{tag}")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu",
                        "--gpus", "1", "--model", "tiny-bert", "--clients", "2", "--steps", "2",
                        "--warmup", "1", "--no-ckpt", "--batch-size", "16",
                        "--set", "train_samples=32", "--set", "global_test_samples=32",
                        *out, *extra],
                       cwd=str(cwd or tmp_path), env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_bench_runs_where_the_working_directory_cannot_hold_runs(tmp_path):
    """Without ``--out`` the run's files go to ``runs/bench/n<N>`` under the working directory; where
    that cannot be made (here ``runs`` is a file; elsewhere a tree the user may not write) the bench
    falls back to the same layout under the temporary directory instead of failing."""
    cwd, tmp = tmp_path / "cwd", tmp_path / "tmp"
    cwd.mkdir()
    tmp.mkdir()
    (cwd / "runs").write_text("not a directory")
    d = _bench_small(tmp_path, "blocked", cwd=cwd, env_extra={"TMPDIR": str(tmp)})
    assert d["steps"] == 2 and d["value"] > 0 and d["ledger"]["height"] > 0
    found = [os.path.join(p, f) for p, _, fs in os.walk(tmp) for f in fs if f == "ledger.jsonl"]
    assert len(found) == 1 and found[0].endswith(os.path.join("runs", "bench", "n1", "ledger.jsonl"))
    assert (cwd / "runs").read_text() == "not a directory" and os.listdir(cwd) == ["runs"]
    # a writable working directory keeps the documented place
    d = _bench_small(tmp_path, "plain", cwd=tmp_path / "tmp")
    assert d["value"] > 0 and os.path.exists(tmp / "runs" / "bench" / "n1" / "ledger.jsonl")


def test_bench_dump_outputs_repeatable_and_full(tmp_path):
    """``--dump-outputs``: float arrays of what the last timed round computed, identical between
    two runs with the same arguments (same inputs); ``--steps`` sets the timed rounds and
    ``ms_per_step`` is one of them in milliseconds; ``--full`` runs to the same result line."""
    import numpy as np
    a = _bench_small(tmp_path, "a", "--dump-outputs", str(tmp_path / "a"))
    b = _bench_small(tmp_path, "b", "--dump-outputs", str(tmp_path / "b"), "--full")
    assert a["full"] is False and b["full"] is True
    for d in (a, b):
        assert d["steps"] == 2 and d["warmup"] == 1
        assert d["accuracy_protocol"]["rounds_trained"] == 3 and len(d["accuracy_curve"]) == 3
        assert d["unit"] == "s/round" and d["higher_is_better"] is False and d["dtype"] == "fp32"
        assert d["value"] > 0 and d["ms_per_step"] == pytest.approx(d["value"] * 1000.0)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["accuracy_curve.npy", "model_client0.npy", "model_client1.npy",
                     "round_metrics.npy"]
    assert sorted(os.listdir(tmp_path / "b")) == names
    total = 0
    for n in names:
        x, y = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert x.dtype in (np.float32, np.float64) and x.size > 0 and np.isfinite(x).all(), n
        assert np.array_equal(x, y), n
        total += x.nbytes
    assert total <= 64 << 20
    m0, m1 = np.load(tmp_path / "a" / "model_client0.npy"), np.load(tmp_path / "a" / "model_client1.npy")
    assert m0.shape == m1.shape and np.abs(m0).max() > 0
    assert np.load(tmp_path / "a" / "accuracy_curve.npy").tolist() == pytest.approx(a["accuracy_curve"], abs=1e-4)
    assert np.load(tmp_path / "a" / "round_metrics.npy")[0] == pytest.approx(a["final_train_loss"])


def test_bench_dump_samples_large_models_at_fixed_positions(tmp_path, monkeypatch):
    """A model above the sample budget is dumped at seeded positions: the same sorted positions
    for every model and every call, and never more than the budget over all models."""
    import types

    import numpy as np
    import torch
    import bench   # the repository root is on sys.path (conftest)
    monkeypatch.setattr(bench, "DUMP_SAMPLE_BYTES", 4 * 3 * 100)   # 100 fp32 values per model
    n = 5000
    masters = {c: torch.arange(n, dtype=torch.float32) + 10000.0 * c for c in range(3)}
    fed = types.SimpleNamespace(
        global_master=None, multi=True, local_clients=[0, 1, 2], client_master=masters,
        flat=types.SimpleNamespace(master=masters[0]), cfg=types.SimpleNamespace(num_clients=3),
        rt=types.SimpleNamespace(is_main=True), global_accuracies=[0.5, 0.75])
    last = {"train_loss": 0.25, "global_acc": 0.75, "global_loss": None}
    bench._dump_outputs(fed, str(tmp_path / "x"), last)
    bench._dump_outputs(fed, str(tmp_path / "y"), last)
    pos = np.load(tmp_path / "x" / "model_client0.npy")
    assert pos.dtype == np.float32 and pos.shape == (100,)
    assert (np.diff(pos) >= 0).all() and pos.min() >= 0 and pos.max() < n and len(set(pos.tolist())) > 50
    for c in range(3):
        x = np.load(tmp_path / "x" / f"model_client{c}.npy")
        assert np.array_equal(x, pos + 10000.0 * c)
        assert np.array_equal(x, np.load(tmp_path / "y" / f"model_client{c}.npy"))
    rm = np.load(tmp_path / "x" / "round_metrics.npy")
    assert rm.dtype == np.float64 and rm[:2].tolist() == [0.25, 0.75] and np.isnan(rm[2])
    assert np.load(tmp_path / "x" / "accuracy_curve.npy").tolist() == [0.5, 0.75]


@pytest.mark.slow
def test_bench_gpus2_cpu_rehearsal(tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    env["OMP_NUM_THREADS"] = "2"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--device", "cpu",
                        "--gpus", "2", "--model", "tiny-bert", "--steps", "1", "--warmup", "1",
                        "--no-ckpt", "--out", str(tmp_path / "b")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["steps"] == 1 and d["warmup"] == 1
    assert d["value"] > 0 and d["higher_is_better"] is False
    assert d["config"]["clients"] == 8 and d["config"]["gossip_transport"] == "mailbox"
