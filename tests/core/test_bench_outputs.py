"""bench.py --dump-outputs / --full on the single-process CPU path (tiny
model): the dump is float32, small, and identical from run to run because
the same arguments seed the same weights and batches."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

REPO_ROOT = os.path.dirname(os.path.dirname(
    os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO_ROOT)

import bench  # noqa: E402


def _run_bench(monkeypatch, *extra):
    monkeypatch.setattr(sys, "argv", [
        "bench.py", "--model", "tiny", "--gpus", "1", "--steps", "2",
        "--warmup", "1", "--batch-size", "2", "--seq-len", "64", *extra])
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    # pin the CPU fp32 path wherever the suite runs: its reduction order is
    # fixed, so equal inputs must give bit-equal outputs
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        bench.main()
    lines = buf.getvalue().strip().splitlines()
    return json.loads(lines[-1]), lines


def test_dump_outputs_written_and_reproducible(monkeypatch, tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    out, _ = _run_bench(monkeypatch, "--dump-outputs", str(a))
    _run_bench(monkeypatch, "--dump-outputs", str(b))

    assert out["dtype"] == "fp32"
    assert out["steps"] == 2 and out["ms_per_step"] > 0
    loss = np.load(a / "loss.npy")
    sample = np.load(a / "params_sample.npy")
    assert loss.dtype == np.float32 and loss.shape == (1,)
    assert sample.dtype == np.float32 and sample.ndim == 1
    assert np.isfinite(loss).all() and np.isfinite(sample).all()
    # the loss in the result line is the dumped one
    assert abs(float(loss[0]) - out["config"]["loss"]) <= 1e-6 * abs(loss[0])
    with open(a / "params_sample_index.json") as f:
        index = json.load(f)
    assert index[-1]["stop"] == sample.size
    assert all(e["stop"] - e["start"] == min(e["numel"], 4096)
               for e in index)
    total = sum(os.path.getsize(a / n) for n in os.listdir(a)
                if n.endswith(".npy"))
    assert total <= 64 * 2**20

    np.testing.assert_array_equal(loss, np.load(b / "loss.npy"))
    np.testing.assert_array_equal(sample, np.load(b / "params_sample.npy"))


def test_full_runs_the_plain_path(monkeypatch, tmp_path):
    """Nothing sits behind --full today: it must print the same single
    result line, computed from the same seeded run, as a plain run."""
    plain, plain_lines = _run_bench(
        monkeypatch, "--dump-outputs", str(tmp_path / "p"))
    full, full_lines = _run_bench(
        monkeypatch, "--full", "--dump-outputs", str(tmp_path / "f"))
    assert len(plain_lines) == len(full_lines) == 1
    timing = {"value", "ms_per_step"}
    assert {k: v for k, v in plain.items() if k not in timing} == \
        {k: v for k, v in full.items() if k not in timing}
    assert full["value"] > 0 and full["ms_per_step"] > 0
    for n in ("loss.npy", "params_sample.npy"):
        np.testing.assert_array_equal(np.load(tmp_path / "p" / n),
                                      np.load(tmp_path / "f" / n))
