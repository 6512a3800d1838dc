"""bench.py's plain run and --dump-outputs, with a stub engine on the CPU: a plain run times the headline and nothing else;
--full is where the roofline, CPU baseline and extra legs live; the dump is the last timed step's outputs as float32."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from modulationdetectioncnn_amd import Topology  # noqa: E402


class _Stub:
    topology = Topology.vtcnn2(11)
    dtype = "bf16"


def _stub_engine(monkeypatch, n, classes=11):
    calls = []
    probs = torch.softmax(torch.from_numpy(np.random.default_rng(1).standard_normal((n, classes)).astype(np.float32)), 1)
    labels = probs.argmax(1).to(torch.int32)

    def run_workload(name, device, steps, warmup, dist=None, frames=None):
        calls.append((name, steps, warmup))
        return _Stub(), None, probs, labels, n, 0.001 * steps

    def refuse(*a, **k):
        raise AssertionError("a plain run measures only the headline")

    monkeypatch.setattr(bench, "run_workload", run_workload)
    monkeypatch.setattr(bench, "select_device", lambda d: None)
    for fn in ("dominant_roofline", "cpu_baseline", "live_traffic", "run_iq_u8", "run_q612", "run_training", "run_host_path"):
        monkeypatch.setattr(bench, fn, refuse)
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    return calls, probs, labels


def _main(argv):
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        rc = bench.main(argv)
    lines = [l for l in buf.getvalue().splitlines() if l.strip()]
    assert rc == 0 and len(lines) == 1
    return json.loads(lines[0])


def test_plain_run_times_the_headline_only_and_dumps_its_outputs(monkeypatch, tmp_path):
    calls, probs, labels = _stub_engine(monkeypatch, 4096)
    j = _main(["--gpus", "1", "--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "out")])
    assert calls == [(bench.DEFAULT, 7, 2)]
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in j
    assert j["steps"] == 7 and j["ms_per_step"] == pytest.approx(1.0) and j["value"] == pytest.approx(4096 * 1000.0)
    assert "roofline" not in j and "cpu_baseline" not in j and "extra" not in j and j["config"]["full"] is False
    assert sorted(os.listdir(tmp_path / "out")) == ["labels.npy", "probs.npy"]
    p, l = np.load(tmp_path / "out" / "probs.npy"), np.load(tmp_path / "out" / "labels.npy")
    assert p.dtype == np.float32 and l.dtype == np.float32
    np.testing.assert_array_equal(p, probs.numpy())
    np.testing.assert_array_equal(l, labels.numpy().astype(np.float32))


def test_full_run_reaches_the_roofline_pass(monkeypatch):
    _stub_engine(monkeypatch, 4096)
    seen = []
    monkeypatch.setattr(bench, "dominant_roofline", lambda *a, **k: seen.append(1) or ({"bound": "mfma", "frac": 0.5}, {}))
    j = _main(["--steps", "3", "--warmup", "1", "--full", "--no-extras", "--no-cpu-baseline", "--no-live-traffic"])
    assert seen == [1] and j["roofline"]["frac"] == 0.5 and j["config"]["full"] is True


def test_dump_of_a_large_output_is_a_fixed_seeded_sample_under_64mb(monkeypatch, tmp_path):
    assert (1 << 20) * 4 * (11 + 1) <= bench.DUMP_BUDGET_BYTES < 64_000_000      # the headline's outputs are dumped whole
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 48 * 100)          # room for 100 rows of 11 + 1 floats (+ the index)
    n = 5000
    probs = torch.arange(n * 11, dtype=torch.float32).reshape(n, 11)
    labels = torch.arange(n, dtype=torch.int32)
    assert bench.dump_outputs(str(tmp_path / "a"), probs, labels) == ["labels", "probs", "sample_rows"]
    bench.dump_outputs(str(tmp_path / "b"), probs, labels)
    rows = np.load(tmp_path / "a" / "sample_rows.npy")
    assert rows.dtype == np.float64 and np.all(np.diff(rows) > 0) and 0 < len(rows) <= 100
    np.testing.assert_array_equal(rows, np.load(tmp_path / "b" / "sample_rows.npy"))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "labels.npy"), rows.astype(np.float32))
    np.testing.assert_array_equal(np.load(tmp_path / "a" / "probs.npy"), probs.numpy()[rows.astype(np.int64)])
