"""bench.py end to end on the GPU at a small size: one JSON line with the driver's keys; with
--full also the MFMA roofline of the minibatch step and the env-step HBM view (the driver runs the
full size).  A plain run prints the headline line only and, with --dump-outputs, writes what its
last timed step computed."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_emits_contract_line():
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "2", "--warmup", "1",
           "--envs", "512", "--rollout", "8", "--minibatches", "4", "--epochs", "2",
           "--full", "--no-cpu-baseline"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1
    assert d["value"] > 0 and d["higher_is_better"] is True and d["scaling"] == "weak"
    # value = env-steps of the timed steps / their wall time
    assert abs(d["value"] - 512 * 8 * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 0.01
    r = d["roofline"]
    assert r["bound"] == "mfma" and r["unit"] == "TFLOP/s" and 0 < r["frac"] < 1
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3
    e = d["roofline_env_step"]
    assert e["bound"] == "hbm" and 0 < e["frac"] < 1 and e["envs_per_launch"] == 512


def test_plain_run_is_lean_and_dumps_its_outputs(tmp_path):
    """A plain run carries the headline keys and none of --full's measurements; --dump-outputs
    writes the last timed step's rollout, parameters and metrics as float32 / float64 .npy."""
    import numpy as np

    E, T, S, H = 512, 8, 60, 256
    out_dir = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2",
           "--warmup", "1", "--envs", str(E), "--rollout", str(T), "--minibatches", "4",
           "--epochs", "2", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config"):
        assert k in d, k
    for k in ("roofline", "roofline_env_step", "cpu_baseline", "breakdown_ms"):
        assert k not in d, k
    assert "reward_parity" not in d["config"]
    assert d["steps"] == 2 and d["dtype"] == "fp32" and d["higher_is_better"] is True
    assert abs(d["value"] - E * T * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 0.01
    shapes = {"states": (T + 1, E, S), "actions": (T, E, 2), "pre_tanh": (T, E, 2),
              "log_probs": (T, E), "values": (T, E), "rewards": (T, E), "terminated": (T, E),
              "truncated": (T, E), "dones": (T, E), "ep_return": (T, E), "ep_length": (T, E),
              "params": (S * H + H + 3 * (H * H + H) + 2 * H + 2 + 2 + H + 1,), "metrics": (7,)}
    assert sorted(os.listdir(out_dir)) == sorted(f"{k}.npy" for k in shapes)
    total = 0
    for name, shape in shapes.items():
        a = np.load(out_dir / f"{name}.npy")
        assert a.shape == shape, (name, a.shape)
        assert a.dtype == (np.float64 if name == "metrics" else np.float32), (name, a.dtype)
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    # the rollout is the policy's own: bounded actions, the next step's first row carried over
    acts = np.load(out_dir / "actions.npy")
    assert np.abs(acts).max() <= 1.0 and acts.std() > 0
    st = np.load(out_dir / "states.npy")
    assert np.array_equal(st[0], st[T])
    assert d["dumped_outputs"]["elements_written_of_total"]["states"] == [st.size, st.size]
