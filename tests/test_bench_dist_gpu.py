"""bench.py's N > 1 path as the driver launches it (torch.distributed.run, one process per
rank), rehearsed with 2 and 4 ranks on one GPU: gloo stands in for RCCL (HWY_BENCH_DIST_BACKEND).
Rank 0 prints one line; value is the whole job's env-steps over the max-over-ranks time."""

import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.parametrize("n", [2, 4])
def test_bench_two_ranks_one_line(n):
    """bench.py under torch.distributed.run with n gloo ranks on the one GPU (the driver's N > 1
    launch, rehearsed): one JSON line, whole-job value over all ranks' envs."""
    env = dict(os.environ, HWY_BENCH_DIST_BACKEND="gloo")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
           os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--steps", "2", "--warmup", "1",
           "--envs", "256", "--rollout", "8", "--minibatches", "4", "--epochs", "2",
           "--full"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=150, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["n_gpus"] == n and d["scaling"] == "weak" and d["cpu_baseline"] is None
    assert d["config"]["global_envs"] == 256 * n
    assert abs(d["value"] - 256 * n * 8 * 2 / (d["ms_per_step"] * 2e-3)) / d["value"] < 0.01
    # the all-reduce's own cost beside the step it burdens: the flat gradient
    # bucket of ActorCritic(60, 2, 256) in fp32, timed alone, and the step time that includes it
    roof = d["roofline"]
    S, H = 60, 256
    n_params = S * H + H + 3 * (H * H + H) + 2 * H + 2 + 2 + H + 1
    ar = roof["allreduce"]
    assert ar["bytes"] == 4 * n_params and ar["us_per_allreduce"] > 0
    # gloo cannot be captured: the all-reduce runs host-mediated between per-step graphs, where
    # the epoch events do not span it (bench.py), so the step that includes it is the
    # synchronised update's host clock per step; one all-reduce is a share of it in (0, 1), and
    # the printed share is re-derived from the printed (rounded) fields at rel 1e-3
    assert d["config"]["epoch_graph_collectives"] == "per-step graphs, all-reduce between them"
    assert roof["includes_allreduce"] is False
    assert roof["step_us_with_allreduce"] == roof["update_host_us_per_step"] > 0
    share = roof["allreduce_share_of_step"]
    assert share == pytest.approx(ar["us_per_allreduce"] / roof["step_us_with_allreduce"], rel=1e-3)
    assert share > 0, (share, ar, roof["step_us_with_allreduce"], roof["avg_launch_us"])
    if n == 2:
        # one all-reduce is part of the step it burdens.  At 4 ranks on the one GPU (and the
        # box's 16-CPU share) the host-mediated gloo timings are contention-bound: a probed
        # all-reduce measured 22.5 ms against 17.5 ms for a whole step that includes one
        assert share < 1, (share, ar, roof["step_us_with_allreduce"], roof["avg_launch_us"])
    # the line proves its ranks from the communicator: world size and backend
    # as the process group reports them, every rank's device and PCI location, whether the epoch
    # graph captured the collective; gloo rehearses both ranks on one GPU (one distinct device)
    rk = d["config"]["ranks"]
    assert rk["world_size"] == n and rk["backend"] == "gloo"
    assert sorted(r["rank"] for r in rk["per_rank"]) == list(range(n))
    assert all(r["pci"] and r["device"] == 0 for r in rk["per_rank"])
    assert rk["distinct_devices"] == 1
    assert d["config"]["epoch_graph_collectives"] in ("captured",
                                                      "per-step graphs, all-reduce between them")
    # per-kernel times of the step beside the epoch-event step time
    pk = roof["per_kernel"]
    assert set(pk) >= {"ppo_rows", "ppo_wgrad", "ppo_wsum", "ppo_adam", "sum_us", "method",
                       "launch_floor_us"}
    assert all(pk[k]["us"] > 0 for k in ("ppo_rows", "ppo_wgrad", "ppo_wsum", "ppo_adam"))
    # the empty kernel's graph launch is the floor every kernel's launch pays
    assert 0 < pk["launch_floor_us"] < min(pk[k]["us"] for k in ("ppo_rows", "ppo_wsum"))
    assert roof["flops_required_per_launch"] < roof["flops_per_launch"]
