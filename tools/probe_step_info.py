"""hwy_step against hwy_step_with_info (development aid): the same env kernel body with and
without the info stores (per-step speed / crashed / lane / reward terms, per-episode sums).
Twin handles from the same state, interleaved, 5 rounds, per env count; prints ms per step for
each (device events) and checks the two produce the same observations.

    python tools/probe_step_info.py [E ...]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                                "highway-rope-ppo_amd"))
import torch  # noqa: E402

from config.base_config import HIGHWAY_CONFIG  # noqa: E402
from hwy.vec_env import HighwayVecEnv, alloc_step_info  # noqa: E402

DEV = torch.device("cuda", 0)
for E in [int(x) for x in (sys.argv[1:] or ["4096", "16384"])]:
    envs = [HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=DEV, autoreset=True, seed_base=42)
            for _ in range(2)]
    for env in envs:
        env.reset()
    bufs = [(torch.zeros(E, 2, device=DEV), torch.empty_like(envs[0].obs_buf),
             torch.empty(E, device=DEV), torch.empty(E, dtype=torch.uint8, device=DEV),
             torch.empty(E, dtype=torch.uint8, device=DEV), torch.empty(E, device=DEV),
             torch.empty(E, dtype=torch.int32, device=DEV)) for _ in range(2)]
    info = alloc_step_info(E, DEV)
    run = {"hwy_step": lambda: envs[0].step_into(*bufs[0]),
           "hwy_step_with_info": lambda: envs[1].step_into(*bufs[1], info=info)}
    for _ in range(5):
        for f in run.values():
            f()
    torch.cuda.synchronize()
    same = torch.equal(bufs[0][1], bufs[1][1])
    n = 50
    res = {k: [] for k in run}
    for _ in range(5):
        for name, f in run.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            for _ in range(n):
                f()
            e.record()
            torch.cuda.synchronize()
            res[name].append(s.elapsed_time(e) / n)
    same = same and torch.equal(bufs[0][1], bufs[1][1])
    print(f"E={E} same obs {same}: " + "  ".join(
        f"{k} {min(v):.4f}-{max(v):.4f} ms (median {sorted(v)[len(v) // 2]:.4f})"
        for k, v in res.items()), flush=True)
    for env in envs:
        env.close()
