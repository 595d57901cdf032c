"""Times hwy_traffic beside two yardsticks in one run (development aid): probe_traffic.py [out.json]

  a  all      HighwayVecEnv.traffic_into with every output: the seven per-vehicle arrays, the ego
              row, acc and ep_stats with two restart masks (hwy_traffic, one launch)
  b  ego_acc  the same with the ego row and acc only: what a rollout that wants the ego's numbers
              asks for (the runner's safety_stats asks for acc and ep_stats with two masks)
  c  copy     torch's copy_ of a buffer half as large as what (a) reads and writes per env
              (1,536 B of state, 1,792 B of per-vehicle arrays, 64 B ego, 32 B acc in and out, 32 B
              ep_stats, 2 B masks), so that it moves as many bytes: the floor
  d  torch    the per-vehicle outputs and the ego row restated with plain torch ops on the exported
              state: what a user has to write without hwy_traffic ([E, 64, 64] candidate masks).
              Its front / rear must equal the kernel's and its gap must be the kernel's bits.

at E = 4,096 and 16,384 envs on states a few steps after the reset, and the per-step cost of
safety_stats in a captured LockstepRollout of 4,096 envs (T = 32, hidden 256) against the same
rollout without it.  Each of a-d is captured as a HIP graph of REPS back-to-back calls, warmed,
and replayed ROUNDS times between two events; the figure is the median replay over REPS, in
microseconds per call.  HWY_LIB overrides the library."""
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "highway-rope-ppo_amd"))
import torch
import hwy.native as native

if os.environ.get("HWY_LIB"):
    native.LIB_PATH = os.environ["HWY_LIB"]
from config.base_config import HIGHWAY_CONFIG
from hwy import _abi
from hwy.vec_env import HighwayVecEnv, alloc_traffic
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS, REPS = 15, 50
INF = float("inf")


def timed(fn, reps):
    """Median microseconds per call of fn over ROUNDS replays of a graph of `reps` calls."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with capture(g, stream=side):
            for _ in range(reps):
                fn()
    torch.cuda.current_stream().wait_stream(side)
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / reps * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def gap_over(gap, den):
    return torch.where(gap <= 0, torch.zeros_like(gap),
                       torch.where(den > 0, gap / den, torch.full_like(gap, INF)))


def torch_traffic(state, cfg, out, horizon=4.0, near=50.0):
    """hwy_traffic's per-vehicle outputs and ego row in float32 torch ops on the packed state."""
    f32 = lambda f: state[f].view(torch.float32)  # noqa: E731
    x, y, h, spd = f32(_abi.F_X), f32(_abi.F_Y), f32(_abi.F_HEADING), f32(_abi.F_SPEED)
    ln = state[_abi.F_LANE]
    E, V, L = x.shape[0], int(cfg.vehicles_count) + 1, int(cfg.lanes_count)
    idx = torch.arange(64, device=dev)
    present = ((state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0) & (idx.view(1, 64) < V)
    cand_k = present & (x >= -5.0) & (x < 10005.0)
    vx = spd * torch.cos(h)
    other = idx.view(64, 1) != idx.view(1, 64)
    xk, xi = x.unsqueeze(1), x.unsqueeze(2)

    def neighbours(lane):
        """(front, rear) [E, 64] on lane `lane` [E, 64] of each vehicle"""
        ok = (lane >= 0) & (lane < L) & present
        lat = y.unsqueeze(1) - (lane.to(torch.float32) * 4.0).unsqueeze(2)
        cand = (lat.abs() <= 3.0) & cand_k.unsqueeze(1) & other & ok.unsqueeze(2)
        ahead, behind = cand & (xk >= xi), cand & (xk < xi)
        mn = torch.where(ahead, xk, torch.full_like(lat, INF)).amin(2, keepdim=True)
        best = ahead & (xk == mn)
        front = torch.where(ahead.any(2), 63 - best.flip(2).to(torch.int8).argmax(2), -1)
        mx = torch.where(behind, xk, torch.full_like(lat, -INF)).amax(2, keepdim=True)
        best = behind & (xk == mx)
        rear = torch.where(behind.any(2), best.to(torch.int8).argmax(2), -1)
        return front, rear

    def gaps(front, rear):
        xf = torch.gather(x, 1, front.clamp(min=0))
        xr = torch.gather(x, 1, rear.clamp(min=0))
        return (torch.where(front >= 0, (xf - x) - 5.0, torch.full_like(x, INF)),
                torch.where(rear >= 0, (x - xr) - 5.0, torch.full_like(x, INF)))

    front, rear = neighbours(ln)
    gap, rgap = gaps(front, rear)
    vxf = torch.gather(vx, 1, front.clamp(min=0))
    vxr = torch.gather(vx, 1, rear.clamp(min=0))
    closing = torch.where(front >= 0, vx - vxf, torch.zeros_like(x))
    rclos = torch.where(rear >= 0, vxr - vx, torch.zeros_like(x))
    inf = torch.full_like(x, INF)
    ttc = torch.where(present, gap_over(gap, closing), inf)
    thw = torch.where(present, gap_over(gap, vx), inf)
    risk = torch.where(ttc < horizon, 1.0 - ttc / horizon, torch.zeros_like(x))
    out["front"].copy_(front)
    out["rear"].copy_(rear)
    for k, v in (("gap", gap), ("closing", closing), ("ttc", ttc), ("thw", thw), ("risk", risk)):
        out[k].copy_(v)
    lf, lr = gaps(*neighbours(ln - 1))
    rf, rr = gaps(*neighbours(ln + 1))
    dx, dy = x - x[:, :1], y - y[:, :1]
    others = present & (idx.view(1, 64) != 0)
    dist = torch.sqrt(torch.where(others, dx * dx + dy * dy, inf).amin(1))
    count = (others & (dx >= 0) & (dx <= near)).sum(1).to(torch.float32)
    ego = torch.stack([gap[:, 0], closing[:, 0], ttc[:, 0], thw[:, 0], rgap[:, 0], rclos[:, 0],
                       gap_over(rgap, rclos)[:, 0], lf[:, 0], lr[:, 0], rf[:, 0], rr[:, 0], dist,
                       count, y[:, 0] - ln[:, 0].to(torch.float32) * 4.0, vx[:, 0], risk[:, 0]], 1)
    out["ego"].copy_(ego)


def states(E, steps=3):
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(steps):
        env.step((torch.rand(E, 2, device=dev, generator=gen) - 0.5) * 0.6)
    return env


def rollout_step_us(safety, E=4096, T=32, hidden=256):
    """median microseconds per rollout step of a replayed LockstepRollout graph"""
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    kw = {"safety_stats": True} if safety else {}
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    sd = env.obs_rows * env.obs_features
    torch.manual_seed(0)
    agent = PPOAgent(sd, 2, hidden_dim=hidden, device=dev, seed=0)
    buf = RolloutBuffer(T, E, sd, 2, dev, **kw)
    obs, _ = env.reset()
    buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, env, buf, use_graph=True, **kw)
    for _ in range(4):
        roll.run()
        roll.start_next()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        roll.run()
        e1.record()
        torch.cuda.synchronize()
        roll.start_next()
        us.append(e0.elapsed_time(e1) / T * 1e3)
    out = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us),
           "replays": roll.stats["rollout_replay"]}
    env.close()
    return out


results = []
for E in (4096, 16384):
    env = states(E)
    t = alloc_traffic(E, dev)
    masks = (torch.zeros(E, dtype=torch.uint8, device=dev), torch.zeros(E, dtype=torch.uint8, device=dev))
    moved = (1536 + 7 * 256 + 64 + 3 * 32 + 2) * E
    src, dst = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    row = {"envs": E, "bytes_moved": moved, "reps": REPS, "rounds": ROUNDS,
           "all": timed(lambda: env.traffic_into(restart=masks, **t), REPS),
           "ego_acc": timed(lambda: env.traffic_into(ego=t["ego"], acc=t["acc"]), REPS),
           "copy": timed(lambda: dst.copy_(src), REPS)}
    for k in ("all", "copy"):
        row[k]["GB_per_s"] = moved / row[k]["median_us"] * 1e-3
    row["all_over_copy"] = row["all"]["median_us"] / row["copy"]["median_us"]
    st, cfg = env.export_state(), env.hwy_config
    tt = alloc_traffic(E, dev)
    row["torch"] = timed(lambda: torch_traffic(st, cfg, tt), 5)
    row["torch"]["how"] = "graph of 5"
    row["torch_over_all"] = row["torch"]["median_us"] / row["all"]["median_us"]
    env.traffic_into(**{k: t[k] for k in _abi.TRAFFIC_VEHICLE_OUTPUTS + ("ego",)})
    torch_traffic(st, cfg, tt)
    row["torch_front_rear_differing"] = int((tt["front"] != t["front"]).sum().item()
                                            + (tt["rear"] != t["rear"]).sum().item())
    row["torch_gap_words_differing"] = int((tt["gap"].view(torch.int32)
                                            != t["gap"].view(torch.int32)).sum().item())
    row["torch_closing_max_abs_diff"] = float((tt["closing"] - t["closing"]).abs().max().item())
    exact = [0, 4, 7, 8, 9, 10, 11, 12, 13]
    row["torch_ego_exact_words_differing"] = int(
        (tt["ego"][:, exact].contiguous().view(torch.int32)
         != t["ego"][:, exact].contiguous().view(torch.int32)).sum().item())
    print(json.dumps(row), flush=True)
    results.append(row)
    env.close()
    del st, tt, t, src, dst
    torch.cuda.empty_cache()
roll = {"envs": 4096, "T": 32, "hidden": 256, "off": rollout_step_us(False), "on": rollout_step_us(True)}
roll["safety_stats_us_per_step"] = roll["on"]["median_us"] - roll["off"]["median_us"]
roll["on_over_off"] = roll["on"]["median_us"] / roll["off"]["median_us"]
print(json.dumps(roll), flush=True)
results.append({"rollout": roll})
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
assert all(math.isfinite(r["all"]["median_us"]) for r in results if "all" in r)
assert all(r.get("torch_front_rear_differing", 0) == 0 for r in results), "the torch neighbours differ"
assert all(r.get("torch_gap_words_differing", 0) == 0 for r in results), "the torch gaps differ"
assert all(r.get("torch_ego_exact_words_differing", 0) == 0 for r in results), "the torch ego row differs"
assert all(r["torch_over_all"] > 1.0 for r in results if "all" in r), "torch beats the kernel"
