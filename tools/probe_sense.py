"""Times hwy_sense beside its yardsticks in one run (development aid): probe_sense.py [out.json]

  a  observe  HighwayVecEnv.observe_into with `obs` only (hwy_observe, one launch): the perfect sensor
  b  null     sense_into with `obs` only under the null sensor (the same rows, bit for bit: asserted)
  c  full     sense_into with `obs` only under line of sight + a 120 m range + dropout 0.2 + noise
  d  all      (c) with every output: obs, row_vehicle, visible, hidden, counts
  e  los      sense_into with `obs` only under line of sight alone
  f  copy     torch's copy_ of a buffer half as large as what (c) reads and writes per env
              (1,536 B of state + 4 N F_out B of rows), so that it moves as many bytes: the floor

at E = 4,096 and 16,384 envs (N 15, F 4, stored `sorted`, no wrapper), on states a few steps after
the reset.  Each is captured as a HIP graph of REPS back-to-back calls, warmed, and replayed ROUNDS
times between two events; the figure is the median replay over REPS, in microseconds per call.

Then the captured rollout of training (LockstepRollout, 4,096 envs x 32 steps, H 256) without a
sensor and under (c): microseconds per rollout step of each and the difference.

probe_sense.py --kernels NAME [launches]: nothing but `launches` (default 200) back-to-back
launches of configuration NAME (observe, null, los, full or all) at 4,096 envs and a
synchronisation, for a kernel-stats profile of that configuration alone.  HWY_LIB overrides the
library."""
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
from hwy import SensorModel
from hwy.vec_env import HighwayVecEnv
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS, REPS = 15, 50
NULL = SensorModel()
LOS = SensorModel(los=True)
FULL = SensorModel(los=True, range=120.0, dropout=0.2, noise=(0.5, 0.2, 0.4), salt=7)


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


def states(E, steps=3):
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(steps):
        env.step((torch.rand(E, 2, device=dev, generator=gen) - 0.5) * 0.6)
    return env


def calls(env):
    """name -> a launch of that configuration on env, and the buffers they write"""
    E, N, Fo = env.num_envs, env.obs_rows, env.obs_features
    obs = torch.empty(E, N, Fo, device=dev)
    out = dict(row_vehicle=torch.empty(E, N, dtype=torch.int32, device=dev),
               visible=torch.empty(E, 64, dtype=torch.uint8, device=dev),
               hidden=torch.empty(E, 64, device=dev),
               counts=torch.empty(E, 4, dtype=torch.int32, device=dev))
    return {"observe": lambda: env.observe_into(obs=obs),
            "null": lambda: env.sense_into(NULL, obs=obs),
            "los": lambda: env.sense_into(LOS, obs=obs),
            "full": lambda: env.sense_into(FULL, obs=obs),
            "all": lambda: env.sense_into(FULL, obs=obs, **out)}, obs, out


def rollout_step_us(sensor, E=4096, T=32):
    """Median microseconds per step of the replayed rollout graph of training, under `sensor`"""
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    sd = env.obs_rows * env.obs_features
    agent = PPOAgent(sd, 2, lr=3e-4, epochs=2, hidden_dim=256, device=dev, num_minibatches=4, seed=5)
    buf = RolloutBuffer(T, E, sd, 2, dev)
    obs, _ = env.reset()
    buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, env, buf, use_graph=True,
                           **({} if sensor is None else {"sensor": sensor}))
    us = []
    for it in range(4 + ROUNDS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        roll.run()
        e1.record()
        torch.cuda.synchronize()
        if it >= 4:
            us.append(e0.elapsed_time(e1) / T * 1e3)
        roll.start_next()
    assert roll.stats["rollout_replay"] >= ROUNDS, roll.stats
    env.close()
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    env = states(4096)
    fn = calls(env)[0][sys.argv[2]]
    for _ in range(int(sys.argv[3]) if len(sys.argv) > 3 else 200):
        fn()
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

results = []
for E in (4096, 16384):
    env = states(E)
    N, Fo = env.obs_rows, env.obs_features
    fns, obs, out = calls(env)
    moved = (1536 + 4 * N * Fo) * E
    src, dst = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))
    row = {"envs": E, "rows": N, "f_out": Fo, "bytes_moved": moved, "reps": REPS, "rounds": ROUNDS,
           "sensor_full": FULL.to_dict()}
    for name, fn in fns.items():
        row[name] = timed(fn, REPS)
    row["copy"] = timed(lambda: dst.copy_(src), REPS)
    for k in ("null", "los", "full", "all"):
        row[f"{k}_over_observe"] = row[k]["median_us"] / row["observe"]["median_us"]
        row[f"{k}_over_copy"] = row[k]["median_us"] / row["copy"]["median_us"]
    fns["null"]()
    assert torch.equal(obs, env.obs_buf), "the null sensor's rows differ from the step's"
    fns["all"]()
    c = out["counts"].double().sum(0)
    row["present_others"], row["out_of_range"], row["blocked"], row["dropped"] = (float(x) for x in c)
    row["visible_others"] = float(out["visible"][:, 1:].sum().item())
    print(json.dumps(row), flush=True)
    results.append(row)
    env.close()
roll = {"envs": 4096, "steps": 32, "hidden": 256, "plain": rollout_step_us(None),
        "sensed": rollout_step_us(FULL)}
roll["added_us_per_step"] = roll["sensed"]["median_us"] - roll["plain"]["median_us"]
roll["added_share"] = roll["added_us_per_step"] / roll["plain"]["median_us"]
print(json.dumps(roll), flush=True)
results.append({"rollout": roll})
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
assert all(math.isfinite(r["full"]["median_us"]) for r in results if "full" in r)
