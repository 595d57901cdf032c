"""Times hwy_lookahead beside its yardsticks in one run (development aid):
probe_lookahead.py [out.json]          the measurements below
probe_lookahead.py --budget [out.json] only hwy_lookahead at E*K = 16,384 and 24,576 waves (to
                                       compare the register budgets: run once with the product
                                       library and once with HWY_LIB=.../libhwy_w4.so from
                                       `make variant V=w4 VEXTRA=-DHWY_STEP_BIG_W=4`, whose
                                       big build is the 4-wave one)

At E = 4,096 envs (default config, states a few steps after the reset), for (K 4, H 3) and
(K 6, H 4), candidates held (hold mode):
  flags   lookahead_into with steps, terminated, truncated
  all     lookahead_into with every output (rewards, ret, ego_final and obs too)
  lazy    lookahead_into with steps, terminated, truncated under lazy
  steps   K*H plain hwy_step launches of E envs on an autoreset-off clone handle, after one
          hwy_import_state of the same states (the step kernel is the one it was before
          hwy_lookahead existed: its code object is unchanged)
  clone   the route without hwy_lookahead: one hwy_export_state, then K times hwy_import_state
          and H hwy_step launches
  import  one hwy_import_state alone (what `steps` carries besides its K*H steps)
Each is captured as a HIP graph of REPS back-to-back calls, warmed, and replayed ROUNDS times
between two events; the figure is the median replay over REPS, in microseconds per call.

Then the captured rollout of training (LockstepRollout, 4,096 envs x 32 steps, H 256) without a
shield and under the default hwy.Shield(): microseconds per rollout step of each, the difference
and the share of steps the shield overrode.  HWY_LIB overrides the library."""
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
from hwy import Shield
from hwy.vec_env import HighwayVecEnv
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS, REPS = 15, 10
HELD = ((0.0, 0.0), (-1.0, 0.0), (1.0, 0.0), (0.3, -0.5), (0.3, 0.5), (-0.3, 0.2))


def timed(fn, reps):
    """Median microseconds per call of fn over ROUNDS replays of a graph of `reps` calls."""
    for _ in range(2):
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
    for _ in range(2):
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


def states(E, steps=3, autoreset=True):
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=autoreset, seed_base=5)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(steps):
        env.step((torch.rand(E, 2, device=dev, generator=gen) - 0.5) * 0.6)
    return env


def outputs(env, K, H, which):
    E, N, Fo = env.num_envs, env.obs_rows, env.obs_features
    kw = dict(device=dev)
    out = dict(steps=torch.empty(E, K, dtype=torch.int32, **kw),
               terminated=torch.empty(E, K, dtype=torch.uint8, **kw),
               truncated=torch.empty(E, K, dtype=torch.uint8, **kw))
    if which == "all":
        out.update(rewards=torch.empty(E, K, H, **kw), ret=torch.empty(E, K, **kw),
                   ego_final=torch.empty(E, K, 4, **kw), obs=torch.empty(E, K, N, Fo, **kw))
    return out


def candidates(E, K):
    return torch.tensor(HELD[:K], dtype=torch.float32, device=dev).repeat(E, 1, 1).contiguous()


def lookahead_rows(E, K, H):
    env = states(E)
    cand = candidates(E, K)
    row = {"envs": E, "k": K, "horizon": H, "waves": E * K, "reps": REPS, "rounds": ROUNDS}
    for name, which, lazy in (("flags", "flags", False), ("all", "all", False), ("lazy", "flags", True)):
        out = outputs(env, K, H, which)
        row[name] = timed(lambda: env.lookahead_into(cand, H, hold=True, lazy=lazy, **out), REPS)
        if name == "flags":
            row["mean_steps"] = float(out["steps"].float().mean().item())
            row["terminated_share"] = float(out["terminated"].float().mean().item())
        if name == "lazy":
            row["lazy_run_share"] = float((out["steps"] > 0).float().mean().item())
    return env, cand, row


def step_rows(env, cand, K, H, row):
    """the reference points on an autoreset-off clone of env's states"""
    E = env.num_envs
    clone = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=False, seed_base=5)
    clone.reset()
    state = env.export_state()
    acts = [cand[:, k].contiguous() for k in range(K)]
    io = (clone.obs_buf, clone.reward_buf, clone.term_buf, clone.trunc_buf)

    def steps():
        clone.import_state(state)
        for k in range(K):
            for _ in range(H):
                clone.step_into(acts[k], *io)

    def route():
        st = env.export_state()
        for k in range(K):
            clone.import_state(st)
            for _ in range(H):
                clone.step_into(acts[k], *io)

    row["steps"] = timed(steps, REPS)
    row["clone"] = timed(route, REPS)
    row["import"] = timed(lambda: clone.import_state(state), REPS)
    for name in ("flags", "all", "lazy"):
        row[f"{name}_over_steps"] = row[name]["median_us"] / row["steps"]["median_us"]
    clone.close()


def rollout_step_us(shield, E=4096, T=32):
    """Median microseconds per step of the replayed rollout graph of training, under `shield`"""
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    sd = env.obs_rows * env.obs_features
    agent = PPOAgent(sd, 2, lr=3e-4, epochs=2, hidden_dim=256, device=dev, num_minibatches=4, seed=5)
    buf = RolloutBuffer(T, E, sd, 2, dev, **({} if shield is None else {"shield": True}))
    obs, _ = env.reset()
    buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, env, buf, use_graph=True,
                           **({} if shield is None else {"shield": shield}))
    us, rates = [], []
    for it in range(4 + ROUNDS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        roll.run()
        e1.record()
        torch.cuda.synchronize()
        if it >= 4:
            us.append(e0.elapsed_time(e1) / T * 1e3)
            if shield is not None:
                rates.append(float((buf.chosen != 0).float().mean().item()))
        roll.start_next()
    assert roll.stats["rollout_replay"] >= ROUNDS, roll.stats
    env.close()
    out = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}
    if rates:
        out["shield_rate"] = statistics.mean(rates)
    return out


def save(results, path):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(results, f, indent=1)


args = [a for a in sys.argv[1:] if not a.startswith("--")]
path = args[0] if args else None
results = []
if "--budget" in sys.argv:
    for E, K, H in ((4096, 4, 3), (4096, 6, 4), (2048, 4, 3)):
        env, cand, row = lookahead_rows(E, K, H)
        row["lib"] = os.path.basename(native.LIB_PATH)
        print(json.dumps(row), flush=True)
        results.append(row)
        env.close()
    save(results, path)
    sys.exit(0)

for K, H in ((4, 3), (6, 4)):
    env, cand, row = lookahead_rows(4096, K, H)
    step_rows(env, cand, K, H, row)
    print(json.dumps(row), flush=True)
    results.append(row)
    env.close()
roll = {"envs": 4096, "steps": 32, "hidden": 256, "shield": Shield().to_dict(),
        "plain": rollout_step_us(None), "shielded": rollout_step_us(Shield())}
roll["added_us_per_step"] = roll["shielded"]["median_us"] - roll["plain"]["median_us"]
roll["added_share"] = roll["added_us_per_step"] / roll["plain"]["median_us"]
print(json.dumps(roll), flush=True)
results.append({"rollout": roll})
save(results, path)
assert all(math.isfinite(r["flags"]["median_us"]) for r in results if "flags" in r)
