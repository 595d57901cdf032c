"""Times hwy_grid beside its yardsticks in one run (development aid): probe_grid.py [out.json]

  a  observe  HighwayVecEnv.observe_into with `obs` only (hwy_observe, one launch)
  b  grid     grid_into with `out` only, the default spec (3 x 24 x 5 and the ego tail)
  c  all      grid_into with every output: out, cell_vehicle, veh_cell, counts
  d  copy     torch's copy_ of a buffer half as large as what (b) reads and writes per env
              (1,280 B of state + 4 stride B of row), so that it moves as many bytes: the floor
  e  copy_all the same for (c)'s bytes
  f  torch    the same rule restated in torch ops on the exported state (presence, vx, vy and the
              tail; asserted equal to (b) up to the device's sin / cos), eager launches and all

at E = 4,096 and 16,384 envs (the shipped config: N 15, F 4, 50 other vehicles), on states a few
steps after the reset.  (a) to (e) are captured as a HIP graph of REPS back-to-back calls, warmed,
and replayed ROUNDS times between two events; the figure is the median replay over REPS, in
microseconds per call.  (f) is timed likewise, eagerly (its ops allocate, so it is not captured).

Then the captured rollout of training (LockstepRollout, 4,096 envs x 32 steps, H 256) on the
Kinematics rows and on the grid: microseconds per rollout step of each and the difference.  The
two differ in the policy's input width (60 against 364 floats) as well as in the hwy_grid launch.

probe_grid.py --minibatch OUT.json: the fused minibatch step at S = 60, 300, 364, 368 and 600,
H 256, 4,096 rows per minibatch (beside profiles/r9/wide's S 300 and S 600), by
tools/wide_step_timing.py's protocol: microseconds per step from events around every epoch.

probe_grid.py --kernels NAME [launches]: nothing but `launches` (default 200) back-to-back
launches of configuration NAME (observe, grid or all) at 4,096 envs and a synchronisation, for a
kernel-stats profile of that configuration alone.  HWY_LIB overrides the library."""
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
from hwy import GridSpec, _abi
from hwy.vec_env import HighwayVecEnv
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS, REPS = 15, 50
SPEC = GridSpec()


def timed(fn, reps, graph=True):
    """Median microseconds per call of fn over ROUNDS runs of `reps` calls (one replayed graph of
    them, or, graph=False, the eager calls)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    run = lambda: [fn() for _ in range(reps)]  # noqa: E731
    if graph:
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        g = torch.cuda.CUDAGraph()
        with torch.cuda.stream(side):
            with capture(g, stream=side):
                run()
        torch.cuda.current_stream().wait_stream(side)
        run = g.replay
    for _ in range(3):
        run()
    torch.cuda.synchronize()
    us = []
    for _ in range(ROUNDS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
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
    out = torch.empty(E, SPEC.stride(int(env.hwy_config.n_features)), device=dev)
    rest = dict(cell_vehicle=torch.empty(E, SPEC.nx, SPEC.ny, dtype=torch.int32, device=dev),
                veh_cell=torch.empty(E, 64, dtype=torch.int32, device=dev),
                counts=torch.empty(E, 4, dtype=torch.int32, device=dev))
    return {"observe": lambda: env.observe_into(obs=obs),
            "grid": lambda: env.grid_into(SPEC, out=out),
            "all": lambda: env.grid_into(SPEC, out=out, **rest)}, out, rest


def torch_grid(env, state):
    """the default spec's rule in torch ops on an exported state [NFIELDS, E, 64] (int32)"""
    cfg = env.hwy_config
    E, V, n = state.shape[1], cfg.vehicles_count + 1, SPEC.nx * SPEC.ny
    f = lambda k: state[k].view(torch.float32)  # noqa: E731
    x, y, h, spd = f(_abi.F_X), f(_abi.F_Y), f(_abi.F_HEADING), f(_abi.F_SPEED)
    present = (state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    present[:, V:] = False
    qx = ((x - x[:, :1]) - SPEC.x0) / SPEC.step_x
    qy = ((y - y[:, :1]) - SPEC.y0) / SPEC.step_y
    inside = present & (qx >= 0) & (qx < SPEC.nx) & (qy >= 0) & (qy < SPEC.ny)
    cell = torch.where(inside, qx.floor().long() * SPEC.ny + qy.floor().long(),
                       torch.full_like(qx, n, dtype=torch.long))
    idx = torch.arange(64, device=state.device).expand(E, 64)
    owner = torch.full((E, n + 1), 64, dtype=torch.long, device=state.device)
    owner.scatter_reduce_(1, cell, idx, "amin")
    owner = owner[:, :n]
    won = owner < 64
    src = owner.clamp(max=63)
    vx, vy = spd * torch.cos(h), spd * torch.sin(h)
    layers = [torch.ones_like(x)]
    for v in (vx, vy):
        rel = v - v[:, :1]
        layers.append((-1.0 + (rel + 80.0) * 2.0 / 160.0).clamp(-1.0, 1.0))
    grid = torch.stack([torch.where(won, l.gather(1, src), torch.zeros_like(x[:, :1]))
                        for l in layers], 1).reshape(E, 3 * n)
    tail = []
    for k in range(cfg.n_features):
        v = {1: x, 2: y, 3: vx, 4: vy}[int(cfg.feature_ids[k])][:, 0]
        lo, hi = cfg.features_range[k][0], cfg.features_range[k][1]
        tail.append((-1.0 + (v - lo) * 2.0 / (hi - lo)).clamp(-1.0, 1.0))
    return torch.cat([grid, torch.stack(tail, 1)], 1)


def rollout_step_us(grid, E=4096, T=32):
    """Median microseconds per step of the replayed rollout graph of training, on `grid`"""
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    sd = (env.obs_rows * env.obs_features if grid is None
          else grid.stride(int(env.hwy_config.n_features)))
    agent = PPOAgent(sd, 2, lr=3e-4, epochs=2, hidden_dim=256, device=dev, num_minibatches=4, seed=5)
    buf = RolloutBuffer(T, E, sd, 2, dev)
    obs, _ = env.reset()
    if grid is None:
        buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, env, buf, use_graph=True, **({} if grid is None else {"grid": grid}))
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
    return {"state_dim": sd, "median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def minibatch_step_us(S, H=256, B=4096, nmb=4, epochs=8, updates=3):
    """Median microseconds per fused minibatch step (S wide, B rows): tools/wide_step_timing.py's
    protocol, HIP events around every epoch of the captured epoch graph (FusedPPO.epoch_events)"""
    from hwy.ppo_native import FusedPPO
    from ppo.agent import PPOAgent

    torch.manual_seed(0)
    ag = PPOAgent(S, 2, lr=3e-4, epochs=epochs, hidden_dim=H, device=dev, backend="hip")
    g = torch.Generator(device=dev).manual_seed(1)
    n = B * nmb
    s = torch.randn(n, S, device=dev, generator=g)
    with torch.no_grad():
        _, z, lp, v = ag.actor_critic.act(s, generator=g)
    z = z.contiguous()
    lp = (lp + 0.05 * torch.randn(n, device=dev, generator=g)).contiguous()
    adv = torch.randn(n, device=dev, generator=g)
    ret = v + torch.randn(n, device=dev, generator=g)
    perm = torch.randperm(n, device=dev, generator=g)
    F = FusedPPO(ag, B, nmb, use_graphs=True)
    assert F._tile_off is not None, "the general path"
    for _ in range(2):  # capture, then warm
        F.run(s, z, lp, adv, ret, perm)
    torch.cuda.synchronize()
    F.epoch_events = []
    for _ in range(updates):
        F.run(s, z, lp, adv, ret, perm)
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 / nmb for a, b in F.epoch_events]
    return {"S": S, "H": H, "rows": B, "epochs_timed": len(us), "median_us": statistics.median(us),
            "min_us": min(us), "max_us": max(us)}


if len(sys.argv) > 2 and sys.argv[1] == "--minibatch":
    steps = [minibatch_step_us(S) for S in (60, 300, 364, 368, 600)]
    print(json.dumps(steps), flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump({"minibatch_step": steps}, f, indent=1)
    sys.exit(0)
if len(sys.argv) > 2 and sys.argv[1] == "--kernels":
    env = states(4096)
    fn = calls(env)[0][sys.argv[2]]
    for _ in range(int(sys.argv[3]) if len(sys.argv) > 3 else 200):
        fn()
    torch.cuda.synchronize()
    env.close()
    sys.exit(0)

results = []


def save():
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(results, f, indent=1)


for E in (4096, 16384):
    env = states(E)
    fns, out, rest = calls(env)
    stride = out.shape[1]
    moved = (1280 + 4 * stride) * E
    moved_all = moved + 4 * (SPEC.nx * SPEC.ny + 64 + 4) * E
    row = {"envs": E, "stride": stride, "bytes_moved": moved, "bytes_moved_all": moved_all,
           "reps": REPS, "rounds": ROUNDS, "spec": SPEC.to_dict()}
    for name, fn in fns.items():
        row[name] = timed(fn, REPS)
    for name, nbytes in (("copy", moved), ("copy_all", moved_all)):
        src, dst = (torch.empty(nbytes // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        row[name] = timed(lambda: dst.copy_(src), REPS)
    state = env.export_state()
    row["torch"] = timed(lambda: torch_grid(env, state), 5, graph=False)
    fns["all"]()
    ref = torch_grid(env, state)
    torch.cuda.synchronize()
    width = SPEC.width(int(env.hwy_config.n_features))
    row["torch_max_abs_diff"] = float((ref - out[:, :width]).abs().max().item())
    assert row["torch_max_abs_diff"] <= 1e-5, row["torch_max_abs_diff"]
    c = rest["counts"].double().sum(0)
    row["present_others"], row["inside"], row["lost_cell"], row["outside"] = (float(x) for x in c)
    for k, floor in (("grid", "copy"), ("all", "copy_all")):
        row[f"{k}_over_{floor}"] = row[k]["median_us"] / row[floor]["median_us"]
        row[f"{k}_over_observe"] = row[k]["median_us"] / row["observe"]["median_us"]
    row["torch_over_grid"] = row["torch"]["median_us"] / row["grid"]["median_us"]
    print(json.dumps(row), flush=True)
    results.append(row)
    save()
    env.close()
roll = {"envs": 4096, "steps": 32, "hidden": 256, "plain": rollout_step_us(None),
        "grid": rollout_step_us(SPEC)}
roll["added_us_per_step"] = roll["grid"]["median_us"] - roll["plain"]["median_us"]
roll["added_share"] = roll["added_us_per_step"] / roll["plain"]["median_us"]
print(json.dumps(roll), flush=True)
results.append({"rollout": roll})
save()
assert all(math.isfinite(r["grid"]["median_us"]) for r in results if "grid" in r and "envs" in r and "stride" in r)
