"""Times hwy_lidar beside its yardsticks in one run (development aid): probe_lidar.py [out.json]

  a  observe  HighwayVecEnv.observe_into with `obs` only (hwy_observe, one launch)
  b  grid     grid_into with `out` only, the default GridSpec (hwy_grid, one launch)
  c  lidar    lidar_into with `out` only, for 16 x 1, 64 x 1 and 64 x 8 rays (cells x sub), 60 m,
              normalised, with the ego tail, unaligned, no sensor errors
  d  all      the same with every output: out, hit_vehicle, seen, counts
  e  copy     torch's copy_ of a buffer half as large as what (c) reads and writes per env
              (1,536 B of state + 4 stride B of row), so that it moves as many bytes: the floor
  f  torch    the same rule restated in torch ops on the exported state ([E, rays, 64] slab tests,
              eager launches and all; the share of cells whose distance differs from (c)'s by more
              than 1e-3 of the range is booked: the device's sin / cos differ from torch's, and a
              ray that grazes a corner may hit in one and miss in the other)

at E = 4,096 and 16,384 envs (the shipped config: N 15, F 4, 50 other vehicles), on states a few
steps after the reset, with every env's ego moved 6 m behind a car of its traffic (a natural ego
drives alone and a lidar would return nothing).  (a) to (e) are captured as a HIP graph of REPS
back-to-back calls, warmed, and replayed ROUNDS times between two events; the figure is the median
replay over REPS, in microseconds per call.  (f) is timed likewise, eagerly.

Then the captured rollout of training (LockstepRollout, 4,096 envs x 32 steps, H 256) on the
Kinematics rows, on the default grid and on the default lidar: microseconds per rollout step.

probe_lidar.py --minibatch OUT.json: the fused minibatch step at S = 36 (the default lidar), 60
(the Kinematics rows), 132 (64 cells) and 364 (the default grid), H 256, 4,096 rows per minibatch,
by tools/wide_step_timing.py's protocol.  HWY_LIB overrides the library."""
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
from hwy import GridSpec, LidarSpec, _abi
from hwy.vec_env import HighwayVecEnv
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS, REPS = 15, 50
RAYS = ((16, 1), (64, 1), (64, 8))
GRID = GridSpec()


def timed(fn, reps, graph=True, rounds=ROUNDS):
    """Median microseconds per call of fn over `rounds` runs of `reps` calls (one replayed graph
    of them, or, graph=False, the eager calls)."""
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
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        us.append(e0.elapsed_time(e1) / reps * 1e3)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us)}


def states(E, steps=3):
    """an env a few steps after the reset, every ego moved 6 m behind and 0.7 m beside vehicle 1"""
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(steps):
        env.step((torch.rand(E, 2, device=dev, generator=gen) - 0.5) * 0.6)
    st = env.export_state()
    x, y = st[_abi.F_X].view(torch.float32), st[_abi.F_Y].view(torch.float32)
    x[:, 0] = x[:, 1] - 6.0
    y[:, 0] = y[:, 1] + 0.7
    env.import_state(st)
    return env


def torch_lidar(env, state, spec):
    """the rule in torch ops on an exported state [NFIELDS, E, 64] (int32): [E, 2 * cells + F]"""
    cfg = env.hwy_config
    E, V = state.shape[1], cfg.vehicles_count + 1
    n, inf = spec.cells * spec.sub, float("inf")
    f = lambda k: state[k].view(torch.float32)  # noqa: E731
    x, y, h, spd = f(_abi.F_X), f(_abi.F_Y), f(_abi.F_HEADING), f(_abi.F_SPEED)
    body = (state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    body[:, V:] = False
    body[:, 0] = False
    theta = (torch.arange(n, device=dev, dtype=torch.float32) + (0.5 - 0.5 * spec.sub)) * (
        2.0 * math.pi / n)
    theta = theta[None, :] + (h[:, :1] if spec.align else 0.0)
    dx, dy = torch.cos(theta)[:, :, None], torch.sin(theta)[:, :, None]
    ck, sk = torch.cos(h)[:, None, :], torch.sin(h)[:, None, :]
    ox, oy = (x[:, :1] - x)[:, None, :], (y[:, :1] - y)[:, None, :]
    ou, ow = ox * ck + oy * sk, oy * ck - ox * sk
    du, dw = dx * ck + dy * sk, dy * ck - dx * sk

    def axis(o, d, H):
        t1, t2 = (-H - o) / d, (H - o) / d
        par, ins = d == 0, o.abs() <= H
        lo = torch.where(par, torch.where(ins, -inf, inf), torch.minimum(t1, t2))
        hi = torch.where(par, torch.where(ins, inf, -inf), torch.maximum(t1, t2))
        return lo, hi

    lo_u, hi_u = axis(ou, du, 2.5)
    lo_w, hi_w = axis(ow, dw, 1.0)
    t_in, t_out = torch.maximum(lo_u, lo_w), torch.minimum(hi_u, hi_w)
    d = t_in.clamp(min=0.0)
    ok = body[:, None, :] & (t_in <= t_out) & (t_out >= 0) & (d <= spec.range_m)
    ray_d, ray_k = torch.where(ok, d, inf).min(2)                       # [E, n]
    cell_d, cell_j = ray_d.view(E, spec.cells, spec.sub).min(2)        # [E, cells]
    ray = torch.arange(spec.cells, device=dev)[None, :] * spec.sub + cell_j
    k = ray_k.gather(1, ray)
    wdx = dx[:, :, 0].expand(E, n).gather(1, ray)
    wdy = dy[:, :, 0].expand(E, n).gather(1, ray)
    vx, vy = spd * torch.cos(h), spd * torch.sin(h)
    vel = (vx.gather(1, k) - vx[:, :1]) * wdx + (vy.gather(1, k) - vy[:, :1]) * wdy
    hit = torch.isfinite(cell_d)
    dist = torch.where(hit, cell_d, spec.range_m)
    vel = torch.where(hit, vel, 0.0)
    if spec.normalize:
        dist, vel = dist / spec.range_m, vel / spec.speed_scale
    tail = []
    for j in range(cfg.n_features):
        v = {1: x, 2: y, 3: vx, 4: vy}[int(cfg.feature_ids[j])][:, 0]
        lo, hi = cfg.features_range[j][0], cfg.features_range[j][1]
        tail.append((-1.0 + (v - lo) * 2.0 / (hi - lo)).clamp(-1.0, 1.0))
    return torch.cat([torch.stack([dist, vel], 2).reshape(E, 2 * spec.cells),
                      torch.stack(tail, 1)], 1)


def rollout_step_us(kind, spec, E=4096, T=32):
    """Median microseconds per step of the replayed rollout graph of training; kind: None (the
    Kinematics rows), "grid" or "lidar" """
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    sd = (env.obs_rows * env.obs_features if kind is None
          else spec.stride(int(env.hwy_config.n_features)))
    agent = PPOAgent(sd, 2, lr=3e-4, epochs=2, hidden_dim=256, device=dev, num_minibatches=4, seed=5)
    buf = RolloutBuffer(T, E, sd, 2, dev)
    obs, _ = env.reset()
    if kind is None:
        buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, env, buf, use_graph=True, **({} if kind is None else {kind: spec}))
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
    for _ in range(2):  # capture, then warm
        F.run(s, z, lp, adv, ret, perm)
    torch.cuda.synchronize()
    F.epoch_events = []
    for _ in range(updates):
        F.run(s, z, lp, adv, ret, perm)
    torch.cuda.synchronize()
    us = [a.elapsed_time(b) * 1e3 / nmb for a, b in F.epoch_events]
    return {"S": S, "H": H, "rows": B, "general_path": F._tile_off is not None,
            "epochs_timed": len(us), "median_us": statistics.median(us), "min_us": min(us),
            "max_us": max(us)}


if len(sys.argv) > 2 and sys.argv[1] == "--minibatch":
    steps = [minibatch_step_us(S) for S in (36, 60, 132, 364)]
    print(json.dumps(steps), flush=True)
    with open(sys.argv[2], "w") as f:
        json.dump({"minibatch_step": steps}, f, indent=1)
    sys.exit(0)

results = []


def save():
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            json.dump(results, f, indent=1)


for E in (4096, 16384):
    env = states(E)
    F = int(env.hwy_config.n_features)
    obs = torch.empty(E, env.obs_rows, env.obs_features, device=dev)
    gout = torch.empty(E, GRID.stride(F), device=dev)
    row = {"envs": E, "reps": REPS, "rounds": ROUNDS,
           "observe": timed(lambda: env.observe_into(obs=obs), REPS),
           "grid": timed(lambda: env.grid_into(GRID, out=gout), REPS)}
    state = env.export_state()
    for cells, sub in RAYS:
        spec = LidarSpec(cells=cells, sub=sub)
        stride = spec.stride(F)
        out = torch.empty(E, stride, device=dev)
        rest = dict(hit_vehicle=torch.empty(E, cells, dtype=torch.int32, device=dev),
                    seen=torch.empty(E, 64, device=dev),
                    counts=torch.empty(E, 4, dtype=torch.int32, device=dev))
        moved = (1536 + 4 * stride) * E
        src, dst = (torch.empty(moved // 2, dtype=torch.uint8, device=dev) for _ in range(2))
        r = {"spec": spec.to_dict(), "stride": stride, "bytes_moved": moved,
             "lidar": timed(lambda: env.lidar_into(spec, out=out), REPS),
             "all": timed(lambda: env.lidar_into(spec, out=out, **rest), REPS),
             "copy": timed(lambda: dst.copy_(src), REPS),
             "torch": timed(lambda: torch_lidar(env, state, spec), 3, graph=False, rounds=5)}
        env.lidar_into(spec, out=out, **rest)
        ref = torch_lidar(env, state, spec)
        torch.cuda.synchronize()
        diff = (ref[:, 0:2 * cells:2] - out[:, 0:2 * cells:2]).abs()
        r["torch_cells_off_share"] = float((diff > 1e-3).float().mean().item())
        r["torch_median_abs_diff"] = float(diff.median().item())
        assert r["torch_cells_off_share"] <= 1e-3, r
        c = rest["counts"].double().mean(0)
        r["bodies_per_env"], r["seen_per_env"], r["returns_per_env"] = (float(v) for v in c[:3])
        for k in ("observe", "grid"):
            r[f"lidar_over_{k}"] = r["lidar"]["median_us"] / row[k]["median_us"]
        r["lidar_over_copy"] = r["lidar"]["median_us"] / r["copy"]["median_us"]
        r["torch_over_lidar"] = r["torch"]["median_us"] / r["lidar"]["median_us"]
        row[f"{cells}x{sub}"] = r
    print(json.dumps(row), flush=True)
    results.append(row)
    save()
    env.close()
roll = {"envs": 4096, "steps": 32, "hidden": 256, "plain": rollout_step_us(None, None),
        "grid": rollout_step_us("grid", GRID), "lidar": rollout_step_us("lidar", LidarSpec())}
for k in ("grid", "lidar"):
    roll[f"{k}_added_us_per_step"] = roll[k]["median_us"] - roll["plain"]["median_us"]
    roll[f"{k}_added_share"] = roll[f"{k}_added_us_per_step"] / roll["plain"]["median_us"]
print(json.dumps(roll), flush=True)
results.append({"rollout": roll})
save()
