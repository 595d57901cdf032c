"""Times hwy_render beside two yardsticks in one run (development aid): probe_render.py [out.json]

  render   HighwayVecEnv.render into a fixed buffer (hwy_render, one launch)
  fill     torch's fill_ of the same buffer: the write floor
  torch    the frame rule restated with plain torch ops on the GPU (first shape only): what a
           user would otherwise write

at 16 frames of 600x150x3 (an evaluation batch) and 4,096 frames of 64x128x1 (a grayscale view of
a training batch), on states a few steps after the reset.  Each is captured as a HIP graph of
REPS back-to-back calls, warmed, and replayed ROUNDS times between two events; the figure is the
median replay over REPS, in microseconds per call, and the bytes written over it.  HWY_LIB
overrides the library."""
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
from hwy.vec_env import HighwayVecEnv
from utils.graphs import capture

dev = torch.device("cuda", 0)
ROUNDS = 15


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


def torch_render(state, lanes, W, H, scaling, centering, out):
    """The frame rule of include/hwy.h in float32 torch ops, all envs at once, into out
    [E, H, W, 3] uint8 (no shade)."""
    f32 = lambda f: state[f].view(torch.float32)  # noqa: E731
    x, y, hd, flags = f32(0), f32(1), f32(2), state[11]
    E = x.shape[0]
    xe, ye = x[:, :1, None], y[:, :1, None]                      # [E, 1, 1]
    px = (((torch.arange(W, device=dev) + 0.5) - centering[0] * W) / scaling).view(1, 1, W)
    py = (((torch.arange(H, device=dev) + 0.5) - centering[1] * H) / scaling).view(1, H, 1)
    in_x = (-xe <= px) & (px <= 10000.0 - xe)

    def paint(mask, colour):  # masked_fill_: no host synchronisation, so the graph can hold it
        for k in range(3):
            out[..., k].masked_fill_(mask, colour[k])

    out.fill_(60)
    paint(in_x & (-2.0 - ye <= py) & (py < (4.0 * lanes - 2.0) - ye), (100, 100, 100))
    u = px + (xe - 8.0 * torch.floor(xe / 8.0))
    dash = u - 8.0 * torch.floor(u / 8.0) < 3.0
    for k in range(lanes + 1):
        on = in_x & ((py - ((4.0 * k - 2.0) - ye)).abs() <= 0.15)
        if 0 < k < lanes:
            on = on & dash
        paint(on, (255, 255, 255))
    sh, ch = torch.sin(hd), torch.cos(hd)
    for v in list(range(1, 64)) + [0]:
        dx = px - (x[:, v] - x[:, 0]).view(E, 1, 1)
        dy = py - (y[:, v] - y[:, 0]).view(E, 1, 1)
        c, s = ch[:, v].view(E, 1, 1), sh[:, v].view(E, 1, 1)
        cov = ((dx * c + dy * s).abs() <= 2.5) & ((dy * c - dx * s).abs() <= 1.0)
        if v:
            cov = cov & ((flags[:, v] & 4) != 0).view(E, 1, 1)
        crashed = ((flags[:, v] & 1) != 0).view(E, 1, 1)
        paint(cov & ~crashed, (100, 200, 255) if v else (50, 200, 0))
        paint(cov & crashed, (255, 100, 100))
    return out


def states(E, steps=3):
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=dev, autoreset=True, seed_base=5)
    env.reset()
    gen = torch.Generator(device=dev).manual_seed(0)
    for _ in range(steps):
        env.step((torch.rand(E, 2, device=dev, generator=gen) - 0.5) * 0.6)
    return env


results = []
for E, W, H, C, reps, with_torch in ((16, 600, 150, 3, 50, True), (4096, 64, 128, 1, 50, False)):
    env = states(E)
    out = torch.empty(E, H, W, C, dtype=torch.uint8, device=dev)
    nbytes = out.numel()
    row = {"frames": E, "width": W, "height": H, "channels": C, "bytes": nbytes, "reps": reps,
           "rounds": ROUNDS,
           "render": timed(lambda: env.render(width=W, height=H, channels=C, out=out), reps),
           "fill": timed(lambda: out.fill_(60), reps)}
    for k in ("render", "fill"):
        row[k]["GB_per_s"] = nbytes / row[k]["median_us"] * 1e-3
    row["render_over_fill"] = row["render"]["median_us"] / row["fill"]["median_us"]
    if with_torch:
        st = env.export_state()
        ref = torch.empty_like(out)
        lanes = int(env.hwy_config.lanes_count)
        # a graph of the restatement alone is ~700 launches: one call per replay
        row["torch"] = timed(lambda: torch_render(st, lanes, W, H, 5.5, (0.3, 0.5), ref), 1)
        row["torch_over_render"] = row["torch"]["median_us"] / row["render"]["median_us"]
        torch_render(st, lanes, W, H, 5.5, (0.3, 0.5), ref)
        env.render(width=W, height=H, channels=C, out=out)
        row["pixels_differing_from_torch_share"] = float(
            (ref != out).any(-1).double().mean().item())
    print(json.dumps(row), flush=True)
    results.append(row)
    env.close()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(results, f, indent=1)
assert all(math.isfinite(r["render"]["median_us"]) for r in results)
