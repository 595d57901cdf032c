#!/usr/bin/env python3
"""Timing of the PPO minibatch step at state rows wider than 256 floats (profiles/r9/wide/).
Run it from the root of the tree to measure, once per tree (it imports that tree's package and
library), so the same script times a commit and its parent in one job:

    python tools/wide_step_timing.py TAG OUT.json            the steps and the sweep shape
    python tools/wide_step_timing.py TAG OUT.json --tiles    ppo_rows around S = 256 at large B

 - the minibatch step (forward/backward + optimizer, captured epoch graph, HIP events around every
   epoch: FusedPPO.epoch_events) at S 600 / H 256 / B 4096 and S 1024 / H 512 / B 4096;
 - the sweep shape S 300 / H 256 / B 64, G = 30 learners: all learners' steps of one epoch as
   solo calls in ONE captured graph, and (where the library groups them) as grouped steps;
 - per-kernel times (hwy_ppo_time_kernels) where the shape takes the fused path;
 - --tiles: the step just below and just above S = 256 at 8,192 - 32,768 rows (the narrow shape
   takes the 32- / 64-row tiles, the wide one the 16-row tile).
"""
import json
import os
import sys

ROOT = os.getcwd()
for p in (os.path.join(ROOT, "highway-rope-ppo_amd"), ROOT):
    sys.path.insert(0, p)

import torch  # noqa: E402

from hwy.ppo_native import FusedPPO, GroupStep  # noqa: E402
from ppo.agent import PPOAgent  # noqa: E402

DEV = torch.device("cuda", 0)
TAG, OUT = sys.argv[1], sys.argv[2]
res = {"tag": TAG, "device": torch.cuda.get_device_name(0)}


def agent(S, H, epochs, seed=0):
    torch.manual_seed(seed)
    return PPOAgent(S, 2, lr=3e-4, epochs=epochs, hidden_dim=H, device=DEV, backend="hip")


def data(n, S, ag, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randn(n, S, device=DEV, generator=g)
    with torch.no_grad():
        _, z, lp, v = ag.actor_critic.act(s, generator=g)
    lp = lp + 0.05 * torch.randn(n, device=DEV, generator=g)
    adv = torch.randn(n, device=DEV, generator=g)
    ret = v + torch.randn(n, device=DEV, generator=g)
    perm = torch.randperm(n, device=DEV, generator=g)
    return s, z.contiguous(), lp.contiguous(), adv, ret, perm


def median(xs):
    xs = sorted(xs)
    return xs[len(xs) // 2]


def solo_step(S, H, B, nmb=4, epochs=8, updates=3):
    ag = agent(S, H, epochs)
    s, z, lp, adv, ret, perm = data(B * nmb, S, ag)
    F = FusedPPO(ag, B, nmb, use_graphs=True)
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())  # capture + warm-up
    torch.cuda.synchronize()
    F.epoch_events = []
    a2, r2, p2 = adv.clone(), ret.clone(), perm.clone()
    F.run(s, z, lp, a2, r2, p2)
    torch.cuda.synchronize()
    F.epoch_events = []
    for _ in range(updates):
        F.run(s, z, lp, a2, r2, p2)
    torch.cuda.synchronize()
    per_step = [a.elapsed_time(b) * 1e3 / nmb for a, b in F.epoch_events]
    out = {"S": S, "H": H, "B": B, "fused": F._tile_off is not None,
           "epochs_timed": len(per_step), "step_us_median": median(per_step),
           "step_us_min": min(per_step), "step_us_max": max(per_step)}
    if F._tile_off is not None:
        out["kernels_us"] = F.time_kernels(16)
    return out


if "--tiles" in sys.argv:
    res["tiles"] = [solo_step(S, H, B, nmb=2, epochs=4, updates=2)
                    for S, H, B in [(256, 256, 8192), (272, 256, 8192), (256, 256, 16384),
                                    (272, 256, 16384), (256, 256, 32768), (272, 256, 32768),
                                    (256, 128, 16384), (272, 128, 16384)]]
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1)
    sys.exit(0)

res["solo"] = [solo_step(600, 256, 4096), solo_step(1024, 512, 4096), solo_step(300, 256, 64),
               solo_step(256, 256, 4096), solo_step(512, 256, 4096), solo_step(1024, 256, 4096),
               solo_step(256, 512, 4096), solo_step(512, 512, 4096)]


def replay_us(g, reps=20):
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    t = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            g.replay()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) * 1e3 / reps)
    return median(t), min(t), max(t)


def sweep(S=300, H=256, B=64, G=30, nmb=4):
    ags = [agent(S, H, 1, seed=g) for g in range(G)]
    ds = [data(B * nmb, S, ag, seed=100 + g) for g, ag in enumerate(ags)]
    Fs = [FusedPPO(ag, B, nmb, use_graphs=False) for ag in ags]
    for F in Fs:  # the replays below never reset counters[1]: room for every metrics row
        F.metrics = torch.zeros(8192, 6, device=DEV)
    args = [[F._args(d[0], d[1], d[2], d[3], d[4], d[5].data_ptr() + i * B * 8) for i in range(nmb)]
            for F, d in zip(Fs, ds)]
    for F, a in zip(Fs, args):
        F.sync_params(a[0])
    torch.cuda.synchronize()
    out = {"S": S, "H": H, "B": B, "G": G, "nmb": nmb, "fused": Fs[0]._tile_off is not None}
    side = torch.cuda.Stream()

    def capture(fn):
        g = torch.cuda.CUDAGraph()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            fn()  # warm-up outside the capture
            torch.cuda.synchronize()
            with torch.cuda.graph(g, stream=side):
                fn()
        torch.cuda.current_stream().wait_stream(side)
        return g

    def solo_all():
        for i in range(nmb):
            for F, a in zip(Fs, args):
                F._fwd_bwd(a[i])
                F._opt(a[i])

    g = capture(solo_all)
    m, lo, hi = replay_us(g)
    out["solo_graph_us_per_minibatch_of_all_learners"] = {"median": m / nmb, "min": lo / nmb,
                                                           "max": hi / nmb}
    try:
        gs = GroupStep(Fs)
        gs.prepare(args)

        def grouped():
            for i in range(nmb):
                gs.step(i)

        g2 = capture(grouped)
        m, lo, hi = replay_us(g2)
        out["grouped_graph_us_per_minibatch_of_all_learners"] = {"median": m / nmb,
                                                                  "min": lo / nmb, "max": hi / nmb}
        out["grouped_launches_per_step"] = gs.launches_per_step
    except (ValueError, RuntimeError) as e:
        out["grouped_error"] = str(e)[:200]
    return out


res["sweep"] = sweep()
with open(OUT, "w") as f:
    json.dump(res, f, indent=1)
print(json.dumps(res))
