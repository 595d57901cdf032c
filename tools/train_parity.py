#!/usr/bin/env python3
"""Reward-parity training runs: the reference's north-star cell on the MI355X env.

Runs `ExperimentRunner.launch` (experiments/runner.py, the reference's runner sequence,
/root/reference/experiments/runner.py:73-122) for the reference experiment
`<condition>_lr0.0003_hidden_dim256_clip_eps0.2_entropy_coef0.005_epochs8_batch_size64` at the
given seeds, 1500 episodes, eval every 50 episodes, and compares `final_reward` (mean of the last 10
evals, each the mean of 5 deterministic episodes seeded exp_seed+1000+k;
training/routine.py:181-186,292) with the reference's published value for the same seed
(artifacts/combined_validated_data-final-run.csv rows sorted_..._hidden_dim256_..._batch_size64:
seed 42 136.8270, 1042 127.8022, 2042 132.6172; mean 132.42).

Usage (GPU box):  python tools/train_parity.py --seeds 42 --out gpurun_out/train
    --num-envs 1   the reference's own loop (1 env, batch-1 select_action, 2048-step updates)
    --num-envs E   the lockstep loop (E envs, same hyperparameters, same episode budget)
    --num-envs E --rollout T --minibatches M
                   the many-env recipe: steps_per_update = E*T, M minibatches per epoch (the
                   bench's configs[1] recipe is E 4096, T 32, M 32), --episodes sets the budget
Under torchrun (--nproc-per-node N) each experiment spans the N GPUs with E envs per rank
(experiments/runner.py); rank 0 prints and writes the summary.
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "highway-rope-ppo_amd"))

# artifacts/combined_validated_data-final-run.csv, lr 3e-4 / h256 / clip .2 / ent .005 / 8 epochs /
# bs 64 (d_embed 4 for the PE conditions; the reference's own DistPE and RoPE rows coincide)
REFERENCE_FINAL = {
    "sorted": {42: 136.8270, 1042: 127.8022, 2042: 132.6172},
    "shuffled_rope": {42: 136.0069, 1042: 82.4615, 2042: 125.5533},
    "shuffled_distpe": {42: 136.0069, 1042: 82.4615, 2042: 125.5533},
    "shuffled_rankpe": {42: 83.2977, 1042: 119.7457, 2042: 119.0862},
}
# the hidden-dim sweep of the sorted condition (the same CSV, rows sorted_..._hidden_dim{384,512}_
# ..._batch_size64_d_embed4: d_embed is unused by the sorted condition)
REFERENCE_FINAL_HIDDEN = {
    ("sorted", 384): {42: 135.6114, 1042: 113.3057, 2042: 108.0399},
    ("sorted", 512): {42: 118.0541, 1042: 110.4705, 2042: 127.7685},
}


def reference_final(condition: str, hidden: int) -> dict:
    if hidden == 256:
        return REFERENCE_FINAL[condition]
    return REFERENCE_FINAL_HIDDEN.get((condition, hidden), {})


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--seeds", type=int, nargs="+", default=[42])
    p.add_argument("--episodes", type=int, default=1500)
    p.add_argument("--num-envs", type=int, default=1)
    p.add_argument("--out", default="gpurun_out/train")
    p.add_argument("--condition", default="sorted", choices=sorted(REFERENCE_FINAL))
    p.add_argument("--rollout", type=int, default=0,
                   help="rollout steps per env per update (0: ceil(2048 / num_envs))")
    p.add_argument("--minibatches", type=int, default=0, help="minibatches per epoch (0: n / 64)")
    p.add_argument("--eval-interval", type=int, default=50)
    p.add_argument("--lr", type=float, default=3e-4)
    p.add_argument("--epochs", type=int, default=8)
    p.add_argument("--hidden", type=int, default=256)
    p.add_argument("--obs-vehicles", type=int, default=0,
                   help="observation vehicles_count (0: HIGHWAY_CONFIG's 15); bench configs[2]/[4]: 30")
    p.add_argument("--order", choices=["sorted", "shuffled"], default=None,
                   help="observation order set explicitly, as bench.py does (default: make_env's own)")
    p.add_argument("--d-embed", type=int, default=4, help="PE d_embed / rotate_dim")
    p.add_argument("--grid", default=None, metavar="JSON",
                   help="train on this occupancy grid (extra['grid']: hwy.GridSpec's fields, or "
                        "true for the default)")
    args = p.parse_args()

    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    import torch

    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    results = []
    cond = {"sorted": Condition.SORTED, "shuffled_rope": Condition.SHUFFLED_ROPE,
            "shuffled_distpe": Condition.SHUFFLED_DISTPE,
            "shuffled_rankpe": Condition.SHUFFLED_RANKPE}[args.condition]
    d_embed = None if args.condition == "sorted" else args.d_embed
    obs_over = {}
    if args.obs_vehicles:
        obs_over["vehicles_count"] = args.obs_vehicles
    if args.order:
        obs_over["order"] = args.order
    for seed in args.seeds:
        name = (f"{args.condition}_lr{args.lr:g}_hidden_dim{args.hidden}_clip_eps0.2_"
                f"entropy_coef0.005_epochs{args.epochs}_batch_size64"
                + (f"_d_embed{d_embed}" if d_embed else "")
                + (f"_obs{args.obs_vehicles}" if args.obs_vehicles else "")
                + (f"_{args.order}" if args.order else "")
                + f"_seed{seed}" + (f"_envs{args.num_envs}" if args.num_envs > 1 else "")
                + (f"_T{args.rollout}_mb{args.minibatches}" if args.rollout else "")
                + ("_grid" if args.grid else ""))
        hp = ConditionHP(lr=args.lr, clip_eps=0.2, epochs=args.epochs, batch_size=64,
                         hidden_dim=args.hidden, d_embed=d_embed)
        hp.entropy_coef = 0.005
        if args.rollout:
            hp.steps_per_update = args.num_envs * args.rollout
        extra = {"log_interval": max(50, args.episodes // 200), "eval_interval": args.eval_interval}
        if args.num_envs > 1:
            extra["num_envs"] = args.num_envs
        if args.minibatches:
            extra["num_minibatches"] = args.minibatches
        if args.grid:
            extra["grid"] = json.loads(args.grid)
        exp = Experiment(name=name, condition=cond, hp=hp, seed=seed,
                         max_episodes=args.episodes, target_reward=130.0, extra=extra,
                         env_config_overrides={"observation": obs_over} if obs_over else {})
        run_dir = os.path.join(out, f"{args.condition}_seed{seed}")
        os.makedirs(run_dir, exist_ok=True)
        cwd = os.getcwd()
        os.chdir(run_dir)
        t0 = time.time()
        try:
            res = ExperimentRunner(HIGHWAY_CONFIG).launch(exp)
        finally:
            os.chdir(cwd)
        wall = time.time() - t0
        row = {"condition": args.condition, "seed": seed, "experiment": name, "status": res["status"], "wall_s": round(wall, 1),
               "num_envs": args.num_envs, "episodes": args.episodes, "rollout": args.rollout,
               "minibatches": args.minibatches, "eval_interval": args.eval_interval,
               "lr": args.lr, "epochs": args.epochs, "hidden_dim": args.hidden,
               "obs_vehicles": args.obs_vehicles or 15, "order": args.order or "make_env default",
               "d_embed": d_embed, "grid": res.get("metrics_history", {}).get("grid"),
               "device": torch.cuda.get_device_name(0) if torch.cuda.is_available() else "cpu"}
        if res["status"] == "COMPLETED":
            avg = res["avg_rewards"]
            hist = res["metrics_history"]
            ups = hist.get("policy_updates", [])
            row.update(final_reward=round(float(avg[-1]), 4), max_reward=round(float(max(avg)), 4),
                       evals=[round(float(x), 2) for x in hist.get("eval_rewards", [])],
                       eval_episodes=hist.get("eval_episode_numbers", []),
                       env_steps=int(sum(u.get("steps", 0) for u in ups)), updates=len(ups),
                       train_s=round(float(sum(u.get("time", 0.0) for u in ups)), 2))
            ref = reference_final(args.condition, args.hidden).get(seed)
            if ref is not None:
                row.update(reference_final_reward=ref,
                           delta=round(float(avg[-1]) - ref, 4))
        else:
            row["error"] = res.get("error_message")
        if res.get("rank", 0) != 0:
            continue
        row["world_size"] = int(os.environ.get("WORLD_SIZE", "1"))
        results.append(row)
        print(json.dumps(row), flush=True)
        with open(os.path.join(out, "summary.jsonl"), "a") as f:
            f.write(json.dumps(row) + "\n")
    done = [r for r in results if "final_reward" in r]
    if done:
        mean = sum(r["final_reward"] for r in done) / len(done)
        rf = reference_final(args.condition, args.hidden)
        refs = [rf[r["seed"]] for r in done if r["seed"] in rf]
        print(json.dumps({"condition": args.condition, "mean_final_reward": round(mean, 4),
                          "reference_mean": round(sum(refs) / len(refs), 4) if refs else None,
                          "n": len(done)}), flush=True)


if __name__ == "__main__":
    main()
