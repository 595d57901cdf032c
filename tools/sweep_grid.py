#!/usr/bin/env python3
"""One condition's reference hyper-parameter grid, run as grouped experiments.

The reference's define_experiments crosses hidden_dim {128, 256, 384} x epochs {6, 8, 10} x
batch_size {32, 64} (and lr; 3e-4 here): 18 cells, each with the seeds of --seeds, at the
reference's update statistics (E = 16 envs x T = 128 steps = 2,048 samples per update, so 64 or 32
minibatches per epoch) to --episodes episodes, evaluation every 50.  Two ways to run them:

  --by-class   one ExperimentRunner.launch_batch per (epochs, batch_size) class: six batches of
               three cells, which share their minibatch schedule and differ in hidden width only
               (hwy_ppo_mixed_*).  192 + 256 + 320 + 384 + 512 + 640 = 2,304 grouped minibatch
               steps per update, one class after another.
  --one-batch  all 18 cells as ONE launch_batch: every cell keeps its own minibatch schedule
               inside shared launches (hwy_ppo_sched_*), 640 grouped steps per update.

Every experiment is bit-identical to its solo launch() either way, so the two modes must agree
in every final_reward.  Writes OUT/sweep.json: per mode the wall time and each experiment's
final_reward, and, when both modes ran (or --compare names the other mode's sweep.json), whether
they are equal experiment by experiment.  No child process is started.

With neither flag --one-batch runs (on one MI355X it took 41.6 s against --by-class's 84.0 s for
the sorted condition, 3 seeds, 1,500 episodes: profiles/r8/grid/).

    python tools/sweep_grid.py --out artifacts/sweep_grid [--by-class] [--one-batch]
        [--condition sorted] [--seeds 42 1042 2042] [--episodes 1500] [--compare OTHER/sweep.json]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "highway-rope-ppo_amd"))

HIDDEN, EPOCHS, BATCH = (128, 256, 384), (6, 8, 10), (32, 64)
E, T = 16, 128


def _cells(args):
    """{(epochs, batch_size): [cell, ...]}, a cell being one hidden width's experiments (one per
    seed)."""
    from experiments.config import Condition, ConditionHP, Experiment

    cond = {"sorted": Condition.SORTED, "shuffled_rope": Condition.SHUFFLED_ROPE,
            "shuffled_distpe": Condition.SHUFFLED_DISTPE,
            "shuffled_rankpe": Condition.SHUFFLED_RANKPE}[args.condition]
    d_embed = None if args.condition == "sorted" else 4
    classes = {}
    for ep in EPOCHS:
        for bs in BATCH:
            for H in HIDDEN:
                exps = []
                for seed in args.seeds:
                    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=ep, batch_size=bs, hidden_dim=H,
                                     d_embed=d_embed)
                    hp.entropy_coef = 0.005
                    hp.steps_per_update = E * T
                    name = (f"{args.condition}_lr0.0003_hidden_dim{H}_epochs{ep}_batch_size{bs}"
                            + (f"_d_embed{d_embed}" if d_embed else "") + f"_seed{seed}")
                    extra = {"log_interval": max(50, args.episodes // 200), "eval_interval": 50,
                             "num_envs": E}
                    exps.append(Experiment(name=name, condition=cond, hp=hp, seed=seed,
                                           max_episodes=args.episodes, target_reward=130.0,
                                           extra=extra, env_config_overrides={}))
                classes.setdefault((ep, bs), []).append(exps)
    return classes


def _run(mode, classes, work):
    """One mode: its launch_batch calls, timed together.  Returns the mode's report entry."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    units = ([[c for cells in classes.values() for c in cells]] if mode == "one_batch"
             else list(classes.values()))
    finals, failed = {}, {}
    os.makedirs(work, exist_ok=True)
    cwd = os.getcwd()
    os.chdir(work)  # the runner writes its logs, checkpoints and artifacts under the cwd
    t0 = time.time()
    try:
        for cells in units:
            for exps, results in zip(cells, ExperimentRunner(HIGHWAY_CONFIG).launch_batch(cells)):
                for e, res in zip(exps, results):
                    if res["status"] == "COMPLETED":
                        finals[e.name] = float(res["avg_rewards"][-1])
                    else:
                        failed[e.name] = res.get("error_message")
    finally:
        os.chdir(cwd)
    return {"wall_s": round(time.time() - t0, 1), "batches": len(units),
            "experiments": len(finals) + len(failed), "final_reward": finals, "failed": failed}


def _equal(a: dict, b: dict) -> dict:
    names = sorted(set(a) | set(b))
    differ = [n for n in names if a.get(n) != b.get(n)]
    return {"compared": len(names), "equal": len(names) - len(differ), "all_equal": not differ,
            "differ": differ}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default="artifacts/sweep_grid")
    p.add_argument("--work", default=None, help="where the runner writes logs, checkpoints and "
                                                "artifacts (default: OUT/work)")
    p.add_argument("--by-class", action="store_true",
                   help="one launch_batch per (epochs, batch_size) class")
    p.add_argument("--one-batch", action="store_true",
                   help="all 18 cells as one launch_batch (the default: measured 2x faster, "
                        "profiles/r8/grid/)")
    p.add_argument("--condition", default="sorted",
                   choices=["sorted", "shuffled_rope", "shuffled_distpe", "shuffled_rankpe"])
    p.add_argument("--seeds", type=int, nargs="+", default=[42, 1042, 2042])
    p.add_argument("--episodes", type=int, default=1500)
    p.add_argument("--compare", default=None,
                   help="a sweep.json of the other mode: final_reward is compared against it")
    args = p.parse_args()
    modes = [m for m, on in (("by_class", args.by_class), ("one_batch", args.one_batch)) if on]
    modes = modes or ["one_batch"]
    out = os.path.abspath(args.out)
    os.makedirs(out, exist_ok=True)
    work = os.path.abspath(args.work) if args.work else os.path.join(out, "work")
    classes = _cells(args)
    report = {"recipe": {"condition": args.condition, "num_envs": E, "rollout": T, "lr": 3e-4,
                         "hidden_dim": HIDDEN, "epochs": EPOCHS, "batch_size": BATCH,
                         "episodes": args.episodes, "eval_interval": 50, "seeds": args.seeds},
              "modes": {}}
    for mode in modes:
        report["modes"][mode] = _run(mode, classes, os.path.join(work, mode))
        print(json.dumps({"mode": mode, **{k: v for k, v in report["modes"][mode].items()
                                            if k not in ("final_reward",)}}), flush=True)
    if len(modes) == 2:
        report["equal_final_reward"] = _equal(report["modes"]["by_class"]["final_reward"],
                                              report["modes"]["one_batch"]["final_reward"])
    elif args.compare:
        other = json.load(open(args.compare))["modes"]
        theirs = next(v for k, v in other.items() if k != modes[0] or len(other) == 1)
        report["equal_final_reward"] = dict(
            _equal(report["modes"][modes[0]]["final_reward"], theirs["final_reward"]),
            against=os.path.relpath(args.compare, out))
    if "equal_final_reward" in report:
        print(json.dumps({"equal_final_reward": {k: v for k, v in
                                                 report["equal_final_reward"].items()}}),
              flush=True)
    with open(os.path.join(out, "sweep.json"), "w") as f:
        json.dump(report, f, indent=1)
    failed = any(m["failed"] for m in report["modes"].values())
    return 1 if failed or not report.get("equal_final_reward", {}).get("all_equal", True) else 0


if __name__ == "__main__":
    sys.exit(main())
