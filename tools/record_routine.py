#!/usr/bin/env python3
"""Record what the training routine's entry points refuse and compute, as JSON, so that two
versions of the Python tree (over the same libhwy.so) can be compared value for value.

    python tools/record_routine.py --refusals --out refusals.json [--pkg DIR]
    python tools/record_routine.py --runs --out runs.json [--pkg DIR]

``--pkg`` is the package directory to import (default: this tree's highway-rope-ppo_amd).

--refusals (no device): train_with_experiment_name on stub env and agent objects for every run
option alone and every pair, on a one-env and a vector stub, with and without a process group on
the agent, with a logger whose first ``info`` raises -- the record is the exception's type and
text, or "reached the run"; the same option values through ExperimentRunner.check_batch (cells of
two experiments), LockstepRollout(...) on stubs, evaluate(...) and visualize_agent(...).  The stubs
carry what either side of a comparison may look for (the per-kind ``*_into`` methods and the view
seam's ``view_into`` / ``view_width``), so the same tool text runs against both trees.  The
file lists each distinct outcome once, by number (``outcomes``); every other section maps an
option set to its outcomes' numbers, one per entry of the section's ``axes``.

--runs (one GPU): a mini experiment (4 envs x 16 steps per update, 12 episodes of at most 12
steps, hidden 64, an evaluation every 4 episodes, seed 42) launched under each option set and as
groups of two seeds, and direct calls of evaluate, safety_profile, shield_profile, attribution and
visualize_agent on one env and agent; per run the rewards, the metrics without their wall times,
the summary CSV row and the SHA-256 of the final weights.
"""

from __future__ import annotations

import argparse
import csv
import hashlib
import itertools
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

VALUES = {"episode_schedule": "reference", "episode_stats": True, "safety_stats": True,
          "truncation": "bootstrap", "attribution": True, "eval_orders": ["shuffled"],
          "eval_sensors": {"a": {}}, "sensor": {}, "eval_shields": {"a": None}, "shield": {},
          "grid": True, "lidar": True, "target_kl": 0.02, "lr_anneal_updates": 10}
CONTROLS = ("target_kl", "lr_anneal_updates")
ROLLOUT_OPTIONS = ("episode_schedule", "episode_stats", "safety_stats", "truncation", "sensor",
                   "shield", "grid", "lidar")


class Reached(Exception):
    """raised by the stub logger: the argument checks let the call through"""


class Stub:
    """an env or agent with just the attributes the argument checks read"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.unwrapped = self


class StopLogger:
    def info(self, *a, **kw):
        raise Reached()


def outcome(fn, reached="reached the run"):
    try:
        fn()
    except Reached:
        return reached
    except Exception as e:  # the record is whatever the call does
        return [type(e).__name__, str(e)]
    return "returned"


def subsets(names, upto=2):
    for r in range(upto + 1):
        for c in itertools.combinations(names, r):
            yield c


def tag(names, **where):
    return "+".join(names or ("none",)) + "".join(f" {k}={v}" for k, v in where.items())


def mini_exp(seed, name, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps
    return Experiment(name=f"rec_{name}_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=12, target_reward=1e9,
                      extra={"num_envs": 4, "eval_interval": 4, "log_interval": 50, **extra},
                      env_config_overrides={"max_episode_steps": 12})


def refusals():
    import torch

    from experiments.runner import ExperimentRunner
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import evaluate, train_with_experiment_name, visualize_agent

    rec = {"train": {}, "check_batch": {}, "rollout": {}, "evaluate": {}, "visualize": {}}
    for names in subsets(VALUES):
        kw = {n: VALUES[n] for n in names if n not in CONTROLS}
        controls = {n: VALUES[n] for n in names if n in CONTROLS}
        for vector in (False, True):
            for dist in (False, True):
                env = Stub(is_vector_env=vector)
                agent = Stub(**controls, **({"_dist": object()} if dist else {}))
                rec["train"][tag(names, vector=vector, dist=dist)] = outcome(
                    lambda: train_with_experiment_name(env, agent, logger=StopLogger(), **kw))
        cell = [mini_exp(s, "g", **{n: VALUES[n] for n in names}) for s in (42, 1042)]
        rec["check_batch"][tag(names)] = outcome(
            lambda: ExperimentRunner.check_batch([cell], own_schedules=True))

    cpu = torch.device("cpu")
    bufs = {"plain": lambda: RolloutBuffer(2, 2, 4, 2, cpu),
            "full": lambda: RolloutBuffer(2, 2, 4, 2, cpu, episode_stats=True, safety_stats=True,
                                          truncation_bootstrap=True, shield=True)}
    # every launch a rollout's constructor may issue is there and not callable, under the names
    # of the per-kind methods and of the view seam; "vec" also answers the constructor's questions
    launches = dict(sense_into=None, grid_into=None, lidar_into=None, view_into=None)
    envs = {"bare": lambda: Stub(sense_into=None, view_into=None),
            "vec": lambda: Stub(shield_into=None, hwy_config=Stub(n_features=4), **launches,
                                view_width=lambda spec: spec.stride(4))}
    for names in subsets(ROLLOUT_OPTIONS):
        kw = {n: VALUES[n] for n in names}
        for b, e in itertools.product(bufs, envs):
            rec["rollout"][tag(names, buf=b, env=e)] = outcome(
                lambda: LockstepRollout(Stub(), envs[e](), bufs[b](), **kw))

    views = {"order": "shuffled", "sensor": {}, "shield": {}, "grid": True, "lidar": True}
    for names in subsets(views, upto=5):
        kw = {n: views[n] for n in names}
        for vector in (False, True):
            rec["evaluate"][tag(names, vector=vector)] = outcome(
                lambda: evaluate(Stub(is_vector_env=vector), Stub(), **kw))

    for attr, tint, sensor, grid, lidar in itertools.product(
            (None, "value"), (None, "ttc", "hidden", "lidar"), (None, {}), (None, True),
            (None, True)):
        rec["visualize"][f"attribution={attr} tint={tint} sensor={sensor} grid={grid} "
                         f"lidar={lidar}"] = outcome(
            lambda: visualize_agent(Stub(is_vector_env=True), Stub(), num_episodes=1,
                                    logger=StopLogger(), attribution=attr, tint=tint,
                                    sensor=sensor, grid=grid, lidar=lidar),
            reached="reached the episodes")
    return rec


# ------------------------------------------------------------------------------------- runs
def _plain(x):
    """x as JSON-ready plain Python (tuples as lists, numpy scalars as numbers)"""
    import numpy as np

    if isinstance(x, dict):
        return {str(k): _plain(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_plain(v) for v in x]
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, np.ndarray):
        return x.tolist()
    return x


def _metrics(mh):
    out = {k: v for k, v in mh.items() if k != "timestamps"}
    out["policy_updates"] = [{k: v for k, v in u.items() if k != "time"}
                             for u in mh["policy_updates"]]
    return _plain(out)


def _weights_sha(agent):
    import torch

    torch.cuda.synchronize()
    h = hashlib.sha256()
    for p in agent.actor_critic.parameters():
        h.update(p.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def _result(res, agent):
    assert res["status"] == "COMPLETED", res.get("error_message")
    name = res["experiment_name"]
    row = list(csv.DictReader(open(os.path.join("artifacts", "highway-ppo",
                                                f"summary_{name}.csv"))))[0]
    return {"rewards": _plain(res["rewards"]), "avg_rewards": _plain(res["avg_rewards"]),
            "metrics_history": _metrics(res["metrics_history"]), "summary": row,
            "weights_sha256": _weights_sha(agent)}


def runs():
    import copy

    import numpy as np
    import torch

    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner
    from hwy import GridSpec, LidarSpec
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent
    from training import routine

    agents = []

    class Runner(ExperimentRunner):
        def _create_agent(self, *a, **kw):
            agents.append(super()._create_agent(*a, **kw))
            return agents[-1]

    sensor = {"los": True, "range": 60.0, "dropout": 0.1, "noise": [0.5, 0.25, 0.1], "salt": 3}
    launched = {
        "plain": {},
        "stats": {"episode_stats": True, "safety_stats": True},
        "reference+stats": {"episode_schedule": "reference", "episode_stats": True,
                            "safety_stats": True},
        "bootstrap": {"truncation": "bootstrap"},
        "sensor": {"sensor": sensor},
        "shield": {"shield": {}, "eval_shields": {"none": None, "default": {}}},
        "grid": {"grid": True},
        "lidar": {"lidar": True},
        "evals": {"attribution": True, "eval_orders": ["sorted", "shuffled"],
                  "eval_sensors": {"perfect": {}, "fog": sensor}},
    }
    rec = {"launch": {}, "launch_group": {}, "direct": {}}
    for name, extra in launched.items():
        del agents[:]
        res = Runner(HIGHWAY_CONFIG).launch(mini_exp(42, name.replace("+", "_"), **extra))
        rec["launch"][name] = _result(res, agents[0])
        print("launch", name, rec["launch"][name]["rewards"], flush=True)
    for schedule in ("lockstep", "reference"):
        del agents[:]
        extra = {"episode_stats": True, "safety_stats": True,
                 **({} if schedule == "lockstep" else {"episode_schedule": schedule})}
        cell = [mini_exp(s, f"group_{schedule}", **extra) for s in (42, 1042)]
        out = Runner(HIGHWAY_CONFIG).launch_group(cell)
        rec["launch_group"][schedule] = [_result(r, a) for r, a in zip(out, agents)]
        print("launch_group", schedule, [r["rewards"] for r in rec["launch_group"][schedule]],
              flush=True)

    dev = torch.device("cuda", 0)
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=5)
    n, seed = 3, 7
    env = HighwayVecEnv(cfg, num_envs=4, device=dev, autoreset=True)

    def agent_of(sd):
        torch.manual_seed(64)
        return PPOAgent(sd, 2, lr=3e-4, epochs=2, hidden_dim=64, device=dev, num_minibatches=4,
                        seed=64)

    agent = agent_of(env.obs_rows * env.obs_features)
    grid_agent = agent_of(GridSpec().stride(int(env.hwy_config.n_features)))
    lidar_agent = agent_of(LidarSpec().stride(int(env.hwy_config.n_features)))
    d = rec["direct"]
    try:
        d["evaluate"] = routine.evaluate(env, agent, n, exp_seed=seed)
        d["evaluate order"] = routine.evaluate(env, agent, n, exp_seed=seed, order="shuffled")
        d["evaluate sensor"] = routine.evaluate(env, agent, n, exp_seed=seed, sensor=sensor)
        d["evaluate sensor+order"] = routine.evaluate(env, agent, n, exp_seed=seed, sensor=sensor,
                                                      order="shuffled")
        d["evaluate shield"] = routine.evaluate(env, agent, n, exp_seed=seed, shield={})
        d["evaluate grid"] = routine.evaluate(env, grid_agent, n, exp_seed=seed, grid=True)
        d["evaluate lidar"] = routine.evaluate(env, lidar_agent, n, exp_seed=seed, lidar=True)
        d["safety_profile"] = _plain(routine.safety_profile(env, agent, n, exp_seed=seed))
        d["shield_profile"] = _plain(routine.shield_profile(env, agent, {}, n, exp_seed=seed))
        d["attribution"] = _plain(routine.attribution(env, agent, n, exp_seed=seed))
        d["evaluate again"] = routine.evaluate(env, agent, n, exp_seed=seed)
        for name, ag, kw in (("tint=ttc", agent, {"tint": "ttc"}),
                             ("tint=hidden+sensor", agent, {"tint": "hidden", "sensor": sensor}),
                             ("attribution=value", agent, {"attribution": "value"}),
                             ("grid", grid_agent, {"grid": True}),
                             ("lidar", lidar_agent, {"lidar": True, "tint": "lidar"})):
            out_dir = os.path.join("viz", name.replace("=", "_").replace("+", "_"))
            rewards = routine.visualize_agent(env, ag, num_episodes=n, exp_seed=seed,
                                              out_dir=out_dir, **kw)
            frames = [hashlib.sha256(np.load(os.path.join(
                out_dir, f"viz_episode_{ep + 1}.npy")).tobytes()).hexdigest() for ep in range(n)]
            d[f"visualize {name}"] = {"rewards": _plain(rewards), "frames_sha256": frames}
            print("visualize", name, rewards, flush=True)
    finally:
        for cache in ("_eval_envs", "_safety_envs", "_attr_envs"):
            for ev in getattr(env, cache, {}).values():
                ev.close()
        env.close()
    return rec


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    mode = p.add_mutually_exclusive_group(required=True)
    mode.add_argument("--refusals", action="store_true")
    mode.add_argument("--runs", action="store_true")
    p.add_argument("--out", required=True)
    p.add_argument("--pkg", default=os.path.join(ROOT, "highway-rope-ppo_amd"))
    args = p.parse_args()
    out = os.path.abspath(args.out)
    sys.path.insert(0, os.path.abspath(args.pkg))
    cwd = os.getcwd()
    with tempfile.TemporaryDirectory() as tmp:  # the runs write artifacts/ under the cwd
        os.chdir(tmp)
        try:
            rec = refusals() if args.refusals else runs()
        finally:
            os.chdir(cwd)
    count = sum(len(v) for v in rec.values())
    if args.refusals:
        rec = _by_outcome(rec)
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:  # one line per run, call or distinct outcome
        dump = lambda x: json.dumps(x, separators=(",", ":"), sort_keys=True)  # noqa: E731
        f.write("{\n" + ",\n".join(
            f"{json.dumps(sec)}:" + (dump(rec[sec]) if "axes" in rec[sec] else "{\n" + ",\n".join(
                f" {json.dumps(k)}:{dump(v)}" for k, v in sorted(rec[sec].items())) + "\n}")
            for sec in sorted(rec)) + "\n}\n")
    print(f"{count} records -> {out}")


def _by_outcome(rec):
    """The refusal record without its repeats: ``outcomes`` lists each distinct outcome once, by
    number, and every section maps an option set to its outcomes' numbers, one per entry of the
    section's ``axes`` (the rest of the case: which stub, which buffer)."""
    numbers, out = {}, {"outcomes": {}}
    for sec, cases in rec.items():
        split = {k: (k.split(" ", 1) + [""])[:2] for k in cases}
        axes = sorted({where for _, where in split.values()})
        out[sec] = {"axes": axes}
        for k, (names, where) in split.items():
            n = numbers.setdefault(json.dumps(cases[k]), len(numbers))
            out["outcomes"][f"{n:03d}"] = cases[k]
            out[sec].setdefault(names, [None] * len(axes))[axes.index(where)] = n
    return out


if __name__ == "__main__":
    main()
