"""What ppo/rollout.py, training/routine.py, experiments/runner.py and visualize.py build on
hwy_grid: the grid rollout captured and by hand, evaluate(grid=...), training under
extra["grid"] on the fused learner, and every refusal."""

from __future__ import annotations

import copy
import json
import os

import numpy as np
import pytest
import torch

from config.base_config import HIGHWAY_CONFIG
from hwy import GridSpec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, T, H = 8, 4, 64
SPEC = GridSpec()            # 3 x 24 x 5 and the shipped four-feature row: 364 floats
SD = SPEC.stride(4)
NAMES = ("states", "actions", "pre_tanh", "log_probs", "values", "rewards", "terminated",
         "truncated", "dones", "ep_return", "ep_length")


def _cfg(**kw):
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(kw)
    return cfg


def _agent(seed=5, **kw):
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    return PPOAgent(SD, 2, lr=3e-4, epochs=2, hidden_dim=H, device=DEV, num_minibatches=4,
                    seed=seed, **kw)


# ------------------------------------------------------------------- the grid rollout
def test_captured_grid_rollout_equals_the_eager_one_and_the_steps_by_hand():
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    assert SD == 364 and SD % 4 == 0
    envs = [HighwayVecEnv(_cfg(max_episode_steps=5), num_envs=E, device=DEV, autoreset=True,
                          seed_base=11) for _ in range(3)]
    try:
        agent = _agent()
        bufs = [RolloutBuffer(T, E, SD, 2, DEV) for _ in range(2)]
        for env in envs:
            env.reset()
        graph, eager, twin = envs
        rolls = [LockstepRollout(agent, graph, bufs[0], use_graph=True, grid=SPEC),
                 LockstepRollout(agent, eager, bufs[1], use_graph=False, grid=SPEC.to_dict())]
        # the launch at construction wrote states[0] from the reset states
        assert torch.equal(bufs[0].states[0], twin.grid(SPEC))
        assert torch.equal(bufs[1].states[0], bufs[0].states[0]) and bool(bufs[0].states[0].any())
        resets = 0
        for it in range(4):
            rolls[0].run()
            bufs[1].noise.copy_(bufs[0].noise)
            bufs[1].draw_noise = lambda g: None   # the eager twin replays the same draws
            rolls[1].run()
            torch.cuda.synchronize()
            for name in NAMES:
                assert torch.equal(getattr(bufs[0], name), getattr(bufs[1], name)), (it, name)
            assert torch.equal(graph.export_state(), eager.export_state()), it
            # states[t + 1] is grid() of a twin stepped eagerly with the taped actions
            for t in range(T):
                _, _, te, tr, _ = twin.step(bufs[0].actions[t].contiguous())
                resets += int((te | tr).sum())
                assert torch.equal(bufs[0].states[t + 1], twin.grid(SPEC)), (it, t)
            # the Kinematics rows of the last step stayed in the env's own buffer
            assert torch.equal(graph.obs_buf, twin.obs_buf)
            for r in rolls:
                r.start_next()
        assert resets > 0, "no autoreset happened"
        assert rolls[0].stats["rollout_replay"] >= 1, rolls[0].stats
        assert rolls[1].stats["rollout_replay"] == 0
        keys = {LockstepRollout(agent, graph, bufs[0], grid=s)._launch_key()
                for s in (SPEC, GridSpec(align=True))}
        assert len(keys) == 2, "the spec is not part of the launch key"
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------- evaluation
def test_evaluate_on_the_grid(monkeypatch):
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    n, seed = 5, 7
    cfg = _cfg(max_episode_steps=8)
    env = HighwayVecEnv(cfg, num_envs=4, device=DEV, autoreset=True)
    twin = HighwayVecEnv(cfg, num_envs=n, device=DEV, autoreset=False)
    agent = _agent(seed=64)
    try:
        got = routine.evaluate(env, agent, n, exp_seed=seed, grid=SPEC)
        assert routine.evaluate(env, agent, n, exp_seed=seed, grid=SPEC) == got   # the key is stable
        assert getattr(env, "_eval_memo", None) is None, "the plain memo was touched"
        # by hand: reset, grid, select_action, step
        twin.reset(seeds=torch.arange(n, device=DEV, dtype=torch.int64) + (seed + 1000))
        total = torch.zeros(n, dtype=torch.float64, device=DEV)
        alive = torch.ones(n, dtype=torch.bool, device=DEV)
        for _ in range(twin.max_episode_steps + 1):
            a = agent.select_action(twin.grid(SPEC), deterministic=True)[0]
            _, r, te, tr, _ = twin.step(a.contiguous())
            total += torch.where(alive, r.double(), torch.zeros_like(total))
            alive &= ~(te.bool() | tr.bool())
        assert not bool(alive.any())
        assert got == float(total.mean().item())
        other = routine.evaluate(env, agent, n, exp_seed=seed, grid=GridSpec(align=True))
        assert np.isfinite(other) and len(env._eval_grid_memo) == 2
        # a memo hit runs nothing, whatever form the spec comes in
        monkeypatch.setattr(routine, "_run_eval_vector", lambda *a, **k: pytest.fail("the memo missed"))
        assert routine.evaluate(env, agent, n, exp_seed=seed, grid=True) == got
        assert routine.evaluate(env, agent, n, exp_seed=seed, grid=SPEC.to_dict()) == got
        monkeypatch.undo()
        # the one-env loop: HighwayEnv.grid per step, the same episodes one at a time
        one = HighwayEnv(cfg)
        try:
            single = routine.evaluate(one, agent, 2, exp_seed=seed, grid=SPEC)
        finally:
            one.close()
        pair = routine.evaluate(env, agent, 2, exp_seed=seed, grid=SPEC)
        print(f"grid evaluation: vector {pair!r}, one env {single!r}")
        assert abs(single - pair) <= 1e-4 * max(1.0, abs(pair))
    finally:
        for e in getattr(env, "_eval_envs", {}).values():
            e.close()
        env.close()
        twin.close()


# ------------------------------------------------------------------- the runner
def _exp(seed, name, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=H, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 16 envs x 4 steps
    return Experiment(name=f"grid_{name}_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=10, target_reward=1e9,
                      extra={"num_envs": 16, "eval_interval": 4, "log_interval": 50,
                             "num_minibatches": 4, **extra},
                      env_config_overrides={"max_episode_steps": 6})


def test_launch_trains_on_the_grid_with_the_fused_learner(tmp_path, monkeypatch):
    from experiments.runner import ExperimentRunner
    from training import routine

    monkeypatch.chdir(tmp_path)
    agents, dims, seen = [], [], []
    inner = routine.evaluate

    def spy(*a, **kw):
        seen.append(kw.get("grid"))
        return inner(*a, **kw)

    monkeypatch.setattr(routine, "evaluate", spy)

    class Runner(ExperimentRunner):
        def _create_agent(self, state_dim, *a, **kw):
            dims.append(state_dim)
            agents.append(super()._create_agent(state_dim, *a, **kw))
            return agents[-1]

    e = _exp(42, "default", grid=True)
    res = Runner(HIGHWAY_CONFIG).launch(e)
    assert res["status"] == "COMPLETED", res.get("error_traceback")
    torch.cuda.synchronize()
    agent = agents[0]
    assert dims == [SD]
    mh = res["metrics_history"]
    art = os.path.join("artifacts", "highway-ppo")
    booked = json.load(open(os.path.join(art, f"training_metrics_{e.name}.json")))
    assert mh["grid"] == booked["grid"] == SPEC.to_dict()
    assert GridSpec.from_dict(booked["grid"]) == SPEC
    assert len(mh["policy_updates"]) >= 2, "fewer than two updates ran"
    for u in mh["policy_updates"]:
        assert all(np.isfinite(v) for v in u.values() if isinstance(v, (int, float))), u
    assert all(np.isfinite(r) for r in res["rewards"]) and all(np.isfinite(mh["episode_rewards"]))
    assert seen and all(s == SPEC for s in seen), "an evaluation of the run did not use its grid"
    # the fused step and fused acting, asserted on the agent
    F = agent._fused
    assert agent.backend != "torch" and F is not None and agent._adam_owner == "fused"
    assert F._tile_off is not None, "the general path, not the four-launch fused step"
    assert int(F.counters[0]) > 0, "no fused minibatch step ran"
    assert agent._act_fused_ok(torch.empty(1, SD, device=DEV))
    assert agent.actor_critic.shared[0].weight.shape == (H, SD)


# ------------------------------------------------------------------- refusals
class _Stub:
    """an env or agent with just the attributes the argument checks read"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.unwrapped = self


def test_refusals():
    import visualize
    from experiments.runner import ExperimentRunner
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout, check_grid
    from training.routine import evaluate, train_with_experiment_name, visualize_agent

    one_env, vec = _Stub(is_vector_env=False), _Stub(is_vector_env=True)
    assert check_grid(None) is None and check_grid(True) == SPEC and check_grid({}) == SPEC
    for kw, word in ((dict(truncation="bootstrap"), 'truncation="bootstrap"'),
                     (dict(episode_schedule="reference"), 'episode_schedule="reference"'),
                     (dict(sensor={}), "grid does not go with sensor"),
                     (dict(shield={}), "grid does not go with shield")):
        with pytest.raises(ValueError, match=word):
            check_grid(SPEC, **kw)
        with pytest.raises(ValueError, match=word):
            LockstepRollout(_Stub(), _Stub(), RolloutBuffer(2, 2, SD, 2, DEV), grid=SPEC, **kw)
    with pytest.raises(ValueError, match="unknown grid keys"):
        check_grid({"cells": 3})
    with pytest.raises(ValueError, match="grid needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), grid=True)
    with pytest.raises(ValueError, match="grid does not run over a process group"):
        train_with_experiment_name(vec, _Stub(_dist=object()), grid=True)
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        train_with_experiment_name(vec, _Stub(), grid=True, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        train_with_experiment_name(vec, _Stub(), grid=True, episode_schedule="reference")
    with pytest.raises(ValueError, match="eval_orders"):
        train_with_experiment_name(vec, _Stub(), grid=True, eval_orders=["sorted"])
    for kw in (dict(order="sorted"), dict(sensor={}), dict(shield={})):
        with pytest.raises(ValueError, match=r"evaluate\(grid=...\) does not go with"):
            evaluate(vec, _Stub(), grid=True, **kw)
    with pytest.raises(ValueError, match="does not go with sensor or attribution"):
        visualize_agent(vec, _Stub(), num_episodes=1, grid=True, sensor={})
    # a buffer of the Kinematics width is refused
    from hwy.vec_env import HighwayVecEnv

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=2, device=DEV)
    try:
        with pytest.raises(ValueError, match="state width 364"):
            LockstepRollout(_Stub(), env, RolloutBuffer(2, 2, 60, 2, DEV), grid=SPEC)
    finally:
        env.close()
    for val in (True, {}, {"align": True}, SPEC):
        cell = [_exp(42, "g", grid=val), _exp(1042, "g", grid=val)]
        with pytest.raises(ValueError, match="grid"):
            ExperimentRunner.check_batch([cell], own_schedules=True)
        with pytest.raises(ValueError, match="grid"):
            ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
    for extra, word in ((dict(grid=True, truncation="bootstrap"), "bootstrap"),
                        (dict(grid=True, episode_schedule="reference"), "reference"),
                        (dict(grid=True, sensor={}), "sensor"), (dict(grid=True, shield={}), "shield"),
                        (dict(grid={"cells": 3}), "unknown grid keys"),
                        (dict(grid=True, num_envs=1), "vectorised loop")):
        res = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, "r", **extra))
        assert res["status"] == "FAILED" and word in res["error_message"], res
    for argv in (["--grid", "{bad"], ["--grid", '{"cells": 1}'], ["--grid", "true", "--sensor", "{}"],
                 ["--grid", "true", "--attribution", "value"]):
        with pytest.raises(SystemExit):
            visualize.main(["--model", "x.pth"] + argv)
    with pytest.raises(ValueError, match="grid does not go with"):
        visualize.record("x.pth", "out", grid=True, attribution="value")


# ------------------------------------------------------------------- a grid checkpoint drives
def test_visualize_a_grid_trained_checkpoint(tmp_path):
    import visualize

    agent = _agent(seed=3)
    path = str(tmp_path / "ppo_highway_best_sorted_grid_demo.pth")
    agent.save(path)
    rewards = visualize.record(path, str(tmp_path / "out"), episodes=2, seed=1, grid=True)
    assert len(rewards) == 2 and all(np.isfinite(rewards))
    frames = np.load(str(tmp_path / "out" / "ppo_highway_best_sorted_grid_demo" / "viz_episode_1.npy"))
    assert frames.ndim == 4 and frames.shape[0] >= 2
    # without the spec the input width does not fit, and a spec of another stride neither
    with pytest.raises(ValueError, match="the checkpoint takes 364 inputs"):
        visualize.record(path, str(tmp_path / "out2"))
    with pytest.raises(ValueError, match="the checkpoint takes 364 inputs"):
        visualize.record(path, str(tmp_path / "out3"), grid={"nx": 12})
