"""What ppo/rollout.py, training/routine.py, experiments/runner.py and visualize.py build on
hwy_lidar: the lidar rollout captured and by hand, evaluate(lidar=...), training under
extra["lidar"] on the fused learner, every refusal, and that a run without the option does not
see it."""

from __future__ import annotations

import copy
import json
import os

import numpy as np
import pytest
import torch

from config.base_config import HIGHWAY_CONFIG
from hwy import LidarSpec

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, T, H = 8, 4, 64
SPEC = LidarSpec()           # 16 cells and the shipped four-feature row: 36 floats
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


# ------------------------------------------------------------------- the lidar rollout
def test_captured_lidar_rollout_equals_the_eager_one_and_the_steps_by_hand():
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    assert SD == 36 and SD < 60
    # errors on: the captured launches read the step word and the seed as the eager ones do
    spec = LidarSpec(p_drop=0.2, sigma_r=0.5, salt=9)
    envs = [HighwayVecEnv(_cfg(max_episode_steps=5), num_envs=E, device=DEV, autoreset=True,
                          seed_base=11) for _ in range(3)]
    try:
        agent = _agent()
        bufs = [RolloutBuffer(T, E, SD, 2, DEV) for _ in range(2)]
        for env in envs:
            env.reset()
        graph, eager, twin = envs
        rolls = [LockstepRollout(agent, graph, bufs[0], use_graph=True, lidar=spec),
                 LockstepRollout(agent, eager, bufs[1], use_graph=False, lidar=spec.to_dict())]
        # the launch at construction wrote states[0] from the reset states
        assert torch.equal(bufs[0].states[0], twin.lidar(spec))
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
            # states[t + 1] is lidar() of a twin stepped eagerly with the taped actions
            for t in range(T):
                _, _, te, tr, _ = twin.step(bufs[0].actions[t].contiguous())
                resets += int((te | tr).sum())
                assert torch.equal(bufs[0].states[t + 1], twin.lidar(spec)), (it, t)
            # the Kinematics rows of the last step stayed in the env's own buffer
            assert torch.equal(graph.obs_buf, twin.obs_buf)
            for r in rolls:
                r.start_next()
        assert resets > 0, "no autoreset happened"
        assert rolls[0].stats["rollout_replay"] >= 1, rolls[0].stats
        assert rolls[1].stats["rollout_replay"] == 0
        keys = {LockstepRollout(agent, graph, bufs[0], lidar=s)._launch_key()
                for s in (spec, LidarSpec(align=True))}
        assert len(keys) == 2, "the spec is not part of the launch key"
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------- evaluation
def test_evaluate_on_the_lidar(monkeypatch):
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    n, seed = 5, 7
    cfg = _cfg(max_episode_steps=8)
    env = HighwayVecEnv(cfg, num_envs=4, device=DEV, autoreset=True)
    twin = HighwayVecEnv(cfg, num_envs=n, device=DEV, autoreset=False)
    agent = _agent(seed=64)
    try:
        got = routine.evaluate(env, agent, n, exp_seed=seed, lidar=SPEC)
        assert routine.evaluate(env, agent, n, exp_seed=seed, lidar=SPEC) == got
        assert getattr(env, "_eval_memo", None) is None, "the plain memo was touched"
        assert getattr(env, "_eval_grid_memo", None) is None, "the grid's memo was touched"
        # by hand: reset, lidar, select_action, step
        twin.reset(seeds=torch.arange(n, device=DEV, dtype=torch.int64) + (seed + 1000))
        total = torch.zeros(n, dtype=torch.float64, device=DEV)
        alive = torch.ones(n, dtype=torch.bool, device=DEV)
        for _ in range(twin.max_episode_steps + 1):
            a = agent.select_action(twin.lidar(SPEC), deterministic=True)[0]
            _, r, te, tr, _ = twin.step(a.contiguous())
            total += torch.where(alive, r.double(), torch.zeros_like(total))
            alive &= ~(te.bool() | tr.bool())
        assert not bool(alive.any())
        assert got == float(total.mean().item())
        other = routine.evaluate(env, agent, n, exp_seed=seed, lidar=LidarSpec(align=True))
        assert np.isfinite(other) and len(env._eval_lidar_memo) == 2
        # a memo hit runs nothing, whatever form the spec comes in
        monkeypatch.setattr(routine, "_run_eval_vector", lambda *a, **k: pytest.fail("the memo missed"))
        assert routine.evaluate(env, agent, n, exp_seed=seed, lidar=True) == got
        assert routine.evaluate(env, agent, n, exp_seed=seed, lidar=SPEC.to_dict()) == got
        monkeypatch.undo()
        # the one-env loop: HighwayEnv.lidar per step, the same episodes one at a time
        one = HighwayEnv(cfg)
        try:
            single = routine.evaluate(one, agent, 2, exp_seed=seed, lidar=SPEC)
        finally:
            one.close()
        pair = routine.evaluate(env, agent, 2, exp_seed=seed, lidar=SPEC)
        print(f"lidar evaluation: vector {pair!r}, one env {single!r}")
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
    hp.steps_per_update = 128  # 16 envs x 8 steps
    return Experiment(name=f"lidar_{name}_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=20, target_reward=1e9,
                      extra={"num_envs": 16, "eval_interval": 8, "log_interval": 50,
                             "num_minibatches": 4, **extra},
                      env_config_overrides={"max_episode_steps": 6})


def test_launch_trains_on_the_lidar_with_the_fused_learner(tmp_path, monkeypatch):
    from experiments.runner import ExperimentRunner
    from training import routine

    monkeypatch.chdir(tmp_path)
    agents, dims, seen = [], [], []
    inner = routine.evaluate

    def spy(*a, **kw):
        seen.append(kw.get("lidar"))
        return inner(*a, **kw)

    monkeypatch.setattr(routine, "evaluate", spy)

    class Runner(ExperimentRunner):
        def _create_agent(self, state_dim, *a, **kw):
            dims.append(state_dim)
            agents.append(super()._create_agent(state_dim, *a, **kw))
            return agents[-1]

    e = _exp(42, "default", lidar=True)
    res = Runner(HIGHWAY_CONFIG).launch(e)
    assert res["status"] == "COMPLETED", res.get("error_traceback")
    torch.cuda.synchronize()
    agent = agents[0]
    assert dims == [SD]
    mh = res["metrics_history"]
    art = os.path.join("artifacts", "highway-ppo")
    booked = json.load(open(os.path.join(art, f"training_metrics_{e.name}.json")))
    assert mh["lidar"] == booked["lidar"] == SPEC.to_dict() and "grid" not in mh
    assert LidarSpec.from_dict(booked["lidar"]) == SPEC
    assert len(mh["policy_updates"]) >= 2, "fewer than two updates ran"
    for u in mh["policy_updates"]:
        assert all(np.isfinite(v) for v in u.values() if isinstance(v, (int, float))), u
    assert all(np.isfinite(r) for r in res["rewards"]) and all(np.isfinite(mh["episode_rewards"]))
    assert seen and all(s == SPEC for s in seen), "an evaluation of the run did not use its lidar"
    # the fused step and fused acting, asserted on the agent
    F = agent._fused
    assert agent.backend != "torch" and F is not None and agent._adam_owner == "fused"
    assert int(F.counters[0]) > 0, "no fused minibatch step ran"
    assert agent._act_fused_ok(torch.empty(1, SD, device=DEV))
    assert agent.actor_critic.shared[0].weight.shape == (H, SD)


def test_a_run_without_the_option_does_not_see_it(tmp_path, monkeypatch):
    """launch() without extra["lidar"], and with it None or False, passes no lidar keyword on to
    the routine, its evaluations or the rollout -- the code a run took before the option existed
    -- and the three runs are the same bit for bit"""
    from experiments import runner
    from experiments.runner import ExperimentRunner
    from ppo import rollout
    from training import routine

    monkeypatch.chdir(tmp_path)
    calls = []
    for mod, name in ((routine, "evaluate"), (runner, "train_with_experiment_name"),
                      (routine, "_train_vector")):
        inner = getattr(mod, name)

        def spy(*a, _inner=inner, _name=name, **kw):
            calls.append((_name, sorted(kw)))
            return _inner(*a, **kw)

        monkeypatch.setattr(mod, name, spy)
    init = rollout.LockstepRollout.__init__

    def init_spy(self, *a, **kw):
        calls.append(("LockstepRollout", sorted(kw)))
        init(self, *a, **kw)
        assert self.lidar is None

    monkeypatch.setattr(rollout.LockstepRollout, "__init__", init_spy)
    runs = []
    for i, extra in enumerate(({}, {"lidar": None}, {"lidar": False})):
        e = _exp(42, f"plain{i}", **extra)
        res = ExperimentRunner(HIGHWAY_CONFIG).launch(e)
        assert res["status"] == "COMPLETED", res.get("error_traceback")
        mh = res["metrics_history"]
        assert "lidar" not in mh
        runs.append((res["rewards"], mh["episode_rewards"],
                     [sorted(u.items()) for u in mh["policy_updates"]]))
    assert {n for n, _ in calls} >= {"evaluate", "train_with_experiment_name", "_train_vector",
                                     "LockstepRollout"}
    assert not any("lidar" in kw for _, kw in calls), calls

    def same(a, b):
        return json.dumps(a, sort_keys=True, default=str) == json.dumps(b, sort_keys=True,
                                                                        default=str)

    strip = [[[kv for kv in u if "time" not in kv[0] and "sec" not in kv[0]] for u in r[2]]
             for r in runs]
    assert runs[0][:2] == runs[1][:2] == runs[2][:2]
    assert same(strip[0], strip[1]) and same(strip[0], strip[2])


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
    from ppo.rollout import LockstepRollout, check_lidar
    from training.routine import evaluate, train_with_experiment_name, visualize_agent

    one_env, vec = _Stub(is_vector_env=False), _Stub(is_vector_env=True)
    assert check_lidar(None) is None and check_lidar(True) == SPEC and check_lidar({}) == SPEC
    for kw, word in ((dict(truncation="bootstrap"), 'truncation="bootstrap"'),
                     (dict(episode_schedule="reference"), 'episode_schedule="reference"'),
                     (dict(sensor={}), "lidar does not go with sensor"),
                     (dict(shield={}), "lidar does not go with shield"),
                     (dict(grid=True), "lidar does not go with grid")):
        with pytest.raises(ValueError, match=word):
            check_lidar(SPEC, **kw)
        with pytest.raises(ValueError, match=word):
            LockstepRollout(_Stub(), _Stub(), RolloutBuffer(2, 2, SD, 2, DEV), lidar=SPEC, **kw)
    with pytest.raises(ValueError, match="unknown lidar keys"):
        check_lidar({"nx": 3})
    with pytest.raises(ValueError, match="lidar needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), lidar=True)
    with pytest.raises(ValueError, match="lidar does not run over a process group"):
        train_with_experiment_name(vec, _Stub(_dist=object()), lidar=True)
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        train_with_experiment_name(vec, _Stub(), lidar=True, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        train_with_experiment_name(vec, _Stub(), lidar=True, episode_schedule="reference")
    with pytest.raises(ValueError, match="lidar does not go with grid"):
        train_with_experiment_name(vec, _Stub(), lidar=True, grid=True)
    with pytest.raises(ValueError, match="eval_orders"):
        train_with_experiment_name(vec, _Stub(), lidar=True, eval_orders=["sorted"])
    for kw in (dict(order="sorted"), dict(sensor={}), dict(shield={}), dict(grid=True)):
        with pytest.raises(ValueError, match=r"evaluate\(lidar=...\) does not go with"):
            evaluate(vec, _Stub(), lidar=True, **kw)
    with pytest.raises(ValueError, match="does not go with sensor, grid or attribution"):
        visualize_agent(vec, _Stub(), num_episodes=1, lidar=True, sensor={})
    with pytest.raises(ValueError, match='tint="lidar" needs a lidar'):
        visualize_agent(vec, _Stub(), num_episodes=1, tint="lidar")
    # a buffer of the Kinematics width is refused
    from hwy.vec_env import HighwayVecEnv

    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=2, device=DEV)
    try:
        with pytest.raises(ValueError, match="state width 36"):
            LockstepRollout(_Stub(), env, RolloutBuffer(2, 2, 60, 2, DEV), lidar=SPEC)
    finally:
        env.close()
    for val in (True, {}, {"align": True}, SPEC):
        cell = [_exp(42, "g", lidar=val), _exp(1042, "g", lidar=val)]
        with pytest.raises(ValueError, match="lidar"):
            ExperimentRunner.check_batch([cell], own_schedules=True)
        with pytest.raises(ValueError, match="lidar"):
            ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
    for extra, word in ((dict(lidar=True, truncation="bootstrap"), "bootstrap"),
                        (dict(lidar=True, episode_schedule="reference"), "reference"),
                        (dict(lidar=True, sensor={}), "sensor"), (dict(lidar=True, shield={}), "shield"),
                        (dict(lidar=True, grid=True), "lidar does not go with grid"),
                        (dict(lidar={"nx": 3}), "unknown lidar keys"),
                        (dict(lidar=True, num_envs=1), "vectorised loop")):
        res = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, "r", **extra))
        assert res["status"] == "FAILED" and word in res["error_message"], res
    for argv in (["--lidar", "{bad"], ["--lidar", '{"nx": 1}'], ["--lidar", "true", "--sensor", "{}"],
                 ["--lidar", "true", "--grid", "true"], ["--lidar", "true", "--attribution", "value"],
                 ["--tint", "lidar"]):
        with pytest.raises(SystemExit):
            visualize.main(["--model", "x.pth"] + argv)
    with pytest.raises(ValueError, match="lidar does not go with"):
        visualize.record("x.pth", "out", lidar=True, attribution="value")
    with pytest.raises(ValueError, match='tint "lidar" needs a lidar'):
        visualize.record("x.pth", "out", tint="lidar")


# ------------------------------------------------------------------- a lidar checkpoint drives
def test_visualize_a_lidar_trained_checkpoint_and_tint_what_it_sees(tmp_path):
    import visualize

    agent = _agent(seed=3)
    path = str(tmp_path / "ppo_highway_best_sorted_lidar_demo.pth")
    agent.save(path)
    rewards = visualize.record(path, str(tmp_path / "out"), episodes=2, seed=1, lidar=True)
    assert len(rewards) == 2 and all(np.isfinite(rewards))
    plain = np.load(str(tmp_path / "out" / "ppo_highway_best_sorted_lidar_demo" / "viz_episode_1.npy"))
    assert plain.ndim == 4 and plain.shape[0] >= 2
    # the same episodes tinted by what a long-range lidar returns: the same drive, other pixels
    wide = {"cells": 16, "range_m": 60.0}
    again = visualize.record(path, str(tmp_path / "tint"), episodes=2, seed=1, lidar=wide,
                             tint="lidar")
    assert again == rewards
    tinted = np.load(str(tmp_path / "tint" / "ppo_highway_best_sorted_lidar_demo" / "viz_episode_1.npy"))
    assert tinted.shape == plain.shape
    # without the spec the input width does not fit, and a spec of another stride neither
    with pytest.raises(ValueError, match="the checkpoint takes 36 inputs"):
        visualize.record(path, str(tmp_path / "out2"))
    with pytest.raises(ValueError, match="the checkpoint takes 36 inputs"):
        visualize.record(path, str(tmp_path / "out3"), lidar={"cells": 12})
