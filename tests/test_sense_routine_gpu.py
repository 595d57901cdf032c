"""What training/routine.py, ppo/rollout.py and experiments/runner.py build on hwy_sense:
evaluate(sensor=...), eval_sensors, training under extra["sensor"], the sensed captured rollout,
the hidden-vehicle tint and every refusal."""

from __future__ import annotations

import copy
import csv
import json
import os

import numpy as np
import pytest
import torch

import sense_util as su
from config.base_config import HIGHWAY_CONFIG
from hwy import SensorModel

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S = SensorModel(los=True, range=90.0, dropout=0.1, noise=(0.5, 0.2, 0.5), salt=3)


# ------------------------------------------------------------------- evaluation
def test_evaluate_under_a_sensor(monkeypatch):
    from test_eval_gpu import _agent, _config
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    n, seed = 5, 7
    env = HighwayVecEnv(_config(), num_envs=4, device=DEV, autoreset=True)
    agent = _agent(64, seed=64)
    twin = HighwayVecEnv(_config(), num_envs=n, device=DEV, autoreset=False)
    try:
        base = routine.evaluate(env, agent, n, exp_seed=seed)
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base   # the memo's key is stable
        shuffled = routine.evaluate(env, agent, n, exp_seed=seed, order="shuffled")
        memo, order_memo = env._eval_memo, dict(env._eval_order_memo)
        assert routine.evaluate(env, agent, n, exp_seed=seed, sensor=su.NULL) == base
        assert routine.evaluate(env, agent, n, exp_seed=seed, sensor={}) == base
        assert routine.evaluate(env, agent, n, exp_seed=seed, sensor=su.NULL, order="shuffled") == shuffled
        got = {o: routine.evaluate(env, agent, n, exp_seed=seed, sensor=S, order=o)
               for o in (None, "sorted", "shuffled")}
        assert env._eval_memo is memo and env._eval_order_memo == order_memo, "another memo was touched"
        assert got[None] == got["sorted"]          # this env's own order
        # by hand: the same episodes through ev.sense
        for o in (None, "shuffled"):
            twin.reset(seeds=torch.arange(n, device=DEV, dtype=torch.int64) + (seed + 1000))
            total, alive = torch.zeros(n, dtype=torch.float64, device=DEV), torch.ones(n, dtype=torch.bool, device=DEV)
            for _ in range(twin.max_episode_steps + 1):
                obs = twin.sense(S, order=o)
                a = agent.select_action(obs.reshape(n, -1), deterministic=True)[0]
                _, r, te, tr, _ = twin.step(a.contiguous())
                total += torch.where(alive, r.double(), torch.zeros_like(total))
                alive &= ~(te.bool() | tr.bool())
            assert not bool(alive.any())
            assert got[o] == float(total.mean().item()), o
        print(f"plain {base!r}, shuffled {shuffled!r}, under the sensor {got!r}")
        assert got[None] != base
        # a memo hit runs nothing; a different sensor misses
        monkeypatch.setattr(routine, "_run_eval_vector", lambda *a, **k: pytest.fail("the memo missed"))
        assert routine.evaluate(env, agent, n, exp_seed=seed, sensor=S.to_dict(), order="shuffled") == got["shuffled"]
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base
        with pytest.raises(pytest.fail.Exception, match="the memo missed"):
            routine.evaluate(env, agent, n, exp_seed=seed, sensor=SensorModel(range=50.0))
    finally:
        for e in getattr(env, "_eval_envs", {}).values():
            e.close()
        env.close()
        twin.close()


# ------------------------------------------------------------------- the sensed rollout
def test_graph_replayed_sensed_rollout_equals_the_steps_by_hand():
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    T, E, sensor = 3, 6, su.LOS
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["max_episode_steps"] = 5
    envs = [HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=True, seed_base=11) for _ in range(2)]
    try:
        agent = PPOAgent(60, 2, lr=3e-4, epochs=2, hidden_dim=64, device=DEV, num_minibatches=4, seed=5)
        bufs = [RolloutBuffer(T, E, 60, 2, DEV) for _ in range(2)]
        plain = []
        for env, buf in zip(envs, bufs):
            obs, _ = env.reset()
            plain.append(obs.clone())
            buf.states[0].copy_(obs.reshape(E, 60))
        env, hand = envs
        buf, hb = bufs
        roll = LockstepRollout(agent, env, buf, use_graph=True, sensor=sensor)
        hand.sense_into(sensor, obs=hb.states[0])
        assert torch.equal(buf.states[0], hb.states[0])
        assert not torch.equal(buf.states[0], plain[0].reshape(E, 60)), "the reset states were not sensed"
        shape = hand.obs_buf.shape[1:]
        for it in range(4):
            roll.run()
            hb.noise.copy_(buf.noise)
            for t in range(T):
                agent.select_action(hb.states[t], out=(hb.actions[t], hb.pre_tanh[t], hb.log_probs[t],
                                                       hb.values[t]), noise=hb.noise[t])
                hand.step_into(hb.actions[t], hb.states[t + 1].view(E, *shape), hb.rewards[t],
                               hb.terminated[t], hb.truncated[t], hb.ep_return[t], hb.ep_length[t])
                plain_next = hb.states[t + 1].clone()
                hand.sense_into(sensor, obs=hb.states[t + 1])
            torch.cuda.synchronize()
            for name in ("states", "actions", "log_probs", "values", "rewards", "terminated",
                         "truncated", "ep_return", "ep_length"):
                assert torch.equal(getattr(buf, name), getattr(hb, name)), (it, name)
            assert torch.equal(env.export_state(), hand.export_state()), it
            roll.start_next()
            hb.states[0].copy_(hb.states[T])
        assert not torch.equal(plain_next, hb.states[T]), "line of sight hid nothing in the last step"
        assert roll.stats["rollout_replay"] >= 1, roll.stats
        keys = {LockstepRollout(agent, env, buf, sensor=s)._launch_key() for s in (su.LOS, su.FULL, None)}
        assert len(keys) == 3, "the sensor is not part of the launch key"
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------- the runner
def _exp(seed, name, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps
    return Experiment(name=f"sense_{name}_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=12, target_reward=1e9,
                      extra={"num_envs": 4, "eval_interval": 4, "log_interval": 50, **extra},
                      env_config_overrides={"max_episode_steps": 12})


def _launch(e):
    from experiments.runner import ExperimentRunner

    agents = []

    class Runner(ExperimentRunner):
        def _create_agent(self, *a, **kw):
            agents.append(super()._create_agent(*a, **kw))
            return agents[-1]

    res = Runner(HIGHWAY_CONFIG).launch(e)
    assert res["status"] == "COMPLETED", res.get("error_message")
    torch.cuda.synchronize()
    res["weights"] = [p.detach().clone() for p in agents[0].actor_critic.parameters()]
    art = os.path.join("artifacts", "highway-ppo")
    res["json"] = json.load(open(os.path.join(art, f"training_metrics_{e.name}.json")))
    res["summary"] = list(csv.DictReader(open(os.path.join(art, f"summary_{e.name}.csv"))))[0]
    return res


def _same_training(a, b, extra_keys):
    assert a["rewards"] == b["rewards"] and a["avg_rewards"] == b["avg_rewards"]
    assert all(torch.equal(x, y) for x, y in zip(a["weights"], b["weights"]))
    assert a["summary"]["final_reward"] == b["summary"]["final_reward"]
    m1, m0 = a["metrics_history"], b["metrics_history"]
    assert set(m1) - set(extra_keys) == set(m0)
    for k in m0:
        if k in ("timestamps", "experiment_name"):
            continue
        if k == "policy_updates":
            assert [u["loss"] for u in m1[k]] == [u["loss"] for u in m0[k]]
        else:
            assert m1[k] == m0[k], k


@pytest.fixture(scope="module")
def plain_run(tmp_path_factory):
    cwd = os.getcwd()
    os.chdir(tmp_path_factory.mktemp("sense_runs"))
    try:
        yield _launch(_exp(42, "plain"))
    finally:
        os.chdir(cwd)


def test_training_under_the_null_sensor_is_the_training_without(plain_run):
    on = _launch(_exp(42, "null", sensor={}))
    _same_training(on, plain_run, {"sensor"})
    assert on["metrics_history"]["sensor"] == on["json"]["sensor"] == SensorModel().to_dict()
    assert "sensor" not in plain_run["json"]


def test_training_under_a_sensor_differs_and_books_it(plain_run, monkeypatch):
    from training import routine

    inner, seen = routine.evaluate, []

    def spy(*a, **kw):
        seen.append(kw.get("sensor"))
        return inner(*a, **kw)

    monkeypatch.setattr(routine, "evaluate", spy)
    on = _launch(_exp(42, "full", sensor=su.FULL.to_dict()))
    assert on["json"]["sensor"] == su.FULL.to_dict()
    assert on["metrics_history"]["episode_rewards"] != plain_run["metrics_history"]["episode_rewards"]
    assert seen and all(s == su.FULL for s in seen), "an evaluation of the run did not use its sensor"
    assert all(np.isfinite(on["rewards"]))


def test_eval_sensors_books_sensor_rewards_after_the_same_training(plain_run, monkeypatch):
    from training import routine

    inner, calls = routine.evaluate, []

    def spy(env, agent, num_episodes=10, render=False, exp_seed=0, order=None, sensor=None):
        value = inner(env, agent, num_episodes, render, exp_seed, order, sensor)
        if sensor is not None:
            plain = inner(env, agent, num_episodes, render, exp_seed)
            calls.append((sensor, num_episodes, exp_seed, value, plain))
        return value

    monkeypatch.setattr(routine, "evaluate", spy)
    sensors = {"perfect": {}, "los": {"los": True}, "fog": S.to_dict()}
    on = _launch(_exp(42, "evals", eval_sensors=sensors))
    _same_training(on, plain_run, {"sensor_rewards"})
    booked = on["metrics_history"]["sensor_rewards"]
    assert booked == on["json"]["sensor_rewards"] and list(booked) == list(sensors)
    assert "sensor_rewards" not in plain_run["json"]
    assert [c[:3] for c in calls] == [(SensorModel.from_dict(s), 10, 42) for s in sensors.values()]
    assert booked == {n: c[3] for n, c in zip(sensors, calls)}
    assert booked["perfect"] == calls[0][4], "the null sensor is not the plain evaluation"
    assert all(np.isfinite(v) for v in booked.values())


# ------------------------------------------------------------------- refusals
class _Stub:
    """an env or agent with just the attributes the argument checks read"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.unwrapped = self


def test_refusals():
    from experiments.runner import ExperimentRunner
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import evaluate, train_with_experiment_name, visualize_agent

    one_env, vec = _Stub(is_vector_env=False), _Stub(is_vector_env=True)
    with pytest.raises(ValueError, match="sensor needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), sensor={})
    with pytest.raises(ValueError, match="eval_sensors needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), eval_sensors={"a": {}})
    with pytest.raises(ValueError, match="sensor does not run over a process group"):
        train_with_experiment_name(vec, _Stub(_dist=object()), sensor={})
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        train_with_experiment_name(vec, _Stub(), sensor={}, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        train_with_experiment_name(vec, _Stub(), sensor={}, episode_schedule="reference")
    with pytest.raises(ValueError, match="dropout"):
        train_with_experiment_name(vec, _Stub(), sensor={"dropout": 2})
    with pytest.raises(ValueError, match="eval_sensors must be a dict"):
        train_with_experiment_name(vec, _Stub(), eval_sensors=[{}])
    with pytest.raises(ValueError, match="unknown sensor keys"):
        train_with_experiment_name(vec, _Stub(), eval_sensors={"a": {"fog": 1}})
    with pytest.raises(ValueError, match=r"evaluate\(sensor=...\) needs a HighwayVecEnv"):
        evaluate(one_env, _Stub(), sensor={})
    buf = RolloutBuffer(2, 2, 4, 2, DEV)
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        LockstepRollout(_Stub(), _Stub(), buf, sensor={}, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        LockstepRollout(_Stub(), _Stub(), buf, sensor={}, episode_schedule="reference")
    with pytest.raises(ValueError, match='tint="hidden" needs a sensor'):
        visualize_agent(vec, _Stub(), num_episodes=1, tint="hidden")
    for key, val in (("sensor", {}), ("sensor", {"los": True}), ("eval_sensors", {"a": {}})):
        cell = [_exp(42, "g", **{key: val}), _exp(1042, "g", **{key: val})]
        with pytest.raises(ValueError, match=key):
            ExperimentRunner.check_batch([cell], own_schedules=True)
        with pytest.raises(ValueError, match=key):
            ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
    for extra, word in ((dict(sensor={}, truncation="bootstrap"), "bootstrap"),
                        (dict(sensor={}, episode_schedule="reference"), "reference")):
        res = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, "r", **extra))
        assert res["status"] == "FAILED" and word in res["error_message"], res


# ------------------------------------------------------------------- frames
def test_visualize_agent_hidden_tint(tmp_path):
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent
    from training.routine import visualize_agent

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=5, vehicles_density=2, screen_width=96, screen_height=32)
    torch.manual_seed(0)
    agent, env = PPOAgent(60, 2, hidden_dim=64, device=DEV), HighwayVecEnv(cfg, num_envs=2, device=DEV)
    n, sensor = 3, SensorModel(los=True, range=60.0)
    twin = HighwayVecEnv(cfg, num_envs=n, device=DEV, autoreset=False)
    try:
        tape, out_dir = [], str(tmp_path / "hidden")
        visualize_agent(env, agent, num_episodes=n, exp_seed=42, out_dir=out_dir, tint="hidden",
                        sensor=sensor.to_dict(), tape=tape)
        frames = [np.load(os.path.join(out_dir, f"viz_episode_{ep + 1}.npy")) for ep in range(n)]
        at, tinted = [0] * n, 0.0
        for obs, state, running in tape:
            twin.import_state(state)
            assert torch.equal(obs, twin.sense(sensor)), "the policy did not act on the sensed rows"
            shade = twin.hidden_vehicles(sensor)
            tinted += float(shade.sum())
            want = twin.render(shade=shade).cpu().numpy()
            for ep in range(n):
                if running[ep]:
                    assert np.array_equal(frames[ep][at[ep]], want[ep]), (ep, at[ep])
                    at[ep] += 1
        assert at == [len(f) for f in frames] and min(at) >= 2 and tinted > 0
    finally:
        env.close()
        twin.close()


def test_visualize_cli_sensor_arguments():
    import visualize

    for argv in (["--tint", "hidden"], ["--sensor", "{bad"], ["--sensor", '{"fog": 1}'],
                 ["--sensor", '{"dropout": 2}'], ["--tint", "hidden", "--sensor", "{}", "--attribution", "value"]):
        with pytest.raises(SystemExit):
            visualize.main(["--model", "x.pth"] + argv)
    with pytest.raises(ValueError, match="needs a sensor"):
        visualize.record("x.pth", "out", tint="hidden")
