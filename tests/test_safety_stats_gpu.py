"""extra["safety_stats"] through the runner: the same training bit for bit with it on and off
(launch on either episode schedule, launch_group, launch_batch), one booked value per booked
episode, the booked values against a hand loop over HighwayVecEnv fed the run's own actions, the
refusals, the metrics file's null for +inf, safety_profile beside evaluate, and the ttc tint."""

from __future__ import annotations

import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from config.base_config import HIGHWAY_CONFIG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HORIZON = 9
E, T = 8, 16
EPISODES = 40          # four rollouts of 8 x 16 steps at a horizon of 9
KEYS = ("episode_min_ttc", "episode_min_headway", "episode_min_gap", "episode_min_distance",
        "episode_ttc_critical_share", "episode_tailgating_share")


def _exp(seed, schedule, on, name, condition="SORTED"):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=32, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = E * T
    extra = {"num_envs": E, "eval_interval": 16, "log_interval": 50}
    if schedule != "lockstep":
        extra["episode_schedule"] = schedule
    if on:
        extra["safety_stats"] = True
    return Experiment(name=f"{name}{int(on)}_{schedule}_{condition}_{seed}",
                      condition=getattr(Condition, condition), hp=hp, seed=seed,
                      max_episodes=EPISODES, target_reward=1e9, extra=extra,
                      env_config_overrides={"max_episode_steps": HORIZON, "vehicles_density": 2})


_RUNS = {}


def _run(tmp, kind, schedule, on):
    """one launch (kind "solo"), launch_group of two seeds ("group") or launch_batch of two cells
    ("batch"), once per key: the flat list of status dicts, each with its agent's final weights,
    its summary lines, its metrics file and (solo) the rollouts' actions and cut masks"""
    from experiments.runner import ExperimentRunner
    from ppo.rollout import LockstepRollout

    key = (kind, schedule, on)
    if key in _RUNS:
        return _RUNS[key]
    agents, tape = [], []

    class Runner(ExperimentRunner):
        def _create_agent(self, *a, **kw):
            agents.append(super()._create_agent(*a, **kw))
            return agents[-1]

    if kind == "solo":
        cells = [[_exp(42, schedule, on, "s")]]
    elif kind == "group":
        cells = [[_exp(s, schedule, on, "g") for s in (42, 1042)]]
    else:
        cells = [[_exp(42, schedule, on, "b", c)] for c in ("SORTED", "SHUFFLED")]
    exps = [e for c in cells for e in c]
    run = LockstepRollout.run

    def taped(self):
        run(self)
        cut = self.cut.clone() if self.episode_schedule == "reference" else None
        tape.append((self.buf.actions.clone(), cut))

    cwd = os.getcwd()
    os.chdir(tmp)
    LockstepRollout.run = taped
    try:
        r = Runner(HIGHWAY_CONFIG)
        if kind == "solo":
            res = [r.launch(exps[0])]
        elif kind == "group":
            res = r.launch_group(exps)
        else:
            res = [x for cell in r.launch_batch(cells) for x in cell]
    finally:
        LockstepRollout.run = run
        os.chdir(cwd)
    torch.cuda.synchronize()
    art = os.path.join(tmp, "artifacts", "highway-ppo")
    for x, ag, e in zip(res, agents, exps):
        assert x["status"] == "COMPLETED", x.get("error_message")
        x["weights"] = [p.detach().clone() for p in ag.actor_critic.parameters()]
        x["summary"] = open(os.path.join(art, f"summary_{e.name}.csv")).read().splitlines()
        x["file"] = json.load(open(os.path.join(art, f"training_metrics_{e.name}.json")))
        x["tape"] = tape
    _RUNS[key] = res
    return res


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("safety_runs"))


def _same_training(on, off):
    from training.routine import near_miss_rate

    mh, m0 = on["metrics_history"], off["metrics_history"]
    assert not any(k in m0 for k in KEYS) and "near_miss_rate" not in off["summary"][0]
    assert sorted(set(mh) - set(m0)) == sorted(KEYS)
    for k in m0:                                     # every pre-existing key, bit for bit
        if k == "policy_updates":
            strip = lambda us: [{a: b for a, b in u.items() if a != "time"} for u in us]
            assert strip(mh[k]) == strip(m0[k])
        elif k not in ("timestamps", "experiment_name"):
            assert mh[k] == m0[k], k
    assert on["rewards"] == off["rewards"] and on["avg_rewards"] == off["avg_rewards"]
    assert all(torch.equal(a, b) for a, b in zip(on["weights"], off["weights"]))
    n = len(mh["episode_rewards"])
    assert n == EPISODES and all(len(mh[k]) == n for k in KEYS)
    for ttc, thw, gap, dist, crit, tail in zip(*(mh[k] for k in KEYS)):
        assert all(type(v) is float for v in (ttc, thw, gap, dist, crit, tail))
        assert ttc >= 0 and thw >= 0 and dist > 0 and gap >= -5.0
        assert 0.0 <= crit <= 1.0 and 0.0 <= tail <= 1.0
        assert (crit > 0) == (ttc < 2.0) and (tail > 0) == (thw < 1.0)
    assert on["summary"][0].split(",")[:7] == off["summary"][0].split(",") + ["near_miss_rate"]
    assert float(on["summary"][1].split(",")[6]) == pytest.approx(
        near_miss_rate(mh["episode_min_ttc"]), abs=5e-5)
    # the file: the same lists, +inf as null
    for k in KEYS:
        assert len(on["file"][k]) == n
        for a, b in zip(on["file"][k], mh[k]):
            assert (a is None and math.isinf(b)) or a == b
    assert {k: v for k, v in off["file"].items() if k not in ("timestamps", "policy_updates")} == \
        {k: v for k, v in m0.items() if k not in ("timestamps", "policy_updates")}


@pytest.mark.parametrize("schedule", ["lockstep", "reference"])
def test_launch_with_safety_stats_is_the_same_training(run_dir, schedule):
    _same_training(_run(run_dir, "solo", schedule, True)[0], _run(run_dir, "solo", schedule, False)[0])


@pytest.mark.parametrize("kind, schedule", [("group", "lockstep"), ("group", "reference"),
                                            ("batch", "lockstep")])
def test_grouped_launches_with_safety_stats_are_the_same_training(run_dir, kind, schedule):
    on, off = _run(run_dir, kind, schedule, True), _run(run_dir, kind, schedule, False)
    assert len(on) == len(off) == 2
    for a, b in zip(on, off):
        _same_training(a, b)
    if kind == "group":     # seed 42 of the group books what its solo launch books
        solo = _run(run_dir, "solo", schedule, True)[0]["metrics_history"]
        for k in KEYS + ("episode_rewards",):
            assert on[0]["metrics_history"][k] == solo[k], k


@pytest.mark.parametrize("schedule", ["lockstep", "reference"])
def test_booked_values_are_a_hand_loops(run_dir, schedule):
    """the run's own actions, stepped by hand with one traffic call per state the policy acts on"""
    from experiments.config import Condition
    from experiments.wrappers import make_env
    from hwy.vec_env import alloc_traffic
    from training.routine import safety_row

    res = _run(run_dir, "solo", schedule, True)[0]
    mh, tape = res["metrics_history"], res["tape"]
    env = make_env(Condition.SORTED, HIGHWAY_CONFIG, d_embed=None,
                   env_overrides={"max_episode_steps": HORIZON, "vehicles_density": 2,
                                  "num_envs": E, "device": DEV}).unwrapped
    try:
        env.set_seed_schedule(42)
        env.reset()
        t = alloc_traffic(E, DEV)
        kw = dict(acc=t["acc"], ep_stats=t["ep_stats"])
        env.traffic_into(acc=t["acc"])
        cut = torch.zeros(E, dtype=torch.uint8, device=DEV)
        booked = []
        for actions, taped_cut in tape:
            assert actions.shape == (T, E, 2)
            for k in range(T):
                _, _, te, tr, _ = env.step(actions[k].contiguous())
                done = (te | tr).bool().cpu().numpy()
                if taped_cut is not None and k == T - 1:
                    env.cut_episodes(env.obs_buf, cut=cut)
                    assert torch.equal(cut, taped_cut), "the hand loop left the run's states"
                    env.traffic_into(restart=(te, tr, cut), **kw)
                    rows = t["ep_stats"].cpu().numpy()
                    booked += [rows[e] for e in np.nonzero(done)[0]]
                    booked += [rows[e] for e in np.nonzero(cut.cpu().numpy())[0]]
                else:
                    env.traffic_into(restart=(te, tr), **kw)
                    rows = t["ep_stats"].cpu().numpy()
                    booked += [rows[e] for e in np.nonzero(done)[0]]
        assert len(booked) >= EPISODES
        want = [safety_row(r) for r in booked[:EPISODES]]
        for i, k in enumerate(KEYS):
            assert mh[k] == [w[i] for w in want], k
        lengths = [int(r[0]) for r in booked[:EPISODES]]
        assert max(lengths) == HORIZON and min(lengths) >= 1
        if schedule == "reference":
            assert sum(int(c.sum()) for _, c in tape) >= 1
    finally:
        env.close()


class _Stub:
    """an env or agent with just the attributes the argument checks read"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.unwrapped = self


def test_refusals():
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import safety_profile, train_batch, train_with_experiment_name

    one_env, vec = _Stub(is_vector_env=False), _Stub(is_vector_env=True)
    with pytest.raises(ValueError, match="safety_stats needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), safety_stats=True)
    with pytest.raises(ValueError, match="safety_stats does not run over a process group"):
        train_with_experiment_name(vec, _Stub(_dist=object()), safety_stats=True)
    with pytest.raises(ValueError, match="safety_profile needs a HighwayVecEnv"):
        safety_profile(one_env, _Stub())
    with pytest.raises(ValueError, match="built with safety_stats=True"):
        train_batch(None, [_Stub(safety_stats=False, episode_stats=False)], ["a"], [1],
                    safety_stats=True)
    with pytest.raises(ValueError, match="RolloutBuffer built with safety_stats=True"):
        LockstepRollout(_Stub(), _Stub(), RolloutBuffer(2, 2, 4, 2, DEV), safety_stats=True)
    buf = RolloutBuffer(2, 3, 4, 2, DEV)
    assert buf.traffic_stats is None and buf.traffic_acc is None
    buf = RolloutBuffer(2, 3, 4, 2, DEV, safety_stats=True)
    assert buf.traffic_stats.shape == (2, 3, 8) and buf.traffic_acc.shape == (3, 8)
    assert not buf.traffic_acc.any()


def test_runner_refuses_mixed_cells():
    from experiments.runner import ExperimentRunner

    cells = [[_exp(42, "lockstep", True, "m")], [_exp(42, "lockstep", False, "m", "SHUFFLED")]]
    with pytest.raises(ValueError, match="share extra\\['safety_stats'\\]"):
        ExperimentRunner.check_batch(cells, own_schedules=True)


def _agent_and_env(num_envs=4):
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=HORIZON, vehicles_density=2, screen_width=96, screen_height=32)
    torch.manual_seed(0)
    return PPOAgent(60, 2, hidden_dim=64, device=DEV), HighwayVecEnv(cfg, num_envs=num_envs, device=DEV)


def test_safety_profile_beside_evaluate():
    from hwy.vec_env import HighwayVecEnv, alloc_traffic
    from training import routine

    agent, env = _agent_and_env()
    n, seed = 5, 3
    twin = HighwayVecEnv(env.config, num_envs=n, device=DEV, autoreset=False)
    try:
        base = routine.evaluate(env, agent, n, exp_seed=seed)
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base   # the memo's key is stable
        memo = env._eval_memo
        p = routine.safety_profile(env, agent, n, exp_seed=seed)
        assert env._eval_memo is memo and routine.evaluate(env, agent, n, exp_seed=seed) == base
        assert p["mean_reward"] == base
        assert p == routine.safety_profile(env, agent, n, exp_seed=seed)
        per = p["episodes"]
        assert sorted(per) == sorted([k[len("episode_"):] for k in KEYS] + ["states", "reward"])
        assert all(len(v) == n for v in per.values())
        assert all(1 <= s <= HORIZON for s in per["states"])
        assert p["mean_min_distance"] == float(np.mean(per["min_distance"]))
        assert p["near_miss_rate"] == float(np.mean([v < 2.0 for v in per["min_ttc"]]))
        # by hand: the same episodes, one call per state acted on, each episode's row as it ended
        obs, _ = twin.reset(seeds=torch.arange(n, device=DEV, dtype=torch.int64) + (seed + 1000))
        t = alloc_traffic(n, DEV)
        rows, alive = np.zeros((n, 8), np.float32), np.ones(n, bool)
        for _ in range(HORIZON):
            twin.traffic_into(acc=t["acc"])
            rows[alive] = t["acc"].cpu().numpy()[alive]
            a = agent.select_action(obs.reshape(n, -1), deterministic=True)[0]
            obs, _, te, tr, _ = twin.step(a.contiguous())
            alive &= ~(te | tr).bool().cpu().numpy()
        assert not alive.any()
        want = [routine.safety_row(r) for r in rows]
        for i, k in enumerate(KEYS):
            assert per[k[len("episode_"):]] == [w[i] for w in want], k
        assert per["states"] == [int(r[0]) for r in rows]
    finally:
        for cache in ("_eval_envs", "_safety_envs"):
            for e in getattr(env, cache, {}).values():
                e.close()
        env.close()
        twin.close()


def test_visualize_agent_ttc_tint(tmp_path):
    from hwy.vec_env import HighwayVecEnv
    from training.routine import visualize_agent

    agent, env = _agent_and_env(2)
    n = 3
    twin = HighwayVecEnv(env.config, num_envs=n, device=DEV, autoreset=False)
    try:
        with pytest.raises(ValueError, match="tint must be None or one of"):
            visualize_agent(env, agent, num_episodes=1, tint="thw")
        with pytest.raises(ValueError, match="give one of them"):
            visualize_agent(env, agent, num_episodes=1, tint="ttc", attribution="value")
        recs = {}
        for name in (None, "ttc"):
            tape, out_dir = [], str(tmp_path / str(name))
            rewards = visualize_agent(env, agent, num_episodes=n, exp_seed=42, out_dir=out_dir,
                                      tint=name, tape=tape)
            frames = [np.load(os.path.join(out_dir, f"viz_episode_{ep + 1}.npy")) for ep in range(n)]
            at, tinted = [0] * n, 0.0
            for obs, state, running in tape:
                twin.import_state(state)
                shade = None if name is None else twin.traffic()["risk"]
                if shade is not None:
                    tinted += float(shade.sum())
                want = twin.render(shade=shade).cpu().numpy()
                for ep in range(n):
                    if running[ep]:
                        assert np.array_equal(frames[ep][at[ep]], want[ep]), (name, ep, at[ep])
                        at[ep] += 1
            assert at == [len(f) for f in frames] and min(at) >= 2
            recs[name] = (rewards, frames, tinted)
        assert recs[None][0] == recs["ttc"][0]
        assert recs["ttc"][2] > 0, "no vehicle of any frame had a time-to-collision under 4 s"
    finally:
        env.close()
        twin.close()


def test_visualize_cli_refuses_both_shades():
    import visualize

    with pytest.raises(SystemExit):
        visualize.main(["--model", "x.pth", "--tint", "ttc", "--attribution", "value"])
    with pytest.raises(ValueError, match="give one of them"):
        visualize.record("x.pth", "out", tint="ttc", attribution="value")
