"""truncation="bootstrap" end to end on the GPU (ppo/rollout.py, PPOAgent.update_rollout,
training/routine.py, experiments/runner.py): the rollout is the default rollout plus two buffers;
boot_values holds V(final observation) -- the final observation checked against the CPU oracle --
at the truncated, not terminated rows and 0 elsewhere; the update's GAE is the restated formula;
without a truncation the training is the default training bit for bit, with truncations it is not.

Shapes: 16 envs x 8 steps, 3-step episodes (so every env truncates at least twice per rollout),
S 60, H 64, and H 256 once for the compact acting kernel."""

import json
import os

import numpy as np
import pytest
import torch

from hwy import _abi
from oracle.oracle import OracleEnv
from test_gae_boot_gpu import _restated

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, T, S, HORIZON = 16, 8, 60, 3
ROLLOUT_KEYS = ("states", "actions", "pre_tanh", "log_probs", "values", "rewards", "terminated",
                "truncated", "dones", "ep_return", "ep_length")


def _setup(truncation, use_graph, H=64, horizon=HORIZON, episode_stats=False):
    from config.base_config import HIGHWAY_CONFIG
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout

    torch.manual_seed(3)
    env = HighwayVecEnv(dict(HIGHWAY_CONFIG, max_episode_steps=horizon), num_envs=E, device=DEV,
                        autoreset=True, seed_base=11)
    agent = PPOAgent(S, 2, lr=3e-4, epochs=2, hidden_dim=H, device=DEV, num_minibatches=4, seed=5)
    boot = truncation == "bootstrap"
    buf = RolloutBuffer(T, E, S, 2, DEV, episode_stats=episode_stats,
                        **({"truncation_bootstrap": True} if boot else {}))
    obs, _ = env.reset()
    buf.states[0].copy_(obs.reshape(E, S))
    roll = LockstepRollout(agent, env, buf, use_graph=use_graph, episode_stats=episode_stats,
                           **({"truncation": truncation} if boot else {}))
    return env, agent, buf, roll


def _snap(buf, keys=ROLLOUT_KEYS):
    return {k: getattr(buf, k).clone() for k in keys}


def _run(truncation, use_graph, iters, H=64, horizon=HORIZON, episode_stats=False):
    """`iters` rollouts, each followed by its update; the buffers after every rollout and the
    weights at the end."""
    env, agent, buf, roll = _setup(truncation, use_graph, H, horizon, episode_stats)
    keys = ROLLOUT_KEYS + (("boot_values",) if truncation == "bootstrap" else ())
    keys += ("ep_stats",) if episode_stats else ()
    snaps = []
    try:
        for _ in range(iters):
            roll.run()
            snaps.append(_snap(buf, keys))
            agent.update_rollout(buf, agent.value(buf.states[T]))
            roll.start_next()
        torch.cuda.synchronize()
        weights = [p.detach().clone() for p in agent.actor_critic.parameters()]
    finally:
        env.close()
    return snaps, weights, roll


def _same(a, b, keys, what):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("H", [64, 256])
def test_bootstrap_rollout_is_the_terminal_rollout_and_graph_equals_eager(H):
    term, _, _ = _run("terminal", False, 1, H)
    # four rollouts: the acting weights' key changes with the first update, so the graph side runs
    # two eagerly, captures (and replays) the third and replays the fourth
    eager, _, r0 = _run("bootstrap", False, 4, H)
    graph, _, r1 = _run("bootstrap", True, 4, H)
    _same(eager[0], term[0], ROLLOUT_KEYS, "bootstrap vs terminal")
    assert r1._graph is not None
    assert r1.stats["rollout_capture"] >= 1 and r1.stats["rollout_replay"] >= 1
    for i, (a, b) in enumerate(zip(eager, graph)):
        _same(a, b, ROLLOUT_KEYS + ("boot_values",), f"eager vs graph, rollout {i}")
    tr, te = eager[0]["truncated"].bool(), eager[0]["terminated"].bool()
    assert int((tr & ~te).sum()) >= E  # every env truncates within 3 steps unless it crashed
    assert bool((eager[0]["boot_values"][~(tr & ~te)] == 0).all())
    assert bool((eager[0]["boot_values"][tr & ~te] != 0).any())


def test_bootstrap_with_episode_stats_goes_through_the_same_launch():
    plain, _, _ = _run("bootstrap", True, 2)
    stats, _, _ = _run("bootstrap", True, 2, episode_stats=True)
    ref, _, _ = _run("terminal", True, 2, episode_stats=True)
    for i in range(2):
        _same(stats[i], plain[i], ROLLOUT_KEYS + ("boot_values",), f"rollout {i}")
        assert torch.equal(stats[i]["ep_stats"], ref[i]["ep_stats"]) or i > 0
    assert bool((stats[0]["ep_stats"] != 0).any())


@pytest.mark.parametrize("H", [64, 256])
def test_boot_values_are_the_values_of_the_oracles_final_observations(H):
    env, agent, buf, roll = _setup("bootstrap", False, H)
    cfg = _abi.HwyConfig.from_buffer_copy(env.hwy_config)
    cfg.autoreset = 0
    ora = OracleEnv(cfg)
    boots = 0
    try:
        buf.draw_noise(agent.generator)
        for t in range(T):
            before = env.export_state()
            roll._steps(t, t + 1)  # the rollout's own launches for step t
            torch.cuda.synchronize()
            ora.state[...] = before.cpu().numpy().view(np.uint32)
            o_obs, _, o_term, o_trunc, _, _ = ora.step(buf.actions[t].cpu().numpy())
            term, trunc = buf.terminated[t].bool().cpu().numpy(), buf.truncated[t].bool().cpu().numpy()
            np.testing.assert_array_equal(term, o_term)
            np.testing.assert_array_equal(trunc, o_trunc)
            done, boot = term | trunc, trunc & ~term
            got = buf.final_obs.cpu().numpy().view(np.uint32)
            want = o_obs.reshape(E, S).view(np.uint32)
            np.testing.assert_array_equal(got[done], want[done], err_msg=f"final obs, step {t}")
            # V of the oracle's final observations, each row at its own place in the batch
            rows = torch.zeros(E, S, device=DEV)
            rows[torch.as_tensor(done, device=DEV)] = torch.as_tensor(o_obs.reshape(E, S)[done],
                                                                      device=DEV)
            v = agent.value(rows)
            bt = torch.as_tensor(boot, device=DEV)
            assert torch.equal(buf.boot_values[t][bt].view(torch.int32), v[bt].view(torch.int32))
            assert bool((buf.boot_values[t][~bt].view(torch.int32) == 0).all())
            boots += int(boot.sum())
        assert boots >= E
    finally:
        env.close()


def test_update_rollout_runs_the_restated_gae(monkeypatch):
    from hwy import ops

    env, agent, buf, roll = _setup("bootstrap", False)
    seen = {}
    real = ops.gae_boot

    def spy(*a, **kw):
        seen["out"] = real(*a, **kw)
        return seen["out"]

    monkeypatch.setattr(ops, "gae_boot", spy)
    monkeypatch.setattr(ops, "gae", lambda *a, **kw: pytest.fail("hwy_gae ran"))
    try:
        roll.run()
        last = agent.value(buf.states[T]).clone()
        np_in = [x.cpu().numpy() for x in (buf.rewards, buf.terminated, buf.truncated, buf.values,
                                           last, buf.boot_values)]
        agent.update_rollout(buf, last)
        torch.cuda.synchronize()
        adv, ret = seen["out"]
        want_adv, want_ret = _restated(*np_in, agent.gamma, agent.lam)
        np.testing.assert_array_equal(adv.cpu().numpy().view(np.uint32), want_adv.view(np.uint32))
        np.testing.assert_array_equal(ret.cpu().numpy().view(np.uint32), want_ret.view(np.uint32))
        boot = (np_in[2] != 0) & (np_in[1] == 0)
        assert boot.sum() >= E
        # a bootstrapped row: its one-step TD error against V(final observation), chain cut
        f64 = np.float64
        td = ((np_in[0].astype(f64) + f64(agent.gamma) * np_in[5].astype(f64))
              - np_in[3].astype(f64)).astype(np.float32)
        np.testing.assert_array_equal(want_adv[boot], td[boot])
    finally:
        env.close()


def test_without_truncation_training_is_unchanged_and_with_it_it_differs():
    _, w_term, _ = _run("terminal", True, 2, horizon=1000)
    snaps, w_boot, _ = _run("bootstrap", True, 2, horizon=1000)
    assert not bool(snaps[0]["truncated"].any()) and not bool(snaps[1]["truncated"].any())
    assert bool((snaps[0]["boot_values"] == 0).all())
    assert all(torch.equal(a, b) for a, b in zip(w_term, w_boot))
    _, w_term3, _ = _run("terminal", True, 2)
    snaps3, w_boot3, _ = _run("bootstrap", True, 2)
    assert bool(snaps3[0]["truncated"].any())
    assert not all(torch.equal(a, b) for a, b in zip(w_term3, w_boot3))


def _exp(seed, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps: ~21 three-step episodes per update
    return Experiment(name=f"trunc_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=30, target_reward=1e9,
                      extra=dict({"num_envs": 4, "eval_interval": 15, "log_interval": 50},
                                 **extra),
                      env_config_overrides={"max_episode_steps": HORIZON})


def test_runner_launch_trains_with_the_option_and_records_it(tmp_path):
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    cwd = os.getcwd()
    os.chdir(tmp_path)
    try:
        on = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, truncation="bootstrap"))
        bad = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(43, truncation="sometimes"))
    finally:
        os.chdir(cwd)
    assert on["status"] == "COMPLETED", on.get("error_message")
    mh = on["metrics_history"]
    assert mh["truncation"] == "bootstrap"
    assert len(mh["policy_updates"]) == 2 and len(mh["episode_rewards"]) == 30
    assert all(np.isfinite(u["loss"]) for u in mh["policy_updates"])
    saved = json.load(open(tmp_path / "artifacts" / "highway-ppo" /
                           "training_metrics_trunc_42.json"))
    assert saved["truncation"] == "bootstrap"
    assert bad["status"] == "FAILED" and "truncation" in bad["error_message"]
