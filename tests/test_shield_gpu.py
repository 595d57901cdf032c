"""What hwy/vec_env.py, ppo/rollout.py, training/routine.py and experiments/runner.py build on
hwy_lookahead: lookahead / lookahead_into / shield_into, the shielded captured rollout,
evaluate(shield=...), shield_profile, extra["shield"] / extra["eval_shields"] and every refusal.
The executed trajectories are replayed through the CPU oracle."""

from __future__ import annotations

import copy

import numpy as np
import pytest
import torch

import lookahead_util as lu
from config.base_config import HIGHWAY_CONFIG
from hwy import Shield
from oracle.oracle import OracleEnv
from parity_util import diff_state

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
S = Shield()                     # horizon 3; brake, idle, throttle; lazy
EAGER = Shield(horizon=3, lazy=False)


def _cfg(**kw):
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=8, **kw)
    return cfg


def _state(env):
    torch.cuda.synchronize()
    return env.export_state().cpu().numpy().view(np.uint32)


def _want_choice(env, state, actions, shield):
    """the shield's choice and executed actions from the oracle, for `actions` [E, 2]"""
    cand = np.concatenate([np.asarray(actions, np.float32)[:, None, :],
                           np.tile(np.asarray(shield.fallbacks, np.float32), (len(actions), 1, 1))], 1)
    out = lu.oracle_lookahead(env.hwy_config, state, cand, hold=True, horizon=shield.horizon)
    ch = lu.choose(out["steps"], out["terminated"], lazy=shield.lazy)
    return ch, cand[np.arange(len(ch)), ch], out


def _throttle_agent():
    """weights that do not depend on what ran before: a seeded init, the mean action's head
    scaled down and biased to (0.6, 0.01), so the ego accelerates into the traffic ahead"""
    from ppo.agent import PPOAgent

    torch.manual_seed(64)
    agent = PPOAgent(60, 2, lr=3e-4, epochs=2, hidden_dim=64, device=DEV, num_minibatches=4, seed=5)
    with torch.no_grad():
        head = agent.actor_critic.actor_mean[2]
        head.weight.mul_(0.05)
        head.bias.copy_(torch.atanh(torch.tensor((0.6, 0.01), dtype=torch.float64)).float())
    return agent


# ------------------------------------------------------------------- the env's methods
def test_lookahead_returns_the_oracles_values():
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv

    E, K, H = 5, 3, 4
    env = HighwayVecEnv(_cfg(), num_envs=E, device=DEV, autoreset=True, seed_base=3)
    try:
        env.reset()
        env.step(torch.zeros(E, 2, device=DEV))
        st = _state(env)
        acts = lu.candidates(E, H)[:, [0, 3, 5]]
        got = env.lookahead(acts, gamma=0.9, obs=True)
        want = lu.oracle_lookahead(env.hwy_config, st, acts, gamma=0.9)
        assert set(got) == set(lu.OUTPUTS)
        for k in lu.OUTPUTS:
            lu.same_bits(got[k].cpu().numpy(), want[k], k)
        assert "obs" not in env.lookahead(acts)
        held = env.lookahead(acts[:, :2, 0], horizon=H)
        for k in ("steps", "terminated", "ret", "ego_final"):
            lu.same_bits(held[k].cpu().numpy(), lu.oracle_lookahead(env.hwy_config, st, acts[:, :2])[k], k)
        assert np.array_equal(_state(env), st)
        with pytest.raises(ValueError, match="give horizon"):
            env.lookahead(acts[:, :, 0])
        with pytest.raises(ValueError, match="differs from"):
            env.lookahead(acts, horizon=H + 1)
        with pytest.raises(ValueError, match="unknown lookahead outputs"):
            env.lookahead_into(torch.zeros(E, K, H, 2, device=DEV), H, returns=torch.zeros(E, K, device=DEV))
    finally:
        env.close()
    one = HighwayEnv(_cfg())
    try:
        one.reset(seed=5)
        seq = lu.candidates(1, 3)[0]
        got = one.lookahead(seq, obs=True)
        st = _state(one._vec)
        want = lu.oracle_lookahead(one._vec.hwy_config, st, seq[None])
        for k in lu.OUTPUTS:
            lu.same_bits(got[k], want[k][0], f"single env {k}")
        with pytest.raises(ValueError, match=r"\[K, H, 2\]"):
            one.lookahead(seq[0])
    finally:
        one.close()


def test_shield_into_is_the_choice_rule_on_the_oracle():
    from hwy.vec_env import HighwayVecEnv

    E = 8
    env = HighwayVecEnv(_cfg(), num_envs=E, device=DEV, autoreset=True, seed_base=11)
    try:
        env.reset()
        rng = np.random.default_rng(0)
        overridden = 0
        for t in range(4):
            st = _state(env)
            a = np.tanh(rng.normal(size=(E, 2)) * np.array([0.6, 0.15])).astype(np.float32)
            at = torch.as_tensor(a, device=DEV)
            for sh in (S, EAGER, S.to_dict()):
                out = torch.full((E, 2), 9.0, device=DEV)
                chosen = torch.full((E,), -1, dtype=torch.int32, device=DEV)
                env.shield_into(sh, at, out, chosen=chosen)
                ch, ex, _ = _want_choice(env, st, a, Shield.from_dict(sh))
                assert chosen.cpu().tolist() == ch.tolist()
                lu.same_bits(out.cpu().numpy(), ex, "executed action")
            overridden += int((ch != 0).sum())
            assert np.array_equal(_state(env), st)
            env.step(out)
        assert overridden > 0, "the shield never intervened"
        assert env._shield_scratch(S) is env._shield_scratch(Shield())  # allocated once per shield
    finally:
        env.close()


# ------------------------------------------------------------------- the shielded rollout
@pytest.mark.parametrize("use_graph", [True, False])
def test_shielded_rollout(use_graph):
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    T, E = 6, 8
    cfg = _cfg()
    envs = [HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=True, seed_base=11) for _ in range(2)]
    try:
        agent = _throttle_agent()
        bufs = [RolloutBuffer(T, E, 60, 2, DEV, shield=True) for _ in range(2)]
        for env, buf in zip(envs, bufs):
            obs, _ = env.reset()
            buf.states[0].copy_(obs.reshape(E, 60))
        env, hand = envs
        buf, hb = bufs
        ora = OracleEnv(env.hwy_config)
        ora.reset()
        roll = LockstepRollout(agent, env, buf, use_graph=use_graph, shield=S)
        shape = hand.obs_buf.shape[1:]
        overridden = 0
        for it in range(4):
            roll.run()
            hb.noise.copy_(buf.noise)
            for t in range(T):
                # the unshielded agent on the same observations and noise
                agent.select_action(hb.states[t], out=(hb.actions[t], hb.pre_tanh[t], hb.log_probs[t],
                                                       hb.values[t]), noise=hb.noise[t])
                # a stand-alone shield_into on the same states
                hand.shield_into(S, hb.actions[t], hb.exec_actions[t], chosen=hb.chosen[t])
                hand.step_into(hb.exec_actions[t], hb.states[t + 1].view(E, *shape), hb.rewards[t],
                               hb.terminated[t], hb.truncated[t], hb.ep_return[t], hb.ep_length[t])
            torch.cuda.synchronize()
            for name in ("states", "actions", "pre_tanh", "log_probs", "values", "exec_actions",
                         "chosen", "rewards", "terminated", "truncated", "ep_return", "ep_length"):
                assert torch.equal(getattr(buf, name), getattr(hb, name)), (it, name)
            assert torch.equal(env.export_state(), hand.export_state()), it
            # the policy's action stands exactly where the shield chose candidate 0
            kept = buf.chosen == 0
            assert torch.equal(buf.exec_actions[kept], buf.actions[kept])
            fb = torch.tensor(S.fallbacks, device=DEV)
            assert torch.equal(buf.exec_actions[~kept], fb[(buf.chosen[~kept] - 1).long()])
            overridden += int((~kept).sum())
            # the executed trajectory through the oracle
            for t in range(T):
                o_obs, o_r, o_te, o_tr, _, _ = ora.step(buf.exec_actions[t].cpu().numpy())
                lu.same_bits(buf.rewards[t].cpu().numpy(), o_r, f"rollout {it} step {t} reward")
                assert buf.terminated[t].cpu().numpy().astype(bool).tolist() == o_te.tolist()
                assert buf.truncated[t].cpu().numpy().astype(bool).tolist() == o_tr.tolist()
                lu.same_bits(buf.states[t + 1].cpu().numpy().reshape(o_obs.shape), o_obs, "obs")
            roll.start_next()
            hb.states[0].copy_(hb.states[T])
        assert overridden > 0, "the shield never intervened"
        if use_graph:
            assert roll.stats["rollout_replay"] >= 1, roll.stats
        keys = {LockstepRollout(agent, env, buf, shield=s)._launch_key() for s in (S, EAGER, None)}
        assert len(keys) == 3, "the shield is not part of the launch key"
    finally:
        for e in envs:
            e.close()


def test_rollout_without_a_shield_is_what_it_was():
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    T, E = 6, 8
    envs = [HighwayVecEnv(_cfg(), num_envs=E, device=DEV, autoreset=True, seed_base=11) for _ in range(2)]
    try:
        agent = _throttle_agent()
        bufs = [RolloutBuffer(T, E, 60, 2, DEV) for _ in range(2)]
        assert bufs[0].exec_actions is None and bufs[0].chosen is None
        for env, buf in zip(envs, bufs):
            obs, _ = env.reset()
            buf.states[0].copy_(obs.reshape(E, 60))
        (env, hand), (buf, hb) = envs, bufs
        roll = LockstepRollout(agent, env, buf, use_graph=True, shield=None)
        assert roll.shield is None
        bare = LockstepRollout(agent, env, buf, use_graph=True)
        assert roll._launch_key() == bare._launch_key()
        shape = hand.obs_buf.shape[1:]
        for it in range(3):
            roll.run()
            hb.noise.copy_(buf.noise)
            for t in range(T):
                agent.select_action(hb.states[t], out=(hb.actions[t], hb.pre_tanh[t], hb.log_probs[t],
                                                       hb.values[t]), noise=hb.noise[t])
                hand.step_into(hb.actions[t], hb.states[t + 1].view(E, *shape), hb.rewards[t],
                               hb.terminated[t], hb.truncated[t], hb.ep_return[t], hb.ep_length[t])
            torch.cuda.synchronize()
            for name in ("states", "actions", "log_probs", "values", "rewards", "terminated",
                         "truncated", "ep_return", "ep_length"):
                assert torch.equal(getattr(buf, name), getattr(hb, name)), (it, name)
            roll.start_next()
            hb.states[0].copy_(hb.states[T])
        assert not hasattr(env, "_shield_cache")
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------- evaluation
def _replay(env, tape, n, seed):
    """the taped episodes through the oracle: (mean return, [(oracle state, terminated)] per step)"""
    off = type(env.hwy_config).from_buffer_copy(env.hwy_config)
    off.num_envs, off.autoreset = n, 0
    ora = OracleEnv(off)
    ora.reset(seeds=np.arange(n, dtype=np.uint64) + np.uint64(seed + 1000))
    total, alive, trace = np.zeros(n, np.float64), np.ones(n, bool), []
    for rec in tape:
        assert diff_state(rec["state"].view(np.uint32), ora.state, off.vehicles_count + 1) is None
        assert rec["alive"].tolist() == alive.tolist()
        before = ora.state.copy()
        _, r, te, tr, _, _ = ora.step(rec["executed"])
        total += np.where(alive, r.astype(np.float64), 0.0)
        trace.append((before, alive.copy(), te.copy()))
        alive &= ~(te | tr)
    assert not alive.any() or len(tape) == off.max_steps + 1
    return float(total.mean()), trace


def test_evaluate_under_a_shield_and_shield_profile(monkeypatch):
    from test_eval_gpu import _agent
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    n, seed = 6, 7
    env = HighwayVecEnv(_cfg(), num_envs=4, device=DEV, autoreset=True)
    agent = _agent(64, seed=64)   # throttle 0.6, nearly straight: it runs into traffic
    try:
        base = routine.evaluate(env, agent, n, exp_seed=seed)
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base   # the memo's key is stable
        memo = env._eval_memo
        tape = []
        got = routine.evaluate(env, agent, n, exp_seed=seed, shield=S, tape=tape)
        assert env._eval_memo is memo, "the plain memo was touched"
        want, trace = _replay(env, tape, n, seed)
        assert got == want
        overridden = 0
        for rec, (before, alive, _) in zip(tape, trace):
            ch, ex, _ = _want_choice(env._eval_envs[n], before, rec["actions"], S)
            assert rec["chosen"].tolist() == ch.tolist()
            lu.same_bits(rec["executed"], ex, "executed")
            overridden += int((ch != 0)[alive].sum())
        assert overridden > 0 and got != base
        print(f"plain {base!r}, shielded {got!r}, {overridden} overrides")
        # the memo: a repeat runs nothing, another shield misses, a dict is the same shield
        monkeypatch.setattr(routine, "_run_eval_vector", lambda *a, **k: pytest.fail("the memo missed"))
        assert routine.evaluate(env, agent, n, exp_seed=seed, shield=S.to_dict()) == got
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base
        with pytest.raises(pytest.fail.Exception, match="the memo missed"):
            routine.evaluate(env, agent, n, exp_seed=seed, shield=Shield(horizon=2))
        monkeypatch.undo()

        # shield_profile: unshielded episodes, the look-ahead beside them
        tape = []
        prof = routine.shield_profile(env, agent, EAGER, num_episodes=n, exp_seed=seed, tape=tape)
        reward, trace = _replay(env, tape, n, seed)
        assert prof["reward"] == reward == base, "the profile's episodes are not the unshielded ones"
        crashes = avoidable = states = override = steps0 = 0
        for rec, (before, alive, te) in zip(tape, trace):
            assert np.array_equal(rec["executed"], rec["actions"])
            ch, _, out = _want_choice(env._eval_envs[n], before, rec["actions"], EAGER)
            assert rec["chosen"].tolist() == ch.tolist()
            safe_fallback = (out["terminated"][:, 1:] == 0).any(1)
            crashed = alive & te
            crashes += int(crashed.sum())
            avoidable += int((crashed & safe_fallback).sum())
            states += int(alive.sum())
            override += int((alive & (ch != 0)).sum())
            steps0 += int(out["steps"][alive, 0].sum())
        assert prof == {"episodes": n, "crashes": crashes, "avoidable": avoidable, "states": states,
                        "would_override": override, "mean_steps0": steps0 / states, "reward": reward}
        print(prof)
        assert crashes > 0 and override > 0
    finally:
        for e in getattr(env, "_eval_envs", {}).values():
            e.close()
        env.close()


# ------------------------------------------------------------------- the runner
def test_training_under_a_shield_and_eval_shields_land_in_the_metrics(tmp_path, monkeypatch):
    from test_sense_routine_gpu import _exp, _launch
    from training import routine

    monkeypatch.chdir(tmp_path)
    inner, seen = routine.evaluate, []

    def spy(*a, **kw):
        seen.append(kw.get("shield"))
        return inner(*a, **kw)

    monkeypatch.setattr(routine, "evaluate", spy)
    evals = {"none": None, "default": {}, "long": {"horizon": 5, "lazy": False}}
    on = _launch(_exp(42, "shield", shield=S.to_dict(), eval_shields=evals))
    js = on["json"]
    assert js["shield"] == on["metrics_history"]["shield"] == S.to_dict()
    rates = [u["shield_rate"] for u in js["policy_updates"]]
    assert rates and all(0.0 <= r <= 1.0 for r in rates) and any(r > 0 for r in rates)
    assert float(on["summary"]["shield_rate"]) == pytest.approx(rates[-1], abs=1e-4)
    booked = js["shield_rewards"]
    assert list(booked) == list(evals) and all(np.isfinite(v) for v in booked.values())
    n_own = len(seen) - len(evals)
    assert n_own >= 1 and all(s == S for s in seen[:n_own]), "a run's own evaluation was unshielded"
    assert seen[n_own:] == [None, Shield(), Shield(horizon=5, lazy=False)]
    monkeypatch.setattr(routine, "evaluate", inner)
    off = _launch(_exp(42, "noshield"))
    assert "shield" not in off["json"] and "shield_rewards" not in off["json"]
    assert "shield_rate" not in off["summary"]
    assert all("shield_rate" not in u for u in off["json"]["policy_updates"])
    assert on["metrics_history"]["episode_rewards"] != off["metrics_history"]["episode_rewards"]


# ------------------------------------------------------------------- refusals
class _Stub:
    """an env or agent with just the attributes the argument checks read"""

    def __init__(self, **kw):
        self.__dict__.update(kw)
        self.unwrapped = self


def test_refusals():
    from test_sense_routine_gpu import _exp
    from experiments.runner import ExperimentRunner
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import evaluate, shield_profile, train_with_experiment_name

    one_env, vec = _Stub(is_vector_env=False), _Stub(is_vector_env=True)
    with pytest.raises(ValueError, match="shield needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), shield={})
    with pytest.raises(ValueError, match="eval_shields needs a HighwayVecEnv"):
        train_with_experiment_name(one_env, _Stub(), eval_shields={"a": {}})
    with pytest.raises(ValueError, match="shield does not run over a process group"):
        train_with_experiment_name(vec, _Stub(_dist=object()), shield={})
    with pytest.raises(ValueError, match="shield does not go with sensor"):
        train_with_experiment_name(vec, _Stub(), shield={}, sensor={})
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        train_with_experiment_name(vec, _Stub(), shield={}, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        train_with_experiment_name(vec, _Stub(), shield={}, episode_schedule="reference")
    with pytest.raises(ValueError, match="horizon"):
        train_with_experiment_name(vec, _Stub(), shield={"horizon": 0})
    with pytest.raises(ValueError, match="eval_shields must be a dict"):
        train_with_experiment_name(vec, _Stub(), eval_shields=[{}])
    with pytest.raises(ValueError, match="unknown shield keys"):
        train_with_experiment_name(vec, _Stub(), eval_shields={"a": {"depth": 1}})
    with pytest.raises(ValueError, match=r"evaluate\(shield=...\) needs a HighwayVecEnv"):
        evaluate(one_env, _Stub(), shield={})
    with pytest.raises(ValueError, match="does not go with sensor or order"):
        evaluate(vec, _Stub(), shield={}, sensor={})
    with pytest.raises(ValueError, match="does not go with sensor or order"):
        evaluate(vec, _Stub(), shield={}, order="sorted")
    with pytest.raises(ValueError, match="shield_profile needs a HighwayVecEnv"):
        shield_profile(one_env, _Stub(), {})
    buf = RolloutBuffer(2, 2, 4, 2, DEV, shield=True)
    with pytest.raises(ValueError, match="shield does not go with sensor"):
        LockstepRollout(_Stub(), _Stub(), buf, shield={}, sensor={})
    with pytest.raises(ValueError, match='truncation="bootstrap"'):
        LockstepRollout(_Stub(), _Stub(), buf, shield={}, truncation="bootstrap")
    with pytest.raises(ValueError, match='episode_schedule="reference"'):
        LockstepRollout(_Stub(), _Stub(), buf, shield={}, episode_schedule="reference")
    with pytest.raises(ValueError, match="shield needs a vector env"):
        LockstepRollout(_Stub(), _Stub(), buf, shield={})
    with pytest.raises(ValueError, match="built with shield=True"):
        LockstepRollout(_Stub(), _Stub(shield_into=None), RolloutBuffer(2, 2, 4, 2, DEV), shield={})
    for key, val in (("shield", {}), ("shield", {"horizon": 2}), ("eval_shields", {"a": {}})):
        cell = [_exp(42, "g", **{key: val}), _exp(1042, "g", **{key: val})]
        with pytest.raises(ValueError, match=key):
            ExperimentRunner.check_batch([cell], own_schedules=True)
        with pytest.raises(ValueError, match=key):
            ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
    for extra, word in ((dict(shield={}, truncation="bootstrap"), "bootstrap"),
                        (dict(shield={}, episode_schedule="reference"), "reference"),
                        (dict(shield={}, sensor={}), "sensor")):
        res = ExperimentRunner(HIGHWAY_CONFIG).launch(_exp(42, "r", **extra))
        assert res["status"] == "FAILED" and word in res["error_message"], res
