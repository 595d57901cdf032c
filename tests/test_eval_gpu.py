"""`final_reward` against an independent replay: training/routine.py's _run_eval_vector,
_run_eval_group and the one-env evaluate, which until now were only compared with each other.

The actions an evaluation takes are taped; the tape is replayed through the CPU oracle
(autoreset off, reset(seeds = exp_seed + 1000 + k)); the mean of the per-episode float64 sums of
the float32 rewards up to each episode's first done must be the returned value within 4 * 2^-53
relative (only the order of the mean can differ).  Each taped action is tanh(mean) of the float64
copy of the model at the taped observation, at the acting tolerance of
test_act_matches_float64_model (rtol 1e-4, atol 2e-5).

Small everything: 5 episodes of at most 12 steps (the `max_episode_steps` key), so the host's
"all done" check at k % 8 == 7 fires once before the horizon and the loop's tail runs.  The
actor head's bias (throttle 0.6, steering 0.01 of full lock; the head's weights scaled to 0.05)
and exp_seed 42 were chosen on the CPU by replaying that constant action through the oracle
(episodes 2 and 4 crash at step 2, the others run to the time limit; with the head's small
obs-dependent part a torch agent on the CPU gives the same two kinds).  The tests assert that
both kinds occur.
"""

import copy

import numpy as np
import pytest
import torch

from config.base_config import HIGHWAY_CONFIG
from oracle.oracle import OracleEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_EP, HORIZON, EXP_SEED = 5, 12, 42
BIAS = (0.6, 0.01)          # the constant action the head's bias alone gives
REL = 4 * 2.0 ** -53


def _config():
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["max_episode_steps"] = HORIZON
    return cfg


def _agent(H, seed, device=DEV, **kw):
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    agent = PPOAgent(60, 2, lr=3e-4, epochs=2, batch_size=16, hidden_dim=H, device=device, **kw)
    with torch.no_grad():
        head = agent.actor_critic.actor_mean[2]
        head.weight.mul_(0.05)
        head.bias.copy_(torch.atanh(torch.tensor(BIAS, dtype=torch.float64)).float())
    return agent


def _vec_env(num_envs=4):
    from hwy.vec_env import HighwayVecEnv

    return HighwayVecEnv(_config(), num_envs=num_envs, device=DEV, autoreset=True)


def check_actions(agent, obs, act):
    """every taped action against tanh(mean) of the float64 copy of the model"""
    m = copy.deepcopy(agent.actor_critic).double().cpu()
    with torch.no_grad():
        mean = m.forward(torch.as_tensor(np.asarray(obs), dtype=torch.float64))[0]
    want = torch.tanh(mean)
    got = torch.as_tensor(np.asarray(act), dtype=torch.float64)
    worst = ((got - want).abs() / (2e-5 + 1e-4 * want.abs())).max().item()
    print(f"actions: worst error / (2e-5 + 1e-4 |ref|) {worst:.3e} over {got.shape[0]} rows")
    torch.testing.assert_close(got, want, rtol=1e-4, atol=2e-5)
    assert (want - torch.tensor(BIAS, dtype=torch.float64)).abs().max() > 1e-4  # it reads the obs


def replay(cfg, seeds, obs_tape, act_tape):
    """The tape through the oracle: per-episode float64 sums of the float32 rewards up to the
    first done, the step of that done, whether it was a crash, and the reward rows.  The taped
    observations of the episodes still running must be the oracle's, bit for bit."""
    n = len(seeds)
    c = type(cfg).from_buffer_copy(cfg)
    c.num_envs, c.autoreset = n, 0
    ora = OracleEnv(c)
    obs = ora.reset(seeds=np.asarray(seeds, np.uint64))
    total, alive = np.zeros(n, np.float64), np.ones(n, bool)
    done_at, crashed, rows = np.zeros(n, int), np.zeros(n, bool), []
    for k, (o, a) in enumerate(zip(obs_tape, act_tape)):
        np.testing.assert_array_equal(np.asarray(o).reshape(n, -1)[alive], obs.reshape(n, -1)[alive],
                                      err_msg=f"taped observation at step {k}")
        obs, r, te, tr, _, _ = ora.step(np.asarray(a, np.float32).reshape(n, 2))
        assert r.dtype == np.float32
        total += np.where(alive, r.astype(np.float64), 0.0)
        first = alive & (te | tr)
        done_at[first], crashed[first] = k + 1, te[first]
        alive &= ~(te | tr)
        rows.append(r)
    assert not alive.any(), "the tape ends before every episode does"
    return total, done_at, crashed, np.stack(rows)


def assert_both_kinds(done_at, crashed):
    assert (crashed & (done_at < 8)).any(), (done_at, crashed)          # a crash before step 8
    assert (~crashed & (done_at == HORIZON)).any(), (done_at, crashed)   # a run to the time limit


class StepTape:
    """wraps an eval env's step: the outputs of every step, and optionally other rewards after
    an episode's end"""

    def __init__(self, ev, spoil=False):
        self.ev, self.inner, self.spoil = ev, ev.step, spoil
        self.rows, self.over = [], None
        ev.step = self

    def __call__(self, a):
        obs, r, te, tr, info = self.inner(a)
        if self.over is None:
            self.over = torch.zeros_like(te, dtype=torch.bool)
        if self.spoil:   # an episode that ended earlier: whatever it reports now must not count
            r.copy_(torch.where(self.over, torch.full_like(r, 1e6), r))
        self.rows.append(tuple(x.clone() for x in (r, te, tr, info["episode_return"])))
        self.over |= te.bool() | tr.bool()
        return obs, r, te, tr, info

    def close(self):
        self.ev.step = self.inner


def tape_select_action(agent, monkeypatch):
    tape = []
    inner = agent.select_action

    def taped(state, deterministic=False, **kw):
        out = inner(state, deterministic=deterministic, **kw)
        assert deterministic
        s = state.detach().cpu().numpy() if isinstance(state, torch.Tensor) else np.array(state)
        a = out[0].detach().cpu().numpy() if isinstance(out[0], torch.Tensor) else np.array(out[0])
        tape.append((s.copy(), a.copy()))
        return out

    monkeypatch.setattr(agent, "select_action", taped)
    return tape


def check_against_replay(value, cfg, seeds, obs_tape, act_tape, ep_returns=None):
    """value: what the evaluation returned.  ep_returns (optional): [steps, n] the kernel's own
    ep_return output per step."""
    total, done_at, crashed, rew = replay(cfg, seeds, obs_tape, act_tape)
    want = float(np.mean(total))
    print(f"value {value!r}, replay {want!r}: relative error {abs(value - want) / abs(want):.2e} (allowed {REL:.2e})")
    assert abs(value - want) <= REL * abs(want), (value, want)
    if ep_returns is not None:
        for e in range(len(seeds)):
            k = done_at[e]
            bound = k * 2.0 ** -24 * float(np.abs(rew[:k, e].astype(np.float64)).sum())
            got = float(ep_returns[k - 1][e])
            print(f"episode {e}: ep_return {got!r} against the float64 sum {total[e]!r}: error "
                  f"{abs(got - total[e]):.2e} (allowed {bound:.2e})")
            assert abs(got - total[e]) <= bound, (e, got, total[e], bound)
    return total, done_at, crashed


@pytest.mark.parametrize("H", [64, 128])
def test_run_eval_vector_against_the_oracles_replay(H, monkeypatch):
    from training import routine

    env, agent = _vec_env(), _agent(H, seed=H)
    ev = routine._eval_env_like(env, N_EP)
    env._eval_envs = {N_EP: ev}
    try:
        tape, steps = tape_select_action(agent, monkeypatch), StepTape(ev)
        value = routine._run_eval_vector(env, agent, N_EP, EXP_SEED)
        steps.close()
        # the host's check at k = 7 found episodes running; the loop's last pass is past the horizon
        assert len(tape) == HORIZON + 1 and len(steps.rows) == HORIZON + 1
        obs_tape, act_tape = [t[0] for t in tape], [t[1] for t in tape]
        seeds = EXP_SEED + 1000 + np.arange(N_EP)
        ep_ret = [row[3].cpu().numpy() for row in steps.rows]
        total, done_at, crashed = check_against_replay(value, ev.hwy_config, seeds, obs_tape[:HORIZON],
                                                       act_tape[:HORIZON], ep_ret)
        assert_both_kinds(done_at, crashed)
        alive_rows = [np.asarray(o)[done_at > k] for k, o in enumerate(obs_tape[:HORIZON])]
        alive_acts = [np.asarray(a)[done_at > k] for k, a in enumerate(act_tape[:HORIZON])]
        check_actions(agent, np.concatenate(alive_rows), np.concatenate(alive_acts))
        print(f"H={H}: value {value!r}, episodes end at {done_at.tolist()}, crashed {crashed.tolist()}")

        # rewards after an episode's end contribute nothing: a twin run whose env reports 1e6
        # for every ended episode returns the same value
        spoiled = StepTape(ev, spoil=True)
        again = routine._run_eval_vector(env, agent, N_EP, EXP_SEED)
        spoiled.close()
        assert any((row[0] == 1e6).any().item() for row in spoiled.rows)
        assert again == value
    finally:
        env.close()
        ev.close()


def test_run_eval_group_against_the_oracles_replay(monkeypatch):
    """three items, two of width 64 and one of 128, in the grouped loop: each item's value
    against the replay of its own tape (taken around the grouped env launch)"""
    from hwy import vec_env as ve
    from training import routine

    items = [(_vec_env(), _agent(H, seed=s), s) for H, s in ((64, 42), (128, 7), (64, 123))]
    launch = ve.GroupEnvStep.launch
    tapes = [[] for _ in items]

    def taped(self, ios, infos=None, final_obs=None):
        torch.cuda.synchronize()
        before = [(io[1].cpu().numpy().copy(), io[0].cpu().numpy().copy()) for io in ios]
        launch(self, ios, infos, final_obs)
        torch.cuda.synchronize()
        for t, io, b in zip(tapes, ios, before):
            t.append(b + (io[2].cpu().numpy().copy(),))

    monkeypatch.setattr(ve.GroupEnvStep, "launch", taped)
    vector_calls = []
    monkeypatch.setattr(routine, "_run_eval_vector", lambda *a, **k: vector_calls.append(a))
    try:
        values = routine._run_eval_group(items, N_EP)
        assert not vector_calls and all(len(t) == HORIZON + 1 for t in tapes)
        kinds = []
        for (env, agent, seed), tape, value in zip(items, tapes, values):
            ev = env._eval_envs[N_EP]
            seeds = seed + 1000 + np.arange(N_EP)
            obs_tape = [t[0].reshape(N_EP, -1) for t in tape[:HORIZON]]
            act_tape = [t[1] for t in tape[:HORIZON]]
            total, done_at, crashed = check_against_replay(value, ev.hwy_config, seeds, obs_tape, act_tape)
            kinds.append((done_at, crashed))
            check_actions(agent, np.concatenate([o[done_at > k] for k, o in enumerate(obs_tape)]),
                          np.concatenate([a[done_at > k] for k, a in enumerate(act_tape)]))
            print(f"seed {seed}: value {value!r}, episodes end at {done_at.tolist()}, crashed {crashed.tolist()}")
        assert_both_kinds(np.concatenate([k[0] for k in kinds]), np.concatenate([k[1] for k in kinds]))
    finally:
        for env, _, _ in items:
            for ev in getattr(env, "_eval_envs", {}).values():
                ev.close()
            env.close()


def test_evaluate_on_the_one_env_facade_against_the_oracles_replay(monkeypatch):
    from hwy.single_env import HighwayEnv
    from training import routine

    env, agent = HighwayEnv(_config(), device=DEV), _agent(64, seed=64)
    try:
        tape = tape_select_action(agent, monkeypatch)
        value = routine.evaluate(env, agent, num_episodes=N_EP, exp_seed=EXP_SEED)
        cfg = env.vec_env.hwy_config
        totals, ends, crashes, at = [], [], [], 0
        for ep in range(N_EP):   # the tape is the episodes one after another
            c = type(cfg).from_buffer_copy(cfg)
            ora = OracleEnv(c)
            obs = ora.reset(seeds=np.array([EXP_SEED + 1000 + ep], np.uint64))
            total, k = 0.0, 0
            while True:
                s, a = tape[at]
                np.testing.assert_array_equal(s.reshape(-1), obs.reshape(-1))
                obs, r, te, tr, _, _ = ora.step(a.reshape(1, 2))
                total += float(r[0])
                at, k = at + 1, k + 1
                if te[0] or tr[0]:
                    break
            totals.append(total)
            ends.append(k)
            crashes.append(bool(te[0]))
        assert at == len(tape)
        want = float(np.mean(totals))
        assert abs(value - want) <= REL * abs(want), (value, want)
        assert_both_kinds(np.array(ends), np.array(crashes))
        check_actions(agent, np.stack([t[0].reshape(-1) for t in tape]), np.stack([t[1].reshape(-1) for t in tape]))
    finally:
        env.close()


def test_evaluate_many_memo_misses_after_a_weight_write_and_hits_otherwise(monkeypatch):
    """evaluate_many's memo: a hit while the weights stand; a miss after a fused update (the
    kernels write through the flat parameter buffer; no parameter's own version counter moves),
    after a torch write through the flat buffer alone, where only that buffer's version moves,
    and after load_state_dict"""
    from ppo.agent import RolloutBuffer
    from training import routine

    items = [(_vec_env(), _agent(64, seed=s), s) for s in (42, 7)]
    runs = []
    group = routine._run_eval_group
    monkeypatch.setattr(routine, "_run_eval_group",
                        lambda its, n: runs.append(len(its)) or group(its, n))
    vector = routine._run_eval_vector
    monkeypatch.setattr(routine, "_run_eval_vector",
                        lambda *a, **k: runs.append(1) or vector(*a, **k))
    try:
        first = routine.evaluate_many(items, num_episodes=N_EP)
        assert runs == [2]
        assert routine.evaluate_many(items, num_episodes=N_EP) == first and runs == [2]   # hit

        env, agent, _ = items[0]
        E, T = env.num_envs, 8
        buf = RolloutBuffer(T, E, 60, 2, DEV)
        obs, _ = env.reset()
        buf.states[0].copy_(obs.reshape(E, 60))
        for t in range(T):
            a, z, lp, v = agent.select_action(buf.states[t])
            for dst, src in ((buf.actions, a), (buf.pre_tanh, z), (buf.log_probs, lp), (buf.values, v)):
                dst[t].copy_(src)
            env.step_into(buf.actions[t], buf.states[t + 1], buf.rewards[t], buf.terminated[t],
                          buf.truncated[t], buf.ep_return[t], buf.ep_length[t])
            torch.bitwise_or(buf.terminated[t], buf.truncated[t], out=buf.dones[t])
        agent.update_rollout(buf, agent.value(buf.states[T]))
        assert getattr(agent, "_flat", None) is not None, "the update was not the fused one"
        second = routine.evaluate_many(items, num_episodes=N_EP)
        assert runs == [2, 1] and second[1] == first[1] and second[0] != first[0]
        assert routine.evaluate_many(items, num_episodes=N_EP) == second and runs == [2, 1]   # hit

        with torch.no_grad():
            agent._flat[0].mul_(0.5)   # a write through the flat buffer alone: agent.updates stands
        third = routine.evaluate_many(items, num_episodes=N_EP)
        assert runs == [2, 1, 1] and third[0] != second[0]

        other = items[1][1]
        other.actor_critic.load_state_dict(copy.deepcopy(agent.actor_critic.state_dict()))
        fourth = routine.evaluate_many(items, num_episodes=N_EP)
        assert runs == [2, 1, 1, 1] and fourth[0] == third[0] and fourth[1] != third[1]
        assert routine.evaluate_many(items, num_episodes=N_EP) == fourth and len(runs) == 4   # hit
    finally:
        for env, _, _ in items:
            for ev in getattr(env, "_eval_envs", {}).values():
                ev.close()
            env.close()
