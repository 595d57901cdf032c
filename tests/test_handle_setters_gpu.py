"""The env handle's setters leave no derived state stale: after any setter the handle steps bit for
bit as a twin handle created directly in the target configuration (export_state and the
observations), also when the setter falls between two replays of a captured rollout graph or
between two launches of a GroupEnvStep table.

2 groups of 4 envs, episodes of at most 4 policy steps: 12 steps run three episodes per env, so the
seeds of the second and third come from the schedule under test (checked against rng_model)."""

import copy

import numpy as np
import pytest
import torch

import coherence_util as cu
import rng_model as rm
from hwy import _abi

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
G, EPG, E, HORIZON, STEPS = 2, 4, 8, 4, 12
D = 4  # RankPE columns


def _config():
    from config.base_config import HIGHWAY_CONFIG

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["vehicles_count"] = 5
    cfg["max_episode_steps"] = HORIZON
    return cfg


def _env(num_envs=E, **kw):
    from hwy.vec_env import HighwayVecEnv

    kw.setdefault("seed_base", 100)
    return HighwayVecEnv(_config(), num_envs=num_envs, device=DEV, autoreset=True, **kw)


def _tables(n, seed=0):
    g = np.random.default_rng(seed)
    return [np.tanh(g.standard_normal(5 * D)).astype(np.float32) for _ in range(n)]


def _actions(steps=STEPS, num_envs=E, seed=0):
    g = torch.Generator().manual_seed(seed)
    a = torch.rand(steps, num_envs, 2, generator=g) * 2 - 1
    a[..., 1] *= 0.1  # gentle steering: most episodes run to the time limit
    return a.to(DEV)


def _state(env):
    return env.export_state().cpu().numpy().view(np.uint32)


def _check_seeds(env, bases=None, group_envs=None, lo=0, note=""):
    """every env's current episode seed is the schedule's for its episode counter"""
    st = _state(env)
    ep = st[_abi.F_ENV][:, _abi.E_EPISODE].astype(np.int64)
    got = rm.state_seeds(st)
    want = rm.schedule_seed(env.hwy_config, np.arange(env.num_envs), ep, bases, group_envs)
    assert np.array_equal(got, want), (note, ep.tolist(), got.tolist(), want.tolist())
    return ep


def _lockstep(envs_and_slices, actions, check=None):
    """Step every (env, slice of the action columns) through all the actions; the first env is
    compared bit for bit with the others on their slices: observations, every step output and the
    packed state.  Returns the largest episode counter reached."""
    main = envs_and_slices[0][0]
    top = 0
    for t in range(actions.shape[0]):
        outs = []
        for env, sl in envs_and_slices:
            o = env.step(actions[t, sl].contiguous())
            outs.append([x.clone() for x in o[:4]] + [o[4]["episode_return"].clone(),
                                                        o[4]["episode_length"].clone()])
        ref = outs[0]
        for (env, sl), got in zip(envs_and_slices[1:], outs[1:]):
            for i, (a, b) in enumerate(zip(ref, got)):
                assert torch.equal(a[sl], b), (t, sl, i)
            assert np.array_equal(_state(main)[:, sl], _state(env)), (t, sl)
        if check is not None:
            top = max(top, int(check(t).max()))
    return top


def test_clearing_seed_groups_restores_the_ungrouped_schedule():
    env, twin = _env(), _env()
    try:
        bases = [7, 900]
        env.set_seed_groups(bases, EPG)
        env.reset()
        acts = _actions(seed=1)
        for t in range(5):  # grouped episodes first: the grouped stride is in use
            env.step(acts[t])
        _check_seeds(env, bases, EPG, note="grouped")
        env.set_seed_groups(None)
        assert env.hwy_config.seed_stride == twin.hwy_config.seed_stride == E
        o, _ = env.reset()
        ot, _ = twin.reset()
        assert torch.equal(o, ot) and np.array_equal(_state(env), _state(twin))
        top = _lockstep([(env, slice(0, E)), (twin, slice(0, E))], _actions(),
                        check=lambda t: _check_seeds(env, note=f"ungrouped step {t}"))
        assert top >= 2, top  # three episodes: two autoresets drew from the restored schedule
        # distinct envs never share an episode seed on the ungrouped schedule
        seeds = rm.schedule_seed(env.hwy_config, np.arange(E)[:, None], np.arange(3)[None, :])
        assert len(set(seeds.ravel().tolist())) == seeds.size
    finally:
        env.close()
        twin.close()


def _solos(tables, bases, n):
    from hwy._abi import PE_RANK

    out = []
    for t, b in zip(tables, bases):
        s = _env(n, pe_kind=PE_RANK, d_embed=D, pe_table=t)
        s.set_seed_schedule(b)
        out.append(s)
    return out


def test_seed_groups_again_keeps_or_invalidates_the_per_group_rank_tables():
    from hwy._abi import PE_RANK
    from hwy.vec_env import GroupEnvStep

    tabs = _tables(4)
    env = _env(pe_kind=PE_RANK, d_embed=D, pe_table=tabs[0])
    solos = []
    try:
        env.set_seed_groups([7, 900], EPG)
        env.set_pe_table(np.concatenate(tabs[:2]))
        # the same geometry with other bases: group g still reads table g
        bases = [11, 500]
        env.set_seed_groups(bases, EPG)
        solos = _solos(tabs[:2], bases, EPG)
        o, _ = env.reset()
        for g, s in enumerate(solos):
            og, _ = s.reset()
            assert torch.equal(o[g * EPG:(g + 1) * EPG], og), g
        assert not torch.equal(o[:EPG, :, -D:], o[EPG:, :, -D:])  # the tables differ in the rows
        top = _lockstep([(env, slice(0, E))] + [(s, slice(g * EPG, (g + 1) * EPG))
                                                for g, s in enumerate(solos)], _actions(),
                        check=lambda t: _check_seeds(env, bases, EPG, note=f"step {t}"))
        assert top >= 2, top
        for s in solos:
            s.close()
        solos = []

        # another geometry: the tables mean nothing until hwy_set_pe_table is called again
        bases4 = [1, 2000, 30000, 400000]
        env.set_seed_groups(bases4, 2)
        a = _actions()[0]
        with pytest.raises(ValueError, match="hwy_set_pe_table"):
            env.reset()
        with pytest.raises(ValueError, match="hwy_set_pe_table"):
            env.step(a)
        with pytest.raises(ValueError, match="hwy_set_pe_table"):
            GroupEnvStep([env]).launch([(a, env.obs_buf, env.reward_buf, env.term_buf,
                                         env.trunc_buf, env.ep_ret_buf, env.ep_len_buf)])
        env.set_pe_table(np.concatenate(tabs))
        solos = _solos(tabs, bases4, 2)
        o, _ = env.reset()
        for g, s in enumerate(solos):
            og, _ = s.reset()
            assert torch.equal(o[g * 2:(g + 1) * 2], og), g
        _lockstep([(env, slice(0, E))] + [(s, slice(g * 2, (g + 1) * 2))
                                          for g, s in enumerate(solos)], _actions(seed=2),
                  check=lambda t: _check_seeds(env, bases4, 2, note=f"4 groups step {t}"))
        for s in solos:
            s.close()
        solos = []

        # grouping off under per-group tables: invalid too; one table makes it a plain handle
        env.set_seed_groups(None)
        with pytest.raises(ValueError, match="hwy_set_pe_table"):
            env.reset()
        env.set_pe_table(tabs[3])
        twin = _env(pe_kind=PE_RANK, d_embed=D, pe_table=tabs[3])
        solos = [twin]
        o, _ = env.reset()
        ot, _ = twin.reset()
        assert torch.equal(o, ot)
        _lockstep([(env, slice(0, E)), (twin, slice(0, E))], _actions(seed=3),
                  check=lambda t: _check_seeds(env, note=f"ungrouped step {t}"))
    finally:
        env.close()
        for s in solos:
            s.close()


# ------------------------------------------------------------------ setters between replays
def _twin_like(env, **kw):
    """a handle created directly in env's configuration, holding env's state"""
    cfg = env.hwy_config
    twin = _env(seed_base=int(cfg.seed_base), pe_kind=int(cfg.pe_kind), d_embed=int(cfg.d_embed),
                pe_table=env._pe_table, **kw)
    if getattr(env, "_groups", None) is not None:
        twin.set_seed_groups(*env._groups)
    twin.import_state(env.export_state())
    return twin


def _set_seed_schedule(env):
    env.set_seed_schedule(77)


def _reset_seed(env):
    env.reset(seed=55)


def _set_seed_groups(env):
    env.set_seed_groups([7, 900], EPG)


def _set_pe_table(env):
    env.set_pe_table(_tables(1, seed=9)[0])


def _enable_pe(env):
    # RoPE rotates in place: the observation keeps its width, so the buffers stay
    env.enable_pe(_abi.PE_ROPE, 2, np.array([0.5], np.float32))


def _import_state(env):
    env.import_state(env._saved)


# name -> (setter, keyword arguments of the handle before it)
SETTERS = {
    "set_seed_schedule": (_set_seed_schedule, {}),
    "reset_seed": (_reset_seed, {}),
    "set_seed_groups": (_set_seed_groups, {}),
    "set_pe_table": (_set_pe_table, dict(pe_kind=_abi.PE_RANK, d_embed=D, pe_table=_tables(1)[0])),
    "enable_pe": (_enable_pe, {}),
    "import_state": (_import_state, {}),
}


@pytest.mark.parametrize("name", list(SETTERS))
def test_setter_between_two_replays_of_a_captured_rollout(name):
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    setter, kw = SETTERS[name]
    env = _env(**kw)
    twin = None
    T = 4
    S = env.obs_rows * env.obs_features
    try:
        agent = cu.make_agent(S, 64, cu.SEED_OLD, DEV)
        buf = RolloutBuffer(T, E, S, 2, DEV)
        obs, _ = env.reset()
        env._saved = env.export_state().clone()
        buf.states[0].copy_(obs.reshape(E, S))
        roll = LockstepRollout(agent, env, buf, use_graph=True)
        for _ in range(6):
            roll.run()
            roll.start_next()
            if roll.stats["rollout_replay"]:
                break
        assert roll.stats["rollout_replay"] >= 1, roll.stats
        setter(env)
        if name == "reset_seed":
            buf.states[0].copy_(env.obs_buf.reshape(E, S))
        twin = _twin_like(env)
        tagent = cu.make_agent(S, 64, cu.SEED_OLD, DEV)
        tagent.generator.set_state(agent.generator.get_state())
        tbuf = RolloutBuffer(T, E, S, 2, DEV)
        tbuf.states[0].copy_(buf.states[0])
        troll = LockstepRollout(tagent, twin, tbuf, use_graph=False)
        for it in range(3):  # eager after the setter, captured again, replayed
            roll.run()
            troll.run()
            torch.cuda.synchronize()
            for a, b in zip((buf.states, buf.actions, buf.rewards, buf.terminated, buf.truncated,
                             buf.ep_return, buf.ep_length),
                            (tbuf.states, tbuf.actions, tbuf.rewards, tbuf.terminated,
                             tbuf.truncated, tbuf.ep_return, tbuf.ep_length)):
                assert torch.equal(a, b), (name, it)
            assert np.array_equal(_state(env), _state(twin)), (name, it)
            roll.start_next()
            troll.start_next()
        assert bool(buf.dones.any())  # autoresets ran under the new configuration
        groups = getattr(env, "_groups", None)
        _check_seeds(env, *(groups if groups else (None, None)), note=name)
    finally:
        env.close()
        if twin is not None:
            twin.close()


@pytest.mark.parametrize("name", list(SETTERS))
def test_setter_between_two_launches_of_a_group_env_step_table(name):
    from hwy.vec_env import GroupEnvStep

    setter, kw = SETTERS[name]
    env, other = _env(**kw), _env(seed_base=4000)
    twin = None
    try:
        env.reset()
        other.reset()
        env._saved = env.export_state().clone()
        acts = _actions(seed=4)

        def ios(t):
            return [(acts[t], e.obs_buf, e.reward_buf, e.term_buf, e.trunc_buf, e.ep_ret_buf,
                     e.ep_len_buf) for e in (env, other)]

        step = GroupEnvStep([env, other])
        step.launch(ios(0))
        step.launch(ios(1))  # from the cached table
        setter(env)
        twin = _twin_like(env)
        otwin = _twin_like(other)
        try:
            for t in range(2, STEPS):
                step.launch(ios(t))
                for e, tw in ((env, twin), (other, otwin)):
                    o = tw.step(acts[t])
                    got = (e.obs_buf, e.reward_buf, e.term_buf, e.trunc_buf, e.ep_ret_buf,
                           e.ep_len_buf)
                    want = o[:4] + (o[4]["episode_return"], o[4]["episode_length"])
                    for i, (a, b) in enumerate(zip(got, want)):
                        assert torch.equal(a, b), (name, t, i)
                    assert np.array_equal(_state(e), _state(tw)), (name, t)
        finally:
            otwin.close()
        groups = getattr(env, "_groups", None)
        _check_seeds(env, *(groups if groups else (None, None)), note=name)
    finally:
        env.close()
        other.close()
        if twin is not None:
            twin.close()
