"""The three variants of the env step (plain, info, final) through ONE GroupEnvStep object and
through HighwayVecEnv.step(): the table cache and the variant dispatch they share.

Two handles of 5 envs (no wrapper, F_out 4) and 6 envs (RankPE d 4, F_out 8) -- a block holds 4
envs, so each has a partial last block -- in shuffled row order, with 4-step episodes at density 3
under hard steering, so episodes end inside the run (test_final_gpu.py's construction).  Twin
handles with the same seeds take every step solo through step_into; all comparisons are bit for
bit."""

import copy

import numpy as np
import pytest
import torch

from hwy import _abi
from hwy.native import lib
from parity_util import pe_table_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
HORIZON, N = 4, 15
SENTINEL = 0x7FC0DEAD  # a NaN payload no observation produces
SPECS = [(5, _abi.PE_NONE, 0, 42), (6, _abi.PE_RANK, 4, 77)]
PREPARES = ("hwy_step_group_prepare", "hwy_step_group_info_prepare",
            "hwy_step_group_final_prepare")


def _vec_env(n, pe, d, seed, **kw):
    from config.base_config import HIGHWAY_CONFIG
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["order"] = "shuffled"
    cfg.update(max_episode_steps=HORIZON, vehicles_density=3)
    return HighwayVecEnv(cfg, num_envs=n, device=DEV, seed_base=seed, pe_kind=pe, d_embed=d,
                         pe_table=pe_table_for(pe, d, N), **kw)


def _bufs(env):
    """(io, info, final_obs): step_into's buffers for ``env``, owned by the test."""
    from hwy.vec_env import alloc_step_info

    n = env.num_envs
    io = (torch.zeros(n, 2, device=DEV), torch.zeros_like(env.obs_buf),
          torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
          torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, device=DEV),
          torch.zeros(n, dtype=torch.int32, device=DEV))
    return io, alloc_step_info(n, DEV), torch.zeros_like(env.obs_buf)


def _hard_steering(rng, n):
    return torch.as_tensor(np.tanh(rng.normal(size=(n, 2)) * 2.0).astype(np.float32), device=DEV)


def test_one_group_object_cycles_the_variants_and_prepares_each_key_once(monkeypatch):
    from hwy.vec_env import GroupEnvStep

    counts = dict.fromkeys(PREPARES, 0)
    for name in PREPARES:
        def counting(*args, _f=getattr(lib(), name), _name=name):
            counts[_name] += 1
            return _f(*args)
        monkeypatch.setattr(lib(), name, counting)

    solo, grouped = [_vec_env(*s) for s in SPECS], [_vec_env(*s) for s in SPECS]
    try:
        for e in solo + grouped:
            e.reset()
        assert [e.obs_features for e in solo] == [4, 8]
        gstep = GroupEnvStep(grouped)
        bs, bg = [_bufs(e) for e in solo], [_bufs(e) for e in grouped]
        rng = np.random.default_rng(0)
        dones = 0

        def step(variant, what):
            """One step of ``variant`` = (with info, with final_obs) on both sides, compared."""
            with_info, with_final = variant
            for (a, _, fa), (b, _, fb) in zip(bs, bg):
                x = _hard_steering(rng, a[0].shape[0])
                a[0].copy_(x)
                b[0].copy_(x)
                fa.view(torch.int32).fill_(SENTINEL)
                fb.view(torch.int32).fill_(SENTINEL)
            for env, (a, ai, fa) in zip(solo, bs):
                env.step_into(*a, info=ai if with_info else None,
                              final_obs=fa if with_final else None)
            gstep.launch([b for b, _, _ in bg],
                         infos=[bi for _, bi, _ in bg] if with_info else None,
                         final_obs=[fb for _, _, fb in bg] if with_final else None)
            torch.cuda.synchronize()
            n = 0
            for i, ((a, ai, fa), (b, bi, fb)) in enumerate(zip(bs, bg)):
                for k in range(1, 7):  # obs, reward, terminated, truncated, ep_return, ep_length
                    assert torch.equal(a[k], b[k]), (what, i, k)
                for k in ai:
                    assert torch.equal(ai[k], bi[k]), (what, i, k)
                assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), (what, i, "final")
                done = (a[3] | a[4]).bool()
                kept = (fb.view(torch.int32) == SENTINEL).flatten(1).all(1)
                want = ~done if with_final else torch.ones_like(done)
                assert torch.equal(kept, want), (what, i, "sentinel rows")
                n += int(done.sum())
            return n

        plain, info, final_info, final = (False, False), (True, False), (True, True), (False, True)
        for t, v in enumerate((plain, info, final_info, final, plain, info)):
            dones += step(v, f"step {t}")
        assert dones >= 5  # 4-step episodes over 6 steps: every env was truncated at least once
        # four (variant, key) combinations, each prepared once; the final variant has two keys
        assert counts == {"hwy_step_group_prepare": 1, "hwy_step_group_info_prepare": 1,
                          "hwy_step_group_final_prepare": 2}
        assert len(gstep._tables) == 4
        step(final_info, "step 6")
        step(plain, "step 7")
        assert sum(counts.values()) == 4 and len(gstep._tables) == 4
        # a new seed schedule bumps launch_version: the next launch prepares once more
        for env in (solo[0], grouped[0]):
            env.set_seed_schedule(42)
        step(plain, "step 8")
        assert counts == {"hwy_step_group_prepare": 2, "hwy_step_group_info_prepare": 1,
                          "hwy_step_group_final_prepare": 2}
        for x, y in zip(solo, grouped):
            assert torch.equal(x.export_state(), y.export_state())
    finally:
        for e in solo + grouped:
            e.close()


@pytest.mark.parametrize("with_info,with_final", [(False, False), (True, False), (False, True),
                                                  (True, True)],
                         ids=["plain", "info", "final", "info-final"])
def test_step_returns_todays_info_keys_and_the_twins_tensors(with_info, with_final):
    env = _vec_env(5, _abi.PE_NONE, 0, 42, info=with_info, final_obs=with_final)
    twin = _vec_env(5, _abi.PE_NONE, 0, 42)
    keys = {"episode_return", "episode_length"}
    if with_info:
        keys |= {"speed", "crashed", "lane", "rewards", "episode_stats"}
    if with_final:
        keys |= {"final_observation", "_final_observation"}
    try:
        env.reset()
        twin.reset()
        io, ti, tf = _bufs(twin)
        rng = np.random.default_rng(0)
        dones = 0
        for t in range(HORIZON + 2):
            a = _hard_steering(rng, 5)
            obs, reward, term, trunc, info = env.step(a)
            io[0].copy_(a)
            twin.step_into(*io, info=ti if with_info else None,
                           final_obs=tf if with_final else None)
            torch.cuda.synchronize()
            assert set(info) == keys, t
            got = (obs, reward, term, trunc, info["episode_return"], info["episode_length"])
            for k, x in enumerate(got, start=1):
                assert torch.equal(x, io[k]), (t, k)
            if with_info:
                for k in ("speed", "crashed", "lane"):
                    assert torch.equal(info[k], ti[k]), (t, k)
                assert list(info["rewards"]) == list(_abi.REWARD_KEYS)
                for i, k in enumerate(_abi.REWARD_KEYS):
                    assert torch.equal(info["rewards"][k], ti["rewards"][:, i]), (t, k)
                assert torch.equal(info["episode_stats"], ti["ep_stats"]), t
            if with_final:
                assert torch.equal(info["final_observation"].view(torch.int32),
                                   tf.view(torch.int32)), t
                assert torch.equal(info["_final_observation"], (io[3] | io[4]).bool()), t
            dones += int((term | trunc).sum())
        assert dones >= 5
    finally:
        env.close()
        twin.close()
