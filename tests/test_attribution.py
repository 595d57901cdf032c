"""Per-vehicle attribution without a GPU: attribution_from / attribution_stats against a plain
loop restatement, PPOAgent.input_gradients on the CPU (torch autograd) against float64, and
agents whose first layer reads chosen observation columns only."""

import numpy as np
import pytest
import torch

from attribution_util import (assert_stats_close, attribution_loop, draw_case, grads64,
                              keep_columns, masks_of, stats_loop)

CPU = torch.device("cpu")


def _agent(S, H=64, seed=0):
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    return PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=CPU, backend="torch")


@pytest.mark.parametrize("ego", [0, 2])
@pytest.mark.parametrize("extra", [0, 4])
def test_attribution_from_matches_the_loop(ego, extra):
    from training.routine import attribution_from, attribution_stats

    B, N, F = 12, 6, 4
    base, grads, alive = draw_case(B, N, F, F + extra, seed=3 + ego + extra)
    got = attribution_from(base, grads, alive, F, ego_idx=ego)
    want = attribution_loop(base, grads, alive, F, ego)
    assert got["by_row"].dtype == torch.float64 and got["by_rank"].dtype == torch.float64
    assert int(got["count"]) == want["count"] == int(alive.sum())
    np.testing.assert_allclose(got["by_row"].numpy(), want["by_row"], rtol=1e-12, atol=0.0)
    np.testing.assert_allclose(got["by_rank"].numpy(), want["by_rank"], rtol=1e-12, atol=0.0)
    # the ranks only move mass between rows: per output and column the totals agree
    np.testing.assert_allclose(got["by_rank"].sum(1).numpy(), got["by_row"].sum(1).numpy(),
                               rtol=1e-12)
    assert_stats_close(attribution_stats(got, F, ego), stats_loop(want, F, ego))
    st = attribution_stats(got, F, ego)
    assert (st["pe_share"] is None) == (extra == 0)


def test_steps_add_up():
    from training.routine import attribution_add, attribution_from, attribution_stats

    B, N, F, Fo = 12, 6, 4, 8
    base, grads, alive = draw_case(B, N, F, Fo, seed=11)
    whole = attribution_loop(base, grads, alive, F, 0)
    total = None
    for lo, hi in ((0, 5), (5, 6), (6, 12)):
        total = attribution_add(total, attribution_from(base[lo:hi], grads[:, lo:hi],
                                                        alive[lo:hi], F))
    assert_stats_close(attribution_stats(total, F), stats_loop(whole, F, 0))


def test_all_dead_step_counts_nothing():
    from training.routine import attribution_from, attribution_stats

    B, N, F, Fo = 12, 6, 4, 8
    base, grads, _ = draw_case(B, N, F, Fo, seed=5)
    got = attribution_from(base, grads, torch.zeros(B, dtype=torch.bool), F)
    assert int(got["count"]) == 0
    assert not got["by_row"].any() and not got["by_rank"].any()
    st = attribution_stats(got, F)
    assert st["samples"] == 0 and st["pe_share"] == [None] * 3 and st["ego_share"] == [None] * 3
    assert not np.asarray(st["by_row"]).any()


def test_ranks_need_relative_xy_first():
    from training.routine import attribution_from

    B, N, F = 12, 6, 5
    base, grads, alive = draw_case(B, N, F, F, seed=7)
    for kw in (dict(features=["presence", "x", "y", "vx", "vy"]),
               dict(features=["x", "y", "vx", "vy", "presence"], absolute=True)):
        got = attribution_from(base, grads, alive, F, **kw)
        assert got["by_rank"] is None
        np.testing.assert_allclose(got["by_row"].numpy(),
                                   attribution_loop(base, grads, alive, F, 0)["by_row"],
                                   rtol=1e-12, atol=0.0)
    assert attribution_from(base, grads, alive, F,
                            features=["x", "y", "vx", "vy", "presence"])["by_rank"] is not None


def test_input_gradients_cpu_against_float64():
    S, B = 60, 33
    ag = _agent(S)
    x = torch.randn(B, S, generator=torch.Generator().manual_seed(1))
    params = list(ag.actor_critic.parameters())
    marks = [torch.full_like(p, 0.25) for p in params]
    for p, m in zip(params, marks):
        p.grad = m.clone()
    versions = [p._version for p in params]
    got = ag.input_gradients(x)
    assert list(got) == ["acceleration", "steering", "value"]
    for p, m, v in zip(params, marks, versions):
        assert torch.equal(p.grad, m) and p._version == v
    assert not x.requires_grad and x.grad is None
    ref = grads64(ag.actor_critic, x, masks_of(ag.actor_critic, x))
    for k, name in enumerate(got):
        g = got[name]
        assert g.shape == (B, S) and g.dtype == torch.float32 and not g.requires_grad
        scale = ref[k].abs().max().item()
        assert scale > 0
        assert torch.allclose(g.double(), ref[k], rtol=1e-3, atol=2e-5 * scale), name


def test_w1_reading_one_row_attributes_to_that_row_only():
    from training.routine import attribution_from, attribution_stats

    B, N, F = 16, 5, 4
    ag = _agent(N * F)
    keep_columns(ag, range(3 * F, 4 * F))
    base = torch.randn(B, N, F, generator=torch.Generator().manual_seed(2))
    g = ag.input_gradients(base.reshape(B, -1))
    grads = torch.stack([g[n] for n in ("acceleration", "steering", "value")])
    got = attribution_from(base, grads, torch.ones(B, dtype=torch.bool), F)
    off = [n for n in range(N) if n != 3]
    assert not got["by_row"][:, off, :].any()
    assert (got["by_row"][:, 3, :].sum(-1) > 0).all()
    st = attribution_stats(got, F)
    assert st["ego_share"] == [0.0, 0.0, 0.0] and st["pe_share"] is None


def test_w1_reading_the_embedding_columns_only_has_pe_share_one():
    from training.routine import attribution_from, attribution_stats

    B, N, F, Fo = 16, 5, 4, 6
    ag = _agent(N * Fo)
    keep_columns(ag, [n * Fo + f for n in range(N) for f in range(F, Fo)])
    gen = torch.Generator().manual_seed(4)
    base = torch.randn(B, N, F, generator=gen)
    obs = torch.cat([base, torch.randn(B, N, Fo - F, generator=gen)], dim=-1)
    g = ag.input_gradients(obs.reshape(B, -1))
    grads = torch.stack([g[n] for n in ("acceleration", "steering", "value")])
    st = attribution_stats(attribution_from(base, grads, torch.ones(B, dtype=torch.bool), F), F)
    assert st["pe_share"] == [1.0, 1.0, 1.0]
    assert not np.asarray(st["by_row"])[:, :, :F].any()


def test_grouped_launches_refuse_the_option():
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    def exp(seed):
        hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64,
                         d_embed=None)
        hp.steps_per_update = 64
        return Experiment(name=f"a{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                          max_episodes=12, target_reward=1e9,
                          extra={"num_envs": 4, "attribution": True}, env_config_overrides={})

    r = ExperimentRunner(HIGHWAY_CONFIG)
    with pytest.raises(ValueError, match="attribution"):
        r.launch_group([exp(42), exp(1042)])
    with pytest.raises(ValueError, match="attribution"):
        r.launch_batch([[exp(42)], [exp(7)]])


def test_attribution_needs_a_vector_env():
    from training.routine import attribution

    class OneEnv:
        unwrapped = None

    env = OneEnv()
    env.unwrapped = env
    with pytest.raises(ValueError, match="HighwayVecEnv"):
        attribution(env, _agent(20))
