"""Per-vehicle attribution on the GPU: PPOAgent.input_gradients through hwy_ppo_input_grad against
the torch backend, attribution() against evaluate() and against attribution_from on a tape of the
same steps, the un-embedded rows' route against the fused env, agents whose first layer reads
chosen columns only, and extra["attribution"] in ExperimentRunner.launch."""

import os

import numpy as np
import pytest
import torch

from attribution_util import (assert_stats_close, attribution_loop, grads64, keep_columns,
                              stats_loop)
from ppo_ref_util import DEV

pytestmark = pytest.mark.gpu
NAMES = ("acceleration", "steering", "value")
HORIZON = 12


def _pair(S, H=64, seed=0):
    """A torch-backend and a hip-backend agent with the same CPU-initialised weights."""
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    ref = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=torch.device("cpu"), backend="torch")
    a = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=DEV, use_graphs=False, backend="torch")
    b = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=DEV, use_graphs=False, backend="hip")
    for ag in (a, b):
        ag.actor_critic.load_state_dict(ref.actor_critic.state_dict())
    return a, b


@pytest.mark.parametrize("S,H,B", [(60, 64, 33), (120, 256, 17), (300, 128, 5)])
def test_input_gradients_fused_against_torch_backend(S, H, B):
    from hwy.ppo_native import fused_input_grad
    from training.routine import _eval_key

    a, b = _pair(S, H)
    x = torch.randn(B, S, generator=torch.Generator().manual_seed(1)).to(DEV)
    b.select_action(x, deterministic=True)  # the flat buffer exists before the key is taken
    key = _eval_key(b, 5, 0)
    grads = [p.grad.clone() for p in b.actor_critic.parameters()]
    got, t32 = b.input_gradients(x), a.input_gradients(x)
    assert _eval_key(b, 5, 0) == key
    assert all(torch.equal(p.grad, g) for p, g in zip(b.actor_critic.parameters(), grads))
    # float64 under the kernel's own ReLU decisions
    hot = torch.eye(3, device=DEV).unsqueeze(1).expand(3, B, 3).contiguous()
    d, bits = fused_input_grad(b, x, hot, want_relu_bits=True)
    sh = torch.arange(32, device=DEV, dtype=torch.int32)
    m = ((bits.unsqueeze(-1) >> sh) & 1).double().reshape(B, 4, H)
    ref = grads64(b.actor_critic, x, {k: m[:, i] for i, k in enumerate(("z1", "z2", "za", "zc"))})
    for k, n in enumerate(NAMES):
        assert torch.equal(got[n], d[k])
        scale = ref[k].abs().max().item()
        g = got[n].double()
        e_k = (g - ref[k]).abs().max().item()
        e_t = (t32[n].double() - ref[k]).abs().max().item()
        print(f"S{S} H{H} {n}: scale {scale:.3e} e_kernel {e_k:.3e} e_torch32 {e_t:.3e}")
        assert (torch.allclose(g, ref[k], rtol=1e-3, atol=2e-5 * scale)
                or torch.allclose(g, t32[n].double(), rtol=1e-3, atol=2e-5 * scale)), n


def test_hip_backend_refuses_an_unsupported_shape_as_acting_does():
    from ppo.agent import PPOAgent

    ag = PPOAgent(62, 2, lr=3e-4, hidden_dim=64, device=DEV, use_graphs=False, backend="hip")
    with pytest.raises(ValueError):
        ag.input_gradients(torch.zeros(4, 62, device=DEV))
    auto = PPOAgent(62, 2, lr=3e-4, hidden_dim=64, device=DEV, use_graphs=False)
    assert auto.input_gradients(torch.randn(4, 62, device=DEV))["value"].shape == (4, 62)


def _env(cond, d=None, E=4):
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from experiments.wrappers import make_env

    over = {"num_envs": E, "max_episode_steps": HORIZON}
    if cond != "SORTED":
        over["observation"] = {"order": "shuffled"}
    torch.manual_seed(0)
    env = make_env(Condition[cond], HIGHWAY_CONFIG, d_embed=d, env_overrides=over)
    return env.to(DEV) if hasattr(env, "to") else env


@pytest.mark.parametrize("cond,d", [("SHUFFLED_RANKPE", 8), ("SHUFFLED_DISTPE", 4),
                                    ("SHUFFLED_ROPE", 4)])
def test_unembedded_route_gives_the_fused_envs_rows(cond, d):
    from training.routine import _attribution_env_like, _eval_env_like, _obs_wrapper_of

    env = _env(cond, d)
    fused, plain = _eval_env_like(env, 4), _attribution_env_like(env, 4)
    try:
        wrap = _obs_wrapper_of(env)
        seeds = torch.arange(4, device=DEV, dtype=torch.int64) + 1000
        of, _ = fused.reset(seeds=seeds)
        op, _ = plain.reset(seeds=seeds)
        assert of.shape[-1] == op.shape[-1] + (0 if cond == "SHUFFLED_ROPE" else d)
        assert torch.equal(of.view(torch.int32), wrap(op).view(torch.int32))
        a = torch.tanh(torch.randn(4, 2, generator=torch.Generator().manual_seed(3))).to(DEV)
        of, rf, *_ = fused.step(a.contiguous())
        op, rp, *_ = plain.step(a.contiguous())
        assert torch.equal(of.view(torch.int32), wrap(op).view(torch.int32))
        assert torch.equal(rf, rp)
    finally:
        for e in (fused, plain, env):
            e.close()


@pytest.mark.parametrize("cond,d", [("SORTED", None), ("SHUFFLED_DISTPE", 4)])
def test_attribution_over_an_evaluation(cond, d):
    from ppo.agent import PPOAgent
    from training.routine import (_eval_env_like, attribution, attribution_add,
                                  attribution_from, attribution_stats, evaluate)

    env = _env(cond, d)
    try:
        N, Fo = env.observation_space.shape
        F = Fo - (d or 0)
        torch.manual_seed(1)
        ag = PPOAgent(N * Fo, 2, lr=3e-4, hidden_dim=64, device=DEV, use_graphs=False)
        tape = []
        got = attribution(env, ag, num_episodes=4, exp_seed=7, tape=tape)
        assert got["mean_reward"] == evaluate(env, ag, num_episodes=4, exp_seed=7)
        assert got["outputs"] == list(NAMES)
        # the episodes' lengths, counted on the evaluation's own (fused) env
        ev = _eval_env_like(env, 4)
        obs, _ = ev.reset(seeds=torch.arange(4, device=DEV, dtype=torch.int64) + 1007)
        lengths = torch.zeros(4, dtype=torch.int64, device=DEV)
        running = torch.ones(4, dtype=torch.bool, device=DEV)
        for _ in range(HORIZON + 1):
            a, _, _, _ = ag.select_action(obs.reshape(4, -1), deterministic=True)
            obs, _, te, tr, _ = ev.step(a.contiguous())
            lengths += running
            running &= ~(te.bool() | tr.bool())
        ev.close()
        assert not running.any() and (lengths >= 1).all() and (lengths <= HORIZON).all()
        assert got["samples"] == int(lengths.sum())
        assert torch.equal(torch.stack([al for _, _, al in tape]).sum(0), lengths)
        total, loop = None, None
        for base, obs, alive in tape:
            assert base.shape == (4, N, F) and obs.shape == (4, N * Fo)
            g = ag.input_gradients(obs)
            grads = torch.stack([g[n] for n in NAMES])
            total = attribution_add(total, attribution_from(base, grads, alive, F))
            part = attribution_loop(base.cpu(), grads.cpu(), alive.cpu(), F, 0)
            loop = part if loop is None else {
                "by_row": loop["by_row"] + part["by_row"],
                "by_rank": loop["by_rank"] + part["by_rank"],
                "count": loop["count"] + part["count"]}
        want = attribution_stats(total, F)
        for k in ("by_row", "by_rank", "pe_share", "ego_share", "samples"):
            assert got[k] == want[k], k
        assert_stats_close(got, stats_loop(loop, F, 0))
        assert (got["pe_share"] is None) == (d is None)
        assert np.asarray(got["by_rank"]).shape == (3, N, Fo)
    finally:
        env.close()


def test_crafted_first_layers_through_the_kernel():
    from training.routine import attribution_from, attribution_stats

    B, N, F, Fo = 33, 15, 4, 8
    gen = torch.Generator().manual_seed(2)
    base = torch.randn(B, N, F, generator=gen)
    obs = torch.cat([base, torch.randn(B, N, Fo - F, generator=gen)], dim=-1)
    alive = torch.ones(B, dtype=torch.bool, device=DEV)
    # W1 reads observed row 3 only
    _, ag = _pair(N * F)
    keep_columns(ag, range(3 * F, 4 * F))
    g = ag.input_gradients(base.reshape(B, -1).to(DEV))
    got = attribution_from(base.to(DEV), torch.stack([g[n] for n in NAMES]), alive, F)
    off = [n for n in range(N) if n != 3]
    assert not got["by_row"][:, off, :].any()
    assert (got["by_row"][:, 3, :].sum(-1) > 0).all()
    # W1 reads the embedding columns only
    _, ag = _pair(N * Fo)
    keep_columns(ag, [n * Fo + f for n in range(N) for f in range(F, Fo)])
    g = ag.input_gradients(obs.reshape(B, -1).to(DEV))
    st = attribution_stats(attribution_from(base.to(DEV), torch.stack([g[n] for n in NAMES]),
                                            alive, F), F)
    assert st["pe_share"] == [1.0, 1.0, 1.0]
    assert not np.asarray(st["by_row"])[:, :, :F].any()


def _exp(seed, on, cond="SORTED", d=None):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=d)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps
    extra = {"num_envs": 4, "eval_interval": 4, "log_interval": 50}
    if on:
        extra["attribution"] = True
    return Experiment(name=f"attr{int(on)}_{seed}", condition=Condition[cond], hp=hp, seed=seed,
                      max_episodes=12, target_reward=1e9, extra=extra,
                      env_config_overrides={"max_episode_steps": HORIZON})


def test_launch_with_attribution_is_the_same_training(tmp_path, monkeypatch):
    import json

    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)
    runs = {}
    for on in (False, True):
        agents = []

        class Runner(ExperimentRunner):
            def _create_agent(self, *a, **kw):
                agents.append(super()._create_agent(*a, **kw))
                return agents[-1]

        e = _exp(42, on)
        res = Runner(HIGHWAY_CONFIG).launch(e)
        assert res["status"] == "COMPLETED", res.get("error_message")
        torch.cuda.synchronize()
        res["weights"] = [p.detach().clone() for p in agents[0].actor_critic.parameters()]
        res["json"] = json.load(open(os.path.join("artifacts", "highway-ppo",
                                                  f"training_metrics_{e.name}.json")))
        runs[on] = res
    on, off = runs[True], runs[False]
    assert on["rewards"] == off["rewards"] and on["avg_rewards"] == off["avg_rewards"]
    assert all(torch.equal(a, b) for a, b in zip(on["weights"], off["weights"]))
    m1, m0 = on["metrics_history"], off["metrics_history"]
    assert "attribution" in m1 and "attribution" not in m0 and "attribution" not in off["json"]
    skip = ("attribution", "experiment_name", "timestamps")
    assert set(m1) - {"attribution"} == set(m0)
    for k in m0:
        if k in skip:
            continue
        if k == "policy_updates":
            assert [u["loss"] for u in m1[k]] == [u["loss"] for u in m0[k]]
        else:
            assert m1[k] == m0[k], k
    at = on["json"]["attribution"]
    assert at == m1["attribution"]
    N, F = 15, 4
    assert np.asarray(at["by_row"]).shape == (3, N, F) and np.asarray(at["by_rank"]).shape == (3, N, F)
    assert at["pe_share"] is None and len(at["ego_share"]) == 3 and at["samples"] >= 5
    assert np.isfinite(at["mean_reward"])


def test_grouped_launches_refuse_the_option():
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    with pytest.raises(ValueError, match="attribution"):
        ExperimentRunner.check_batch([[_exp(42, True), _exp(1042, True)]], own_schedules=True)
    with pytest.raises(ValueError, match="attribution"):
        ExperimentRunner(HIGHWAY_CONFIG).launch_group([_exp(42, True), _exp(1042, True)])
