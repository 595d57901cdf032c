"""The KL stop and the lr schedule without a GPU: the control block's geometry and the argument
checks of hwy_ppo_sched_ctl_* / hwy_ppo_sched_set_lr (refused before any device call), the
options' way from an experiment's `extra` to PPOAgent, the three refusals, and backend="torch"
on the CPU -- the readable restatement of both rules -- against a loop written out by hand."""

import ctypes

import numpy as np
import pytest
import torch


def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _plan(**kw):
    """A plan that passes the library's plan checks (one 8-wave learner), fields overridable."""
    from hwy.ppo_native import PpoSchedPlan

    p = PpoSchedPlan()
    p.G, p.grid_wgrad, p.grid_wsum, p.grid_adam, p.max_steps, p.period = 1, 1, 1, 1, 4, 4
    p.present[0], p.grid_rows[0], p.lds_bytes[0] = 1, 1, 1024
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_control_block_geometry_and_struct_sizes():
    from hwy.ppo_native import PpoSchedPlan

    L = _lib()
    assert ctypes.sizeof(PpoSchedPlan) == 12 * 4  # include/hwy_ppo.h: hwy_ppo_sched_plan
    up = lambda x: (x + 255) // 256 * 256  # noqa: E731
    for G in (1, 3, 32, 33, 64, 65, 1000):
        nb, off = L.hwy_ppo_sched_ctl_bytes(G), L.hwy_ppo_sched_ctl_stopped_offset(G)
        assert off == up(8 * G) and nb == off + 2 * up(4 * G)  # the documented layout
    for G in (0, -1):
        assert L.hwy_ppo_sched_ctl_bytes(G) == -1
        assert L.hwy_ppo_sched_ctl_stopped_offset(G) == -1


def test_control_calls_refuse_bad_arguments_without_a_device():
    L = _lib()
    ok, ptr = _plan(), ctypes.c_void_p(4096)  # never dereferenced: every call is refused first
    lim, on = (ctypes.c_float * 1)(0.03), (ctypes.c_int32 * 1)(1)
    prepare, begin = L.hwy_ppo_sched_ctl_prepare, L.hwy_ppo_sched_ctl_begin
    step, set_lr = L.hwy_ppo_sched_ctl_step, L.hwy_ppo_sched_set_lr
    assert prepare(None, lim, on, ptr, None) == -1
    assert prepare(ctypes.byref(ok), None, on, ptr, None) == -1
    assert prepare(ctypes.byref(ok), lim, None, ptr, None) == -1
    assert prepare(ctypes.byref(ok), lim, on, None, None) == -1
    assert prepare(ctypes.byref(ok), lim, (ctypes.c_int32 * 1)(2), ptr, None) == -1
    assert prepare(ctypes.byref(ok), lim, (ctypes.c_int32 * 1)(-1), ptr, None) == -1
    for bad in (_plan(G=0), _plan(max_steps=0), _plan(period=0), _plan(grid_adam=0),
                _plan(grid_wsum=0), _plan(grid_wgrad=0)):
        assert prepare(ctypes.byref(bad), lim, on, ptr, None) == -1
        assert begin(ctypes.byref(bad), ptr, ptr, None) == -1
        assert step(ctypes.byref(bad), ptr, ptr, 0, None) == -1
        assert set_lr(ctypes.byref(bad), ptr, ptr, None) == -1
    none = _plan()
    none.present[0] = 0
    assert step(ctypes.byref(none), ptr, ptr, 0, None) == -1
    assert begin(None, ptr, ptr, None) == -1
    assert begin(ctypes.byref(ok), None, ptr, None) == -1
    assert begin(ctypes.byref(ok), ptr, None, None) == -1
    assert step(None, ptr, ptr, 0, None) == -1
    assert step(ctypes.byref(ok), None, ptr, 0, None) == -1
    assert step(ctypes.byref(ok), ptr, None, 0, None) == -1
    assert step(ctypes.byref(ok), ptr, ptr, -1, None) == -1
    assert set_lr(None, ptr, ptr, None) == -1
    assert set_lr(ctypes.byref(ok), None, ptr, None) == -1
    assert set_lr(ctypes.byref(ok), ptr, None, None) == -1


def test_options_reach_the_agent_and_default_to_off():
    from experiments.config import ConditionHP
    from experiments.runner import ExperimentRunner
    from ppo.agent import PPOAgent

    ag = PPOAgent(60, 2)
    assert ag.target_kl is None and ag.kl_limit is None and ag.lr_anneal_updates is None
    assert not ag.controlled and ag.lr_device() is None and ag.lr_at(7) == 1e-4
    ag = PPOAgent(60, 2, target_kl=0.02, lr_anneal_updates=10)
    assert ag.controlled and ag.kl_limit == float(np.float32(1.5 * 0.02))
    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=64, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    mk = ExperimentRunner._create_agent
    dev = torch.device("cpu")
    ag = mk(None, 60, 2, hp, None, dev, {"target_kl": 0.01, "lr_anneal_updates": 5})
    assert ag.target_kl == 0.01 and ag.lr_anneal_updates == 5
    ag = mk(None, 60, 2, hp, None, dev, {"num_envs": 8})
    assert not ag.controlled
    for bad in (dict(target_kl=-0.1), dict(target_kl=float("nan")), dict(lr_anneal_updates=0)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            PPOAgent(60, 2, **bad)


def test_the_three_refusals_name_the_option():
    from ppo.agent import PPOAgent
    from training.routine import train_with_experiment_name

    for kw in (dict(target_kl=0.02), dict(lr_anneal_updates=10)):
        name = next(iter(kw))
        with pytest.raises(ValueError, match=name):  # a process group
            PPOAgent(60, 2, process_group=object(), **kw)
        ag = PPOAgent(60, 2, hidden_dim=64, **kw)
        with pytest.raises(ValueError, match=name):  # the one-env PPOMemory loop
            ag.update(0.0)

        class OneEnv:  # not a HighwayVecEnv: train_with_experiment_name takes the one-env loop
            unwrapped = property(lambda self: self)

        with pytest.raises(ValueError, match=name):
            train_with_experiment_name(OneEnv(), ag, max_episodes=1)
        ag.check_control_dims(64, 4)
        with pytest.raises(ValueError, match=name):  # 32-row tiles
            ag.check_control_dims(16384, 2)
        odd = PPOAgent(62, 2, hidden_dim=64, **kw)  # state_dim % 4 != 0: the general path
        with pytest.raises(ValueError, match=name):
            odd.check_control_dims(64, 4)


def _data(n=128, S=12, seed=0):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    return r(n, S), r(n, 2) * 0.5, r(n), r(n), torch.randperm(n, generator=g)


def _twin_agents(**kw):
    from ppo.agent import PPOAgent

    torch.manual_seed(1)
    a = PPOAgent(12, 2, lr=3e-3, epochs=4, batch_size=32, hidden_dim=64, backend="torch", **kw)
    b = PPOAgent(12, 2, lr=3e-3, epochs=4, batch_size=32, hidden_dim=64, backend="torch")
    b.actor_critic.load_state_dict(a.actor_critic.state_dict())
    return a, b


def _hand_loop(ag, states, z, old, adv, ret, batches, limit):
    """The SB3 rule written out: per minibatch, in update order, evaluate, and unless the mean KL
    is <= limit stop before the optimizer step.  Returns (applied steps, per-step KLs)."""
    opt = torch.optim.Adam(ag.actor_critic.parameters(), lr=3e-3)
    kls, applied = [], 0
    for _ in range(ag.epochs):
        for b in batches:
            lp, v, ent = ag.actor_critic.evaluate(states[b], torch.tanh(z[b]), z[b])
            log_ratio = lp - old[b]
            ratio = torch.exp(log_ratio)
            pg = -torch.min(ratio * adv[b], torch.clamp(ratio, 0.8, 1.2) * adv[b]).mean()
            loss = pg + 0.5 * torch.nn.functional.mse_loss(v.squeeze(-1), ret[b]) \
                - 0.005 * ent.mean()
            kl = float(((ratio - 1) - log_ratio).mean().detach())
            kls.append(kl)
            if limit is not None and not (kl <= limit):
                return applied, kls
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(ag.actor_critic.parameters(), 0.5)
            opt.step()
            applied += 1
    return applied, kls


def test_torch_backend_stops_where_the_hand_written_rule_stops():
    states, z, adv, ret, perm = _data()
    _, probe = _twin_agents()
    with torch.no_grad():  # the start policy's own log-probabilities: the KL starts at 0
        old = probe.actor_critic.evaluate(states, torch.tanh(z), z)[0]
    batches = [perm[i * 32:(i + 1) * 32] for i in range(4)]
    _, kls = _hand_loop(probe, states, z, old, adv, ret, batches, None)
    j = next(j for j in range(2, 15) if kls[j] > max(kls[:j]))  # a new maximum in mid-update
    limit = float(np.float32((max(kls[:j]) + kls[j]) / 2))
    tau = limit / 1.5
    ag, hand = _twin_agents(target_kl=tau)
    assert ag.kl_limit == pytest.approx(limit, rel=1e-6)
    applied, hkls = _hand_loop(hand, states, z, old, adv, ret, batches, ag.kl_limit)
    assert applied == j and len(hkls) == j + 1
    rows = ag._run_epochs(states, z, old, adv, ret, batches)
    written, stopped = ag._last_ctl
    assert int(written) == j + 1 and bool(stopped)
    st = ag.optimizer.state[next(iter(ag.actor_critic.parameters()))]
    assert int(st["step"]) == j  # exactly the applied steps
    np.testing.assert_allclose(rows[:j + 1, 5].numpy(), np.asarray(hkls, np.float32), rtol=1e-5)
    for p, q in zip(ag.actor_critic.parameters(), hand.actor_critic.parameters()):
        torch.testing.assert_close(p, q, rtol=1e-5, atol=1e-7)
    m = ag._finish_metrics(rows, [32] * 4, ret, ret, ctl=ag._last_ctl)
    assert m["steps_applied"] == j and m["kl_stopped"] is True
    assert m["approx_kl_last"] == pytest.approx(hkls[j], rel=1e-5)
    assert m["approx_kl"] == pytest.approx(np.mean(hkls[:j]), rel=1e-4)
    # without a trip the six means are the plain aggregation's
    big, _ = _twin_agents(target_kl=1e6)
    rows = big._run_epochs(states, z, old, adv, ret, batches)
    m = big._finish_metrics(rows, [32] * 4, ret, ret, ctl=big._last_ctl)
    want = big._finish_metrics(rows, [32] * 4, ret, ret)
    assert m["steps_applied"] == 16 and m["kl_stopped"] is False
    assert set(m) - set(want) == {"steps_applied", "kl_stopped", "approx_kl_last"}
    for k, v in want.items():
        assert m[k] == pytest.approx(v, rel=1e-12)


def test_lr_schedule_follows_the_formula():
    states, z, adv, ret, perm = _data(seed=1)
    ag, _ = _twin_agents(lr_anneal_updates=4)
    old = torch.zeros(128) - 2.0
    batches = [perm[i * 32:(i + 1) * 32] for i in range(4)]
    for u in range(7):
        want = float(np.float32(3e-3 * max(1 - u / 4, 0)))
        assert ag.lr_at(u) == want
        ag._run_epochs(states, z, old, adv, ret, batches)
        assert ag.optimizer.param_groups[0]["lr"] == want, u
        ag.updates += 1  # as update_rollout counts them
    assert ag.lr_at(4) == 0.0 and ag.lr_at(100) == 0.0
