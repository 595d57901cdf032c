"""The KL stop and the device-side learning rate of the scheduled PPO update (include/hwy_ppo.h:
hwy_ppo_sched_ctl_*, hwy_ppo_sched_set_lr; hwy/ppo_native.py GroupStep; PPOAgent(target_kl=,
lr_anneal_updates=)).  An applied step runs the solo step's kernel bodies, so the steps before a
trip are bit-identical to the plain run's: the trip decision is exact and every comparison at
the C ABI is bit equality -- no tolerance.  Learners and data: tests/klstop_util.py."""

import ctypes

import numpy as np
import pytest
import torch

from klstop_util import (DEV, LEARNERS, MAX_STEPS, PERIOD, SENTINEL, Learner, Sched, first_trip,
                         mid_update_limit)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def plain():
    """The plain scheduled update (hwy_ppo_sched_step) of the three learners, the per-step KLs
    it stored, and per learner a limit that trips in mid-update.  Left as it is."""
    sc = Sched(LEARNERS).run_eager()
    assert (sc.plan.max_steps, sc.plan.period) == (MAX_STEPS, PERIOD)
    kls = [l.metrics[:, 5].cpu().tolist() for l in sc.ls]
    picks = [mid_update_limit(k) for k in kls]
    print("stored KLs per learner:", kls, "limits, trips:", picks)
    return {"sched": sc, "snap": sc.snapshot(), "kls": kls, "limits": [p[0] for p in picks],
            "trips": [p[1] for p in picks]}


def _assert_equals_plain(l, want, spec):
    assert int(l.counters[0]) == int(l.counters[1]) == l.steps, spec
    for k, v in l.state().items():
        assert torch.equal(v, want[k]), (spec, k)
    assert torch.equal(l.metrics, want["metrics"]), spec


def _assert_stopped(l, j, plain_metrics, spec):
    """Learner l tripped in slot j: counters, metrics rows and state of hwy_ppo.h's rule."""
    assert int(l.counters[0]) == j and int(l.counters[1]) == j + 1, (spec, l.counters.tolist())
    assert torch.equal(l.metrics[:j + 1], plain_metrics[:j + 1]), spec
    assert bool((l.metrics[j + 1:] == SENTINEL).all()), spec
    want = Learner(*spec).solo_steps(j)
    for k, v in l.state().items():
        assert torch.equal(v, want.state()[k]), (spec, k, j)


def _check_run(sc, plain, limits):
    """Every learner of a control run against the rule applied to the plain run's KLs."""
    stopped = sc.stopped_at.cpu().tolist()
    for g, (spec, l) in enumerate(zip(LEARNERS, sc.ls)):
        j = None if limits[g] is None else first_trip(plain["kls"][g], limits[g])
        assert stopped[g] == (-1 if j is None else j), (spec, stopped, j)
        if j is None:
            _assert_equals_plain(l, plain["snap"][g], spec)
        else:
            _assert_stopped(l, j, plain["snap"][g]["metrics"], spec)


def test_a_stopped_update_is_the_solo_prefix(plain):
    """The core test: limits between two stored KLs trip each learner in mid-update; the rows up
    to the tripping one are the plain run's, later rows are untouched, and weights, moments and
    tile image are those of exactly j solo steps."""
    assert all(0 < j < l[3] * l[4] - 1 for j, l in zip(plain["trips"], LEARNERS))
    sc = Sched(LEARNERS, plain["limits"]).run_eager()
    assert sc.stopped_at.cpu().tolist() == plain["trips"]
    _check_run(sc, plain, plain["limits"])


def test_edges_share_a_group(plain):
    """kl_on = 0 beside stopping neighbours is the plain run; a limit of -1 trips in slot 0 with
    nothing applied; a limit above every KL never trips.  Then each role on another learner."""
    big = 2.0 * max(max(k) for k in plain["kls"]) + 1.0
    for limits in ([None, -1.0, big], [-1.0, plain["limits"][1], None],
                   [big, None, float("nan")]):
        sc = Sched(LEARNERS, limits).run_eager()
        _check_run(sc, plain, limits)
        for g, lim in enumerate(limits):
            if lim is not None and not lim >= 0:  # -1 and NaN: tripped at once
                l = sc.ls[g]
                assert sc.stopped_at[g].item() == 0 and l.counters.tolist() == [0, 1]
                assert torch.equal(l.flat, l.st["flat"]) and not bool(l.m.any() | l.v.any())


@pytest.mark.parametrize("where", ["inside", "boundary"])
def test_graph_replays_equal_eager(plain, where):
    """A captured graph of P slots plus the advance, replayed: the trip state survives replays
    and the advance.  With j the first learner's tripping slot, P = j + 1 places the trip inside
    the first replay and P = j on the first slot of the second."""
    j = plain["trips"][0]
    P = j + 1 if where == "inside" else j
    assert (j % P != 0) == (where == "inside")
    sc = Sched(LEARNERS, plain["limits"]).run_graph(P)
    assert sc.stopped_at.cpu().tolist() == plain["trips"]
    _check_run(sc, plain, plain["limits"])
    eager = Sched(LEARNERS, plain["limits"]).run_eager()
    for a, b in zip(sc.snapshot(), eager.snapshot()):
        for k in a:
            assert torch.equal(a[k], b[k]), k


def _act(l, tiles):
    """hwy_ppo_act (deterministic) of learner l's weights on 32 stored states."""
    from hwy.ppo_native import PpoActArgs, PpoDims
    from klstop_util import lib, stream

    o = [torch.zeros(32, 2, device=DEV), torch.zeros(32, 2, device=DEV),
         torch.zeros(32, device=DEV), torch.zeros(32, device=DEV)]
    a = PpoActArgs()
    a.dims = PpoDims(32, l.dims.S, l.dims.H, 2)
    a.states, a.params, a.noise = l.st["states"].data_ptr(), l.flat.data_ptr(), None
    a.action, a.pre_tanh, a.logp, a.value = (t.data_ptr() for t in o)
    a.tiles = tiles
    assert lib().hwy_ppo_act(ctypes.byref(a), stream()) == 0
    torch.cuda.synchronize()
    return o


def test_begin_clears_the_trip_and_the_image_serves_acting(plain):
    """Two updates in a row: the second starts clean -- its rows and its trips are those the rule
    gives on a plain update from the same state -- and after a stopped update acting from the
    tile image equals acting from params."""
    sc = Sched(LEARNERS, plain["limits"]).run_eager()
    assert sc.stopped_at.cpu().tolist() == plain["trips"]
    ref = Sched(LEARNERS)  # the second update from the same state, without a stop
    for l, r in zip(sc.ls, ref.ls):
        for dst, src in ((r.flat, l.flat), (r.m, l.m), (r.v, l.v)):
            dst.copy_(src)
        r.counters[0] = l.counters[0]
        r.sync()
        assert torch.equal(r.tile_image, l.tile_image)
        # acting from the stopped update's image against acting from the params: their rows for
        # H 64 / 128 (the same kernel either way), an image rebuilt from them at H = 256, where
        # acting always streams an image (the compact kernel)
        other = r.workspace.data_ptr() + r.tile_off if l.dims.H == 256 else None
        for x, y in zip(_act(l, l.workspace.data_ptr() + l.tile_off), _act(l, other)):
            assert torch.equal(x, y), l.dims.H
        l.counters[1].zero_()  # as FusedPPO.run does before an update
        l.metrics.fill_(SENTINEL)
    first = [int(l.counters[0]) for l in sc.ls]
    ref.run_eager()
    sc.run_eager()
    stopped = sc.stopped_at.cpu().tolist()
    for g, (spec, l, r) in enumerate(zip(LEARNERS, sc.ls, ref.ls)):
        j = first_trip(r.metrics[:, 5].cpu().tolist(), plain["limits"][g])
        assert stopped[g] == (-1 if j is None else j), (spec, stopped, j)
        done, rows = (l.steps, l.steps) if j is None else (j, j + 1)
        assert rows >= 1 and l.counters.tolist() == [first[g] + done, rows], spec
        assert torch.equal(l.metrics[:rows], r.metrics[:rows]), spec
        assert bool((l.metrics[rows:] == SENTINEL).all()), spec


@pytest.mark.parametrize("ctl", [False, True])
def test_set_lr_equals_a_table_prepared_with_that_lr(ctl):
    """An update after hwy_ppo_sched_set_lr(L) is bit for bit the update of a table prepared with
    args.lr = L, through the plain step call and through the control step call."""
    lrs = [1e-3, 7e-4, 2.5e-3]
    big = [1e30] * 3 if ctl else None
    want = Sched(LEARNERS, big, lrs=lrs).run_eager()
    sc = Sched(LEARNERS, big)  # prepared with the default lr
    lr_dev = torch.tensor(lrs, dtype=torch.float32, device=DEV)
    assert sc.set_lr(lr_dev) == 0
    sc.run_eager()
    for a, b in zip(sc.snapshot(), want.snapshot()):
        for k in a:
            assert torch.equal(a[k], b[k]), k
    assert all(l.counters.tolist() == [l.steps, l.steps] for l in sc.ls)


# ---------------------------------------------------------------- PPOAgent and the runner
def _rollout(S, T, E, seed):
    from ppo.agent import RolloutBuffer

    g = torch.Generator(device=DEV).manual_seed(seed)
    buf = RolloutBuffer(T, E, S, 2, DEV)
    buf.states.copy_(torch.randn(T + 1, E, S, device=DEV, generator=g))
    buf.rewards.copy_(torch.randn(T, E, device=DEV, generator=g))
    return buf, g


def _agent(backend, **kw):
    from ppo.agent import PPOAgent
    from utils.reproducibility import set_random_seeds

    set_random_seeds(3)
    return PPOAgent(60, 2, lr=3e-3, epochs=4, batch_size=32, hidden_dim=128, device=DEV,
                    seed=5, backend=backend, use_graphs=backend == "hip", **kw)


def _fill(agent, buf, gen):
    """The agent's own actions on the stored states, so that the first step's KL is ~0."""
    T = buf.T
    with torch.no_grad():
        for t in range(T):
            noise = torch.randn(buf.E, 2, device=DEV, generator=gen)
            a, z, lp, v = agent.actor_critic.act(buf.states[t], False, noise=noise)
            buf.actions[t].copy_(a)
            buf.pre_tanh[t].copy_(z)
            buf.log_probs[t].copy_(lp)
            buf.values[t].copy_(v)
        return agent.actor_critic.forward(buf.states[T])[2].squeeze(-1)


def _restated_kls(agent, buf, last_v, perm, steps):
    """A float64 CPU restatement of the update without a stop: the per-step KLs."""
    from ppo.agent import PPOAgent

    T, E = buf.T, buf.E
    n = T * E
    rew, val = buf.rewards.double().cpu(), buf.values.double().cpu()
    adv = torch.zeros(T, E, dtype=torch.float64)
    nxt, run = last_v.double().cpu(), torch.zeros(E, dtype=torch.float64)
    for t in reversed(range(T)):  # no episode ends in the stored rollout
        delta = rew[t] + agent.gamma * nxt - val[t]
        run = delta + agent.gamma * agent.lam * run
        adv[t], nxt = run, val[t]
    ret = (adv + val).reshape(n)
    adv = adv.reshape(n)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ref = PPOAgent(60, 2, lr=3e-3, epochs=agent.epochs, batch_size=agent.batch_size,
                   hidden_dim=128, device=torch.device("cpu"), backend="torch")
    ref.actor_critic.load_state_dict({k: v.cpu() for k, v in agent.actor_critic.state_dict().items()})
    ref.actor_critic.double()
    opt = torch.optim.Adam(ref.actor_critic.parameters(), lr=3e-3)
    s = buf.states[:T].reshape(n, -1).double().cpu()
    z = buf.pre_tanh.reshape(n, -1).double().cpu()
    old = buf.log_probs.reshape(n).double().cpu()
    perm = perm.cpu()
    mb = agent.batch_size
    kls = []
    for step in range(steps):
        i = step % (n // mb)
        idx = perm[i * mb:(i + 1) * mb]
        lp, v, ent = ref.actor_critic.evaluate(s[idx], torch.tanh(z[idx]), z[idx])
        lr_ = lp - old[idx]
        ratio = torch.exp(lr_)
        a = adv[idx]
        pg = -torch.min(ratio * a, torch.clamp(ratio, 0.8, 1.2) * a).mean()
        loss = pg + ref.value_coef * ((v.squeeze(-1) - ret[idx]) ** 2).mean() \
            - ref.entropy_coef * ent.mean()
        kls.append(float(((ratio - 1) - lr_).mean().detach()))
        opt.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(ref.actor_critic.parameters(), ref.max_grad_norm)
        opt.step()
    return kls


def test_fused_and_torch_learners_stop_at_the_same_step():
    """PPOAgent(target_kl) on the fused backend and on backend="torch" (the host restatement)
    from the same weights and rollout.  The limit comes from a float64 CPU restatement and is
    placed so that every KL up to the trip is at least 20 % of the limit away from it, which the
    restatement itself is checked to meet; both learners then stop at that step."""
    T, E = 8, 16
    buf, gen = _rollout(60, T, E, 11)
    probe = _agent("torch")
    last_v = _fill(probe, buf, gen)
    perm = torch.randperm(T * E, device=DEV, generator=gen)
    steps = probe.epochs * (T * E // probe.batch_size)
    kls = _restated_kls(probe, buf, last_v, perm, steps)
    print("restated KLs:", kls)
    pick = None
    for j in range(2, steps - 1):  # a trip in mid-update with the margin on both sides
        lo = max(kls[:j])
        if kls[j] > lo:
            lim = float(np.float32((lo + kls[j]) / 2))
            if all(abs(k - lim) >= 0.2 * lim for k in kls[:j + 1]):
                pick = (j, lim)
                break
    assert pick is not None, kls
    j, lim = pick
    tau = lim / 1.5
    got = {}
    for backend in ("hip", "torch"):
        ag = _agent(backend, target_kl=tau)
        assert abs(ag.kl_limit - lim) <= 1e-6 * lim
        for (_, p), (_, q) in zip(ag.actor_critic.state_dict().items(),
                                  probe.actor_critic.state_dict().items()):
            assert torch.equal(p, q)
        m = ag.update_rollout(buf, last_v, perm=perm.clone())
        got[backend] = m
        assert m["kl_stopped"] is True and m["steps_applied"] == j, (backend, m, j)
        assert not (m["approx_kl_last"] <= ag.kl_limit)
        assert all(np.isfinite(m[k]) for k in ("loss", "approx_kl", "entropy"))
    assert got["hip"]["approx_kl"] == pytest.approx(got["torch"]["approx_kl"], rel=1e-3, abs=1e-6)


def test_fused_agent_without_a_trip_equals_the_plain_fused_update():
    """A KL target that never trips, and an lr schedule at update 0, leave update_rollout's
    weights bit for bit those of the plain fused update; the next update runs at the annealed
    rate, equal to a plain agent given that rate."""
    T, E = 8, 16
    buf, gen = _rollout(60, T, E, 12)
    plain = _agent("hip")
    last_v = _fill(plain, buf, gen)
    perms = [torch.randperm(T * E, device=DEV, generator=gen) for _ in range(2)]
    ctl = _agent("hip", target_kl=1e6, lr_anneal_updates=4)
    for u, perm in enumerate(perms):
        plain.optimizer.param_groups[0]["lr"] = float(np.float32(3e-3 * (1 - u / 4)))
        mp = plain.update_rollout(buf, last_v, perm=perm.clone())
        mc = ctl.update_rollout(buf, last_v, perm=perm.clone())
        for (k, p), (_, q) in zip(plain.actor_critic.state_dict().items(),
                                  ctl.actor_critic.state_dict().items()):
            assert torch.equal(p, q), (u, k)
        assert mc["kl_stopped"] is False and mc["steps_applied"] == 16
        for k, v in mp.items():
            assert mc[k] == pytest.approx(v, rel=1e-12, abs=0), (u, k)
    assert set(mp) == {"loss", "policy_loss", "value_loss", "entropy", "clip_fraction",
                       "approx_kl", "explained_variance"}
    # and a target that does trip trains differently
    tight = _agent("hip", target_kl=1e-4)
    mt = tight.update_rollout(buf, last_v, perm=perms[0].clone())
    assert mt["kl_stopped"] is True and 0 < mt["steps_applied"] < 16
    fresh = _agent("hip")
    fresh.update_rollout(buf, last_v, perm=perms[0].clone())
    assert not all(torch.equal(p, q) for p, q in zip(tight.actor_critic.state_dict().values(),
                                                     fresh.actor_critic.state_dict().values()))


def _comparable(mh):
    out = {k: v for k, v in mh.items() if k != "timestamps"}
    out["policy_updates"] = [{k: v for k, v in u.items() if k != "time"}
                             for u in mh["policy_updates"]]
    return out


def test_runner_launch_group_with_target_kl_equals_solo_launches(tmp_path, monkeypatch):
    """launch_group with extra["target_kl"] / extra["lr_anneal_updates"] gives each experiment
    its solo launch() result; the options are recorded in the metrics."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)

    def exp(seed):
        hp = ConditionHP(lr=3e-3, clip_eps=0.2, epochs=3, batch_size=64, hidden_dim=64,
                         d_embed=None)
        hp.entropy_coef = 0.005
        hp.steps_per_update = 16 * 16
        return Experiment(name=f"kl_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                          max_episodes=16, target_reward=1e9,
                          extra={"num_envs": 16, "eval_interval": 8, "log_interval": 50,
                                 "target_kl": 0.004, "lr_anneal_updates": 3},
                          env_config_overrides={})

    cell = [exp(42), exp(1042)]
    grouped = ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
    stops = 0
    for e, b in zip(cell, grouped):
        a = ExperimentRunner(HIGHWAY_CONFIG).launch(e)
        assert a["status"] == b["status"] == "COMPLETED", (a.get("error_message"),
                                                           b.get("error_message"))
        assert a["rewards"] == b["rewards"] and a["avg_rewards"] == b["avg_rewards"]
        assert _comparable(a["metrics_history"]) == _comparable(b["metrics_history"])
        mh = b["metrics_history"]
        assert mh["target_kl"] == 0.004 and mh["lr_anneal_updates"] == 3
        assert all("steps_applied" in u for u in mh["policy_updates"])
        stops += sum(u["kl_stopped"] for u in mh["policy_updates"])
    print("updates stopped:", stops)
