"""Every write to the policy's weights reaches every kernel: the writer x consumer matrix.

A PPOAgent's weights live in the module's parameters (views of one flat buffer), in the FusedPPO
workspace's tile image, in the acting-only tile image, in grouped acting tables, in captured
rollout graphs and behind the evaluation memo.  Each case primes those caches with the old
weights, writes new ones through one idiom of coherence_util.WRITERS, and then checks a consumer
against the float64 forward of the module as it stands after the write, at the project's own
tolerances -- and, where paths are bit-identical by construction, against a twin agent that was
newly built with the current state dict and has no caches.  The visibility condition
(coherence_util.assert_visible) is asserted in every acting case on the weights actually written,
so a consumer that used one stale tensor is at least 9 allowances outside its tolerance.

Histories: "fresh" has no FusedPPO yet (H = 256 acts from the acting-only image, the other widths
from the params rows); "updated" has run one fused update, so acting streams FusedPPO's image at
every width."""

import copy
import types

import pytest
import torch

import coherence_util as cu
from ppo_ref_util import _check_grads, _fused_relu_masks, _grad64, _torch_grad

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

_shape_id = lambda s: f"{s[0]}-{s[1]}"  # noqa: E731
DEEP_SHAPES = ((20, 64), (20, 256))     # consumers 5 to 8: params-row acting and ppo_act_c


def _acting_bits(agent, s, noise, trunc, term):
    with torch.no_grad():
        out = agent.select_action(s, noise=noise) + agent.select_action(s, deterministic=True)
        out += (agent.value(s), agent.value_masked(s, trunc, term))
        g = agent.input_gradients(s)
    return tuple(t.clone() for t in out) + tuple(g[n].clone() for n in cu.GRAD_OUTPUTS)


def _prepared(S, H, history, **kw):
    """The SEED_OLD agent with every acting cache built on its old weights."""
    agent = cu.make_agent(S, H, cu.SEED_OLD, DEV, **kw)
    if history == "updated":
        cu.fused_update(agent)
        from hwy.ppo_native import flat_params

        assert agent._fused.current_tiles(flat_params(agent)[0]) is not None
    _acting_bits(agent, *cu.inputs(S, DEV))
    if history == "fresh":
        assert agent._fused is None
    return agent


def _twin(holder, seed=cu.SEED_NEW, **kw):
    """A newly built agent holding the holder's current state dict: no caches of any kind."""
    S, H = cu._dims(holder)
    twin = cu.make_agent(S, H, seed, DEV, **kw)
    twin.actor_critic.load_state_dict(cu.cpu_state(holder))
    return twin


def _equal(a, b, what):
    for i, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), (what, i, (x.double() - y.double()).abs().max().item())


def _check_input_grads(agent, s):
    """input_gradients against float64 autograd under the kernel's own ReLU decisions, at the
    input-gradient test's bound (test_gradients_against_float64_under_the_kernels_masks)."""
    from hwy.ppo_native import fused_input_grad
    from test_input_grad_gpu import _grad_ref, _masks

    H = cu._dims(agent)[1]
    B = s.shape[0]
    got = agent.input_gradients(s)
    cot = torch.eye(3, device=DEV).unsqueeze(1).expand(3, B, 3).contiguous()
    d, bits = fused_input_grad(agent, s, cot, want_relu_bits=True)
    masks = _masks(bits, H)
    ref = _grad_ref(agent.actor_critic, s, cot, masks, torch.float64)
    t32 = _grad_ref(agent.actor_critic, s, cot, masks, torch.float32).double()
    for k, n in enumerate(cu.GRAD_OUTPUTS):
        assert torch.equal(got[n], d[k]), n
        g = got[n].double()
        scale = ref[k].abs().max().item()
        assert scale > 0.0
        e_k, e_t = (g - ref[k]).abs().max().item(), (t32[k] - ref[k]).abs().max().item()
        ok64 = torch.allclose(g, ref[k], rtol=1e-3, atol=2e-5 * scale)
        ok32 = torch.allclose(g, t32[k], rtol=1e-3, atol=2e-5 * scale)
        assert ok64 or ok32, (n, e_k, e_t, scale)
        assert e_k <= 2 * e_t + 2e-5 * scale, (n, e_k, e_t, scale)


# ------------------------------------------------------------------ consumers 1 to 4
@pytest.mark.parametrize("writer", list(cu.WRITERS))
@pytest.mark.parametrize("history", ["fresh", "updated"])
@pytest.mark.parametrize("shape", cu.SHAPES, ids=_shape_id)
def test_acting_value_and_input_gradients_use_the_written_weights(shape, history, writer):
    S, H = shape
    s, noise, trunc, term = cu.inputs(S, DEV)
    agent = _prepared(S, H, history)
    old = cu.cpu_state(agent)
    before = _acting_bits(agent, s, noise, trunc, term)
    holder = cu.WRITERS[writer][0](agent, cu.new_state(S, H))
    new = cu.cpu_state(holder)
    worst = cu.assert_visible(S, H, old, new, s, noise)
    # 1, 2: select_action sampled and deterministic, value
    got = cu.check_acting(holder, s, noise, msg=f"{shape} {history} {writer}")
    # 3: value_masked is the deterministic value's bits on the marked rows and exactly 0 elsewhere
    mark = (trunc.bool() & ~term.bool())
    vm = holder.value_masked(s, trunc, term)
    assert torch.equal(vm[mark], got[7][mark]) and bool((vm[~mark] == 0).all())
    assert mark.any() and (~mark).any()
    # 4: input gradients
    _check_input_grads(holder, s)
    # the same bits as a twin built from the state dict, which has nothing to be stale
    _equal(_acting_bits(holder, s, noise, trunc, term),
           _acting_bits(_twin(holder), s, noise, trunc, term), "twin")
    if holder is not agent:  # the original of a deep copy still acts with its old weights
        _equal(_acting_bits(agent, s, noise, trunc, term), before, "original")
        assert all(torch.equal(v, old[k]) for k, v in cu.cpu_state(agent).items())
    print(f"{shape} {history} {writer}: least visible stale tensor {worst:.1f} allowances")


# ------------------------------------------------------------------ consumer 5: the fused step
def _step_data(agent, S):
    buf, _, perm = cu.update_buffer(agent, S, seed=6)
    n = buf.n
    g = torch.Generator().manual_seed(12)
    adv = torch.randn(n, generator=g).to(DEV)
    ret = buf.values.reshape(n) + torch.randn(n, generator=g).to(DEV)
    return (buf.states[:buf.T].reshape(n, -1).contiguous(), buf.pre_tanh.reshape(n, -1).contiguous(),
            buf.log_probs.reshape(n).contiguous(), adv, ret, perm)


@pytest.mark.parametrize("writer", list(cu.WRITERS))
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=_shape_id)
def test_fused_step_trains_the_written_weights(shape, writer):
    """F.grads of one forward_backward against float64 (_check_grads), then a whole update of the
    same geometry (so that the agent may reuse its FusedPPO): the module's parameters move.  A
    FusedPPO left on a flat buffer the parameters no longer view trains weights nobody reads."""
    from hwy.ppo_native import _PARAM_ORDER, flat_params

    S, H = shape
    mb, n = cu.N_UPD // cu.NMB_UPD, cu.N_UPD
    agent = _prepared(S, H, "updated")
    holder = cu.WRITERS[writer][0](agent, cu.new_state(S, H))
    s, z, lp, adv, ret, perm = _step_data(holder, S)
    idx = perm[:mb].contiguous()
    F = holder._fused_for(mb, cu.NMB_UPD, n)
    flat, _, offs, params = flat_params(holder)
    assert F.flat is flat and F.agent is holder
    holder._adam_to("fused")  # as update_rollout does: Adam's state is the fused step's from here
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F.counters[1].zero_()
    F.sync_params(args)
    F._fwd_bwd(args)
    torch.cuda.synchronize()
    a = _twin(holder, backend="torch")
    _torch_grad(a, s, z, lp, adv, ret, idx)
    masks, _ = _fused_relu_masks(F, a, s, idx, mb, H)
    g64 = _grad64(a, s, z, lp, adv, ret, idx, masks)
    ga = dict(a.actor_critic.named_parameters())
    gb = {name: types.SimpleNamespace(grad=F.grads[off:off + p.numel()].view_as(p))
          for name, off, p in zip(_PARAM_ORDER, offs, params)}
    _check_grads(ga, gb, g64, msg=f"{shape} {writer}")
    # a whole update through the agent: every tensor of the module moves, and stays the flat view
    before = cu.cpu_state(holder)
    steps = int(F.counters[0].item())
    cu.fused_update(holder)
    after = cu.cpu_state(holder)
    for k in before:
        assert not torch.equal(before[k], after[k]), f"{k} did not move"
    F2 = holder._fused
    assert F2.flat is flat_params(holder)[0]
    assert int(F2.counters[0].item()) == steps + cu.NMB_UPD  # Adam's step count carried on
    assert steps >= cu.NMB_UPD  # ... from the history's update, across any rebuild or copy
    # and acting reads what the update wrote
    cu.check_acting(holder, *cu.inputs(S, DEV)[:2], msg=f"{shape} {writer} after the update")


# ------------------------------------------------------------------ consumer 6: captured rollout
def _env_config(horizon=6):
    from config.base_config import HIGHWAY_CONFIG

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["vehicles_count"] = 5  # 5 rows x 4 features: S = 20
    cfg["max_episode_steps"] = horizon
    return cfg


def _buffer_bits(buf):
    return tuple(t.clone() for t in (buf.states, buf.actions, buf.pre_tanh, buf.log_probs,
                                     buf.values, buf.rewards, buf.terminated, buf.truncated,
                                     buf.dones, buf.ep_return, buf.ep_length, buf.noise))


@pytest.mark.parametrize("writer", list(cu.WRITERS))
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=_shape_id)
def test_captured_rollout_acts_with_the_written_weights(shape, writer):
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    S, H = shape
    E, T = 4, 4
    agent = _prepared(S, H, "updated")
    env = HighwayVecEnv(_env_config(), num_envs=E, device=DEV, autoreset=True, seed_base=31)
    twin_env = HighwayVecEnv(_env_config(), num_envs=E, device=DEV, autoreset=True, seed_base=31)
    try:
        buf = RolloutBuffer(T, E, S, 2, DEV)
        obs, _ = env.reset()
        buf.states[0].copy_(obs.reshape(E, S))
        roll = LockstepRollout(agent, env, buf, use_graph=True)
        for _ in range(6):
            roll.run()
            roll.start_next()
            if roll.stats["rollout_replay"]:
                break
        assert roll.stats["rollout_replay"] >= 1, roll.stats
        holder = cu.WRITERS[writer][0](agent, cu.new_state(S, H))
        roll.agent = holder
        twin = _twin(holder)
        twin.generator.set_state(holder.generator.get_state())
        twin_env.import_state(env.export_state())
        tbuf = RolloutBuffer(T, E, S, 2, DEV)
        tbuf.states[0].copy_(buf.states[0])
        for it in range(2):  # the run after the write, and the one after it (captured again)
            roll.run()
            LockstepRollout(twin, twin_env, tbuf, use_graph=False).run()
            torch.cuda.synchronize()
            _equal(_buffer_bits(buf), _buffer_bits(tbuf), f"rollout {it} after {writer}")
            roll.start_next()
            tbuf.states[0].copy_(tbuf.states[T])
        assert bool(buf.dones.any()) or True
    finally:
        env.close()
        twin_env.close()


def test_captured_rollout_before_the_first_update_at_h256():
    """H = 256 before any fused update acts from the acting-only tile image: no address a
    captured rollout keys on moves when the weights are written in place, so the image must be
    brought in step before the replay."""
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    S, H, E, T = 20, 256, 4, 4
    for writer in ("b-param_copy", "n-data_copy"):
        agent = _prepared(S, H, "fresh")
        env = HighwayVecEnv(_env_config(), num_envs=E, device=DEV, autoreset=True, seed_base=31)
        twin_env = HighwayVecEnv(_env_config(), num_envs=E, device=DEV, autoreset=True, seed_base=31)
        try:
            buf = RolloutBuffer(T, E, S, 2, DEV)
            obs, _ = env.reset()
            buf.states[0].copy_(obs.reshape(E, S))
            roll = LockstepRollout(agent, env, buf, use_graph=True)
            for _ in range(6):
                roll.run()
                roll.start_next()
                if roll.stats["rollout_replay"]:
                    break
            assert roll.stats["rollout_replay"] >= 1, roll.stats
            cu.WRITERS[writer][0](agent, cu.new_state(S, H))
            twin = _twin(agent)
            twin.generator.set_state(agent.generator.get_state())
            twin_env.import_state(env.export_state())
            tbuf = RolloutBuffer(T, E, S, 2, DEV)
            tbuf.states[0].copy_(buf.states[0])
            roll.run()
            LockstepRollout(twin, twin_env, tbuf, use_graph=False).run()
            torch.cuda.synchronize()
            _equal(_buffer_bits(buf), _buffer_bits(tbuf), writer)
        finally:
            env.close()
            twin_env.close()


# ------------------------------------------------------------------ consumer 7: grouped acting
@pytest.mark.parametrize("writer", list(cu.WRITERS))
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=_shape_id)
def test_group_act_writes_reach_the_written_agent_only(shape, writer):
    from hwy.ppo_native import GroupAct
    from ppo.agent import PPOAgent

    S, H = shape
    B = cu.ROWS
    s, noise, _, _ = cu.inputs(S, DEV, rows=2 * B)
    one = _prepared(S, H, "updated")
    # another seed's weights, and its FusedPPO image still in step: after the write the group
    # holds one learner with a current image and one whose image is retired
    torch.manual_seed(cu.SEED_NEW + 1)
    other = PPOAgent(S, 2, lr=cu.LR, epochs=1, hidden_dim=H, device=DEV, use_graphs=False,
                     num_minibatches=cu.NMB_UPD, seed=3)
    cu.fused_update(other)
    act = GroupAct([one, other], B)
    out = (torch.zeros(2 * B, 2, device=DEV), torch.zeros(2 * B, 2, device=DEV),
           torch.zeros(2 * B, device=DEV), torch.zeros(2 * B, device=DEV))
    act(s, out, noise)
    act(s, out, noise)  # from the cached table
    before = tuple(t.clone() for t in out)
    with torch.no_grad():
        solo_other = other.select_action(s[B:], noise=noise[B:])
    _equal(tuple(t[B:] for t in before), solo_other, "other, before")
    holder = cu.WRITERS[writer][0](one, cu.new_state(S, H))
    act.agents[0] = holder
    for t in out:
        t.zero_()
    act(s, out, noise)
    torch.cuda.synchronize()
    _equal(tuple(t[B:] for t in out), tuple(t[B:] for t in before), "other, after")
    with torch.no_grad():
        want = _twin(holder).select_action(s[:B], noise=noise[:B])
    _equal(tuple(t[:B] for t in out), want, f"written agent after {writer}")
    ref, _ = cu.act64(holder, s[:B], noise[:B])
    for g, r in zip(out, ref):
        torch.testing.assert_close(g[:B].double(), r, rtol=cu.RTOL, atol=cu.ATOL)


# ------------------------------------------------------------------ consumer 8: the eval memo
@pytest.mark.parametrize("writer", list(cu.WRITERS))
@pytest.mark.parametrize("shape", DEEP_SHAPES, ids=_shape_id)
def test_evaluation_after_a_write_is_the_twins_not_the_memo(shape, writer):
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    S, H = shape
    n_ep, seed = 4, 42
    agent = _prepared(S, H, "updated")
    env = HighwayVecEnv(_env_config(), num_envs=4, device=DEV, autoreset=True)
    twin_env = HighwayVecEnv(_env_config(), num_envs=4, device=DEV, autoreset=True)
    try:
        first = routine._evaluate_vector(env, agent, n_ep, seed)
        assert routine._evaluate_vector(env, agent, n_ep, seed) == first
        assert env._eval_memo[1] == first
        holder = cu.WRITERS[writer][0](agent, cu.new_state(S, H))
        want = routine._run_eval_vector(twin_env, _twin(holder), n_ep, seed)
        assert want != first, "the evaluation does not tell the two weight sets apart"
        assert routine._evaluate_vector(env, holder, n_ep, seed) == want
    finally:
        for e in (env, twin_env):
            for ev in getattr(e, "_eval_envs", {}).values():
                ev.close()
            e.close()
