"""The bookkeeping half of weight coherence, on CPU tensors (flat_params needs only the library's
layout query): after every writer of coherence_util.WRITERS the staleness keys move or the flat
buffer is a new one, the parameters are views of the flat buffer at their layout offsets and it
holds the written weights, a deep copy shares no storage -- and the visibility condition that
gives the GPU matrix (test_weight_coherence_gpu.py) its teeth, asserted on the float64 reference
for the seeds and shapes used there.

The fused update (writer g) runs kernels: its row of this file is in the GPU matrix."""

import copy

import pytest
import torch

import coherence_util as cu

CPU = torch.device("cpu")
CPU_WRITERS = [w for w in cu.WRITERS if w != "g-fused_update"]


def _keys(agent):
    from hwy.ppo_native import _param_versions, flat_params
    from training.routine import _eval_key

    flat, _, _, params = flat_params(agent)
    return flat, _param_versions(agent, flat, params), _eval_key(agent, 5, 42)


def _assert_views(agent, want=None):
    """every parameter is a view of the flat buffer at its layout offset, which holds `want`"""
    from hwy.ppo_native import _PARAM_ORDER, flat_params, param_layout

    flat, grads, offs, params = flat_params(agent)
    S, H = cu._dims(agent)
    assert offs == param_layout(S, H)[0]
    named = dict(agent.actor_critic.named_parameters())
    assert set(named) == set(_PARAM_ORDER)
    for name, off, p in zip(_PARAM_ORDER, offs, params):
        assert named[name] is p, name
        assert p.data_ptr() == flat[off:].data_ptr(), name
        assert p._base is flat or p.data.untyped_storage().data_ptr() == flat.untyped_storage().data_ptr()
        if want is not None:
            assert torch.equal(flat[off:off + p.numel()].view_as(p), want[name]), name
            assert torch.equal(p.detach(), want[name]), name


@pytest.mark.parametrize("shape", cu.SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
def test_one_stale_tensor_is_visible_in_the_reference(shape):
    S, H = shape
    old = cu.cpu_state(cu.make_agent(S, H, cu.SEED_OLD, CPU, backend="torch"))
    s, noise, _, _ = cu.inputs(S)
    worst = cu.assert_visible(S, H, old, cu.new_state(S, H), s, noise)
    print(f"{shape}: the least visible stale tensor is {worst:.1f} allowances away")


@pytest.mark.parametrize("shape", cu.SHAPES, ids=lambda s: f"{s[0]}-{s[1]}")
@pytest.mark.parametrize("writer", ["e-torch_eager_update", "f-torch_graph_update"])
def test_one_stale_tensor_is_visible_after_an_update(shape, writer):
    S, H = shape
    agent = cu.make_agent(S, H, cu.SEED_OLD, CPU, backend="torch")
    old = cu.cpu_state(agent)
    cu.WRITERS[writer][0](agent, None)
    s, noise, _, _ = cu.inputs(S)
    worst = cu.assert_visible(S, H, old, cu.cpu_state(agent), s, noise)
    print(f"{shape} {writer}: the least visible stale tensor is {worst:.1f} allowances away")


@pytest.mark.parametrize("writer", CPU_WRITERS)
@pytest.mark.parametrize("shape", [(20, 64), (20, 256)], ids=lambda s: f"{s[0]}-{s[1]}")
def test_writer_moves_a_key_or_the_buffer_and_leaves_views(shape, writer):
    S, H = shape
    agent = cu.make_agent(S, H, cu.SEED_OLD, CPU, backend="torch")
    old = cu.cpu_state(agent)
    flat0, versions0, eval0 = _keys(agent)
    _assert_views(agent, old)
    fn, kind = cu.WRITERS[writer]
    sd = cu.new_state(S, H)
    holder = fn(agent, sd)
    flat1, versions1, eval1 = _keys(holder)
    assert flat1 is not flat0 or (versions1 != versions0 and eval1 != eval0), writer
    if writer == "m-deepcopy":
        assert holder is not agent and flat1 is not flat0
    want = cu.cpu_state(holder) if kind == "update" else sd
    if kind == "update":
        assert any(not torch.equal(want[k], old[k]) for k in want)
        assert all(torch.isfinite(v).all() for v in want.values())
    else:
        for k in sd:
            assert torch.equal(want[k], holder.actor_critic.state_dict()[k]), k
    _assert_views(holder, want)
    if holder is not agent:  # the original of a deep copy is as it was
        _assert_views(agent, old)
        assert _keys(agent) == (flat0, versions0, eval0) or _keys(agent)[0] is flat0


def test_silent_writes_move_nothing_until_params_written():
    """p.data.copy_() and torch._foreach_copy_ over .data bump no counter (why params_written()
    exists); the call moves the tile images' key and the evaluation memo's"""
    S, H = 20, 64
    sd = cu.new_state(S, H)
    for idiom in ("copy", "foreach"):
        agent = cu.make_agent(S, H, cu.SEED_OLD, CPU, backend="torch")
        flat0, versions0, eval0 = _keys(agent)
        named = list(agent.actor_critic.named_parameters())
        if idiom == "copy":
            for n, p in named:
                p.data.copy_(sd[n])
        else:
            torch._foreach_copy_([p.data for _, p in named], [sd[n] for n, _ in named])
        assert _keys(agent) == (flat0, versions0, eval0)
        learner = agent._learner_for(64, 32, 2, False)
        agent.params_written()
        flat1, versions1, eval1 = _keys(agent)
        assert flat1 is flat0 and versions1 != versions0 and eval1 != eval0
        assert learner not in agent._learners.values()
        _assert_views(agent, sd)


def test_deep_copy_shares_no_storage():
    S, H = 20, 64
    agent = cu.make_agent(S, H, cu.SEED_OLD, CPU, backend="torch")
    cu.w_torch_eager_update(agent, None)  # optimizer state exists
    _keys(agent)
    twin = copy.deepcopy(agent)

    def storages(ag):
        ts = list(ag.actor_critic.parameters())
        ts += [p.grad for p in ag.actor_critic.parameters() if p.grad is not None]
        for st in ag.optimizer.state.values():
            ts += [v for v in st.values() if torch.is_tensor(v)]
        if getattr(ag, "_flat", None) is not None:
            ts += [ag._flat[0], ag._flat[1]]
        return {t.untyped_storage().data_ptr() for t in ts}

    _keys(twin)
    assert not storages(agent) & storages(twin)
    assert twin._fused is None and twin._learners == {} and twin.actor_critic is not agent.actor_critic
    # the copy's optimizer steps the copy's parameters, with the original's Adam state
    mine = {id(p) for p in twin.actor_critic.parameters()}
    assert {id(p) for g in twin.optimizer.param_groups for p in g["params"]} == mine
    for p, q in zip(agent.actor_critic.parameters(), twin.actor_critic.parameters()):
        assert torch.equal(p, q)
        assert torch.equal(agent.optimizer.state[p]["exp_avg"], twin.optimizer.state[q]["exp_avg"])
    # writing one leaves the other
    before = cu.cpu_state(agent)
    cu.w_load_state_dict(twin, cu.new_state(S, H))
    after = cu.cpu_state(agent)
    assert all(torch.equal(before[k], after[k]) for k in before)
