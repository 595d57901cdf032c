"""hwy_ppo_value_masked (include/hwy_ppo.h) on the GPU: value[b] is hwy_ppo_act's deterministic
value, bit for bit, where row b is truncated and not terminated, and exactly 0.0f elsewhere; it
writes nothing else; and it agrees with the float64 torch forward at the tolerance the acting test
uses for `value` (tests/test_ppo_fused_gpu.py::test_fused_act_matches_actor_critic_act:
rtol 1e-4, atol 2e-5).

Shapes: B = 40 (two full 16-row tiles and a partial third) over every kernel family the launch
chooses between -- ppo_act with and without the tile image (H 64, 128, 384; H 256 without), the
compact ppo_act_c (H 256 with the image), the chunked kernels past S = 256 -- and B = 64 x CUs
at (60, 256, image), where the compact kernel switches to 32-row tiles."""

import copy
import ctypes
import functools

import pytest
import torch

from hwy.native import lib, stream_ptr
from hwy.ppo_native import PpoActArgs, PpoDims, _bind, _TileImage, flat_params

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
B = 40
VALUE_RTOL, VALUE_ATOL = 1e-4, 2e-5  # test_ppo_fused_gpu.py's tolerance for value
CASES = [(60, 256, True), (60, 256, False), (120, 128, True), (60, 64, False), (60, 384, True),
         (300, 256, True)]
MASKS = ["none", "all", "last", "random", "random_term"]


@functools.lru_cache(maxsize=None)
def _setup(S, H, tiles, rows):
    """One agent, its states, the acting kernel's deterministic values and the float64 forward's,
    computed once per shape and left unchanged."""
    from ppo.agent import PPOAgent

    torch.manual_seed(1000 + S + H)
    agent = PPOAgent(S, 2, hidden_dim=H, device=DEV, backend="hip")
    flat = flat_params(agent)[0]
    image = _TileImage(agent, flat, S, H) if tiles else None
    tp = image.current() if tiles else None
    states = torch.randn(rows, S, device=DEV)
    act = {k: torch.empty(rows, *shp, device=DEV)
           for k, shp in (("action", (2,)), ("pre", (2,)), ("logp", ()), ("value", ()))}
    a = PpoActArgs()
    a.dims = PpoDims(rows, S, H, 2)
    a.states, a.params, a.tiles = states.data_ptr(), flat.data_ptr(), tp
    a.action, a.pre_tanh, a.logp, a.value = (act["action"].data_ptr(), act["pre"].data_ptr(),
                                             act["logp"].data_ptr(), act["value"].data_ptr())
    assert _bind(lib()).hwy_ppo_act(ctypes.byref(a), stream_ptr()) == 0
    with torch.no_grad():
        ref64 = copy.deepcopy(agent.actor_critic).double().forward(states.double())[2].squeeze(-1)
    torch.cuda.synchronize()
    return agent, flat, image, tp, states, act["value"], ref64


def _mask(kind, rows):
    g = torch.Generator(device="cpu").manual_seed(5)
    trunc = torch.zeros(rows, dtype=torch.uint8)
    term = None
    if kind == "all":
        trunc[:] = 1
    elif kind == "last":
        trunc[rows - 1] = 1
    elif kind in ("random", "random_term"):
        trunc = (torch.rand(rows, generator=g) < 0.3).to(torch.uint8)
        trunc[17] = 1  # one marked row in the middle tile whatever the draw
        if kind == "random_term":
            term = (torch.rand(rows, generator=g) < 0.4).to(torch.uint8)
            term[17] = 0
            term[torch.nonzero(trunc)[0]] = 1  # an overlap whatever the draw
    marked = trunc.bool() if term is None else trunc.bool() & ~term.bool()
    return (trunc.to(DEV), None if term is None else term.to(DEV), marked.to(DEV))


def _masked(flat, tp, states, S, H, trunc, term, noise=None, with_outputs=False):
    rows = states.shape[0]
    out = torch.full((rows,), float("nan"), device=DEV)
    a = PpoActArgs()
    a.dims = PpoDims(rows, S, H, 2)
    a.states, a.params, a.tiles = states.data_ptr(), flat.data_ptr(), tp
    a.value = out.data_ptr()
    guard = None
    if with_outputs:  # non-NULL action / pre_tanh / logp must stay untouched
        guard = torch.full((5, rows), 7.0, device=DEV)
        a.action, a.pre_tanh, a.logp = (guard[0:2].data_ptr(), guard[2:4].data_ptr(),
                                        guard[4].data_ptr())
    rc = _bind(lib()).hwy_ppo_value_masked(ctypes.byref(a), trunc.data_ptr(),
                                           None if term is None else term.data_ptr(),
                                           stream_ptr())
    torch.cuda.synchronize()
    return rc, out, guard


def _check(out, marked, act_value, ref64):
    assert torch.equal(out[marked].view(torch.int32), act_value[marked].view(torch.int32))
    # exactly +0.0f, not merely == 0
    assert bool((out[~marked].view(torch.int32) == 0).all())
    torch.testing.assert_close(out[marked].double(), ref64[marked], rtol=VALUE_RTOL,
                               atol=VALUE_ATOL)


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("S,H,tiles", CASES)
def test_masked_values_are_the_acting_values(S, H, tiles, kind):
    agent, flat, image, tp, states, act_value, ref64 = _setup(S, H, tiles, B)
    trunc, term, marked = _mask(kind, B)
    if kind == "none":
        assert not bool(marked.any())
    elif kind == "last":
        assert marked.nonzero().flatten().tolist() == [B - 1]
    elif kind == "random_term":
        assert bool((trunc.bool() & term.bool()).any()) and bool(marked.any())
        assert not bool(marked.all())
    rc, out, guard = _masked(flat, tp, states, S, H, trunc, term, with_outputs=(kind == "random"))
    assert rc == 0
    _check(out, marked, act_value, ref64)
    if guard is not None:
        assert bool((guard == 7.0).all())


def test_the_32_row_compact_tile():
    S, H = 60, 256
    rows = 64 * torch.cuda.get_device_properties(0).multi_processor_count
    agent, flat, image, tp, states, act_value, ref64 = _setup(S, H, True, rows)
    g = torch.Generator(device="cpu").manual_seed(9)
    trunc = (torch.rand(rows, generator=g) < 0.02).to(torch.uint8)  # most 32-row tiles hold none
    trunc[rows - 1] = 1
    term = (torch.rand(rows, generator=g) < 0.3).to(torch.uint8)
    term[rows - 1] = 0
    marked = (trunc.bool() & ~term.bool()).to(DEV)
    tiles_marked = marked.view(-1, 32).any(1)
    assert bool(tiles_marked.any()) and not bool(tiles_marked.all())
    rc, out, _ = _masked(flat, tp, states, S, H, trunc.to(DEV), term.to(DEV))
    assert rc == 0
    _check(out, marked, act_value, ref64)


def test_python_entry_points():
    """fused_value_masked / PPOAgent.value_masked: the acting path's tiles, out= rows, the torch
    fallback, and the refusals."""
    from hwy.ppo_native import fused_act, fused_value_masked
    from ppo.agent import PPOAgent

    S, H = 60, 256
    torch.manual_seed(3)
    agent = PPOAgent(S, 2, hidden_dim=H, device=DEV, backend="hip")
    states = torch.randn(B, S, device=DEV)
    trunc, term, marked = _mask("random_term", B)
    want = fused_act(agent, states, deterministic=True)[3]
    got = fused_value_masked(agent, states, trunc, term)
    rows = torch.full((2, B), float("nan"), device=DEV)
    res = agent.value_masked(states, trunc, term, out=rows[1])
    torch.cuda.synchronize()
    assert res.data_ptr() == rows[1].data_ptr()
    for x in (got, rows[1]):
        assert torch.equal(x[marked], want[marked]) and bool((x[~marked] == 0).all())
    assert bool(torch.isnan(rows[0]).all())
    no_term = agent.value_masked(states, trunc)
    assert torch.equal(no_term[trunc.bool()], want[trunc.bool()])
    # the torch fallback computes the same thing to fp32 rounding
    tagent = PPOAgent(S, 2, hidden_dim=H, device=DEV, backend="torch")
    tagent.actor_critic.load_state_dict(agent.actor_critic.state_dict())
    tv = tagent.value_masked(states, trunc, term)
    assert bool((tv[~marked] == 0).all())
    torch.testing.assert_close(tv[marked], want[marked], rtol=VALUE_RTOL, atol=VALUE_ATOL)
    with pytest.raises(ValueError, match="truncated"):
        fused_value_masked(agent, states, trunc.bool(), term)
    with pytest.raises(ValueError, match="out"):
        fused_value_masked(agent, states, trunc, term, out=torch.zeros(B + 1, device=DEV))
    bad = PPOAgent(62, 2, hidden_dim=H, device=DEV, backend="hip")  # S % 4 != 0
    with pytest.raises(ValueError, match="backend='hip'"):
        bad.value_masked(torch.randn(B, 62, device=DEV), trunc, term)


def test_captured_in_a_graph():
    from utils.graphs import capture

    S, H = 60, 256
    agent, flat, image, tp, states, act_value, ref64 = _setup(S, H, True, B)
    trunc, term, marked = _mask("random", B)
    out = torch.full((B,), float("nan"), device=DEV)
    a = PpoActArgs()
    a.dims = PpoDims(B, S, H, 2)
    a.states, a.params, a.tiles, a.value = (states.data_ptr(), flat.data_ptr(), tp,
                                            out.data_ptr())
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with capture(g, stream=s):
            assert _bind(lib()).hwy_ppo_value_masked(ctypes.byref(a), trunc.data_ptr(), None,
                                                     stream_ptr()) == 0
    torch.cuda.current_stream().wait_stream(s)
    for _ in range(2):
        out.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        _check(out, marked, act_value, ref64)
