"""The fused PPO step and fused acting for state rows wider than 256 floats (S % 4 == 0,
S <= 1,024): the row and act kernels run their first layer over chunks of 256 state columns
(csrc/ppo_kernels.hip rows_forward, WIDE).  Same references and tolerances as the narrow shapes'
tests in test_ppo_fused_gpu.py; every test also asserts that the fused path -- the weight tile
image, hwy_ppo_act -- is what ran."""

import pytest
import torch

from hwy.ppo_native import FusedPPO
from ppo_ref_util import _agents, _check_grads, _data, _fused_relu_masks, _grad64, _torch_grad
from test_ppo_fused_gpu import _tile_image_floats

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("S,H,mb", [
    (260, 64, 48),       # one full chunk plus the smallest tail (4 columns of one padded block)
    (300, 256, 100),     # ragged last row tile (4 of 16 rows)
    (512, 128, 64),      # exact chunks
    (516, 192, 33),      # chunk boundary plus 4 columns, the 4-wave class
    (600, 384, 256),     # mid-range width at H = 384
    (1024, 512, 40),     # the limit, at the LDS-tightest H
    (1000, 256, 8200),   # past the narrow shapes' 32-row-tile threshold: still 16-row tiles,
                         # ragged last workgroup (8 rows), 63 state blocks
])
def test_wide_fused_gradient_matches_autograd(S, H, mb):
    """test_fused_gradient_matches_autograd's recipe at wide S: the float64 autograd reference
    takes the fused step's own ReLU decisions (each checked against float64 to rounding), the
    gradient criterion is _check_grads, the metrics row agrees at rtol 1e-4 / atol 1e-6."""
    a, b = _agents(S, H)
    n = mb * 2
    s, z, lp, adv, ret, perm = _data(n, S, a)
    idx = perm[:mb].contiguous()
    g_ref, m_ref = _torch_grad(a, s, z, lp, adv, ret, idx)
    F = FusedPPO(b, mb, 2, use_graphs=False)
    assert F._tile_off is not None  # the four-launch fused step, not the general path
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F.counters.zero_()
    F.sync_params(args)
    F._fwd_bwd(args)
    torch.cuda.synchronize()
    masks, _ = _fused_relu_masks(F, a, s, idx, mb, H)
    g64 = _grad64(a, s, z, lp, adv, ret, idx, masks)
    ga = dict(a.actor_critic.named_parameters())
    gb = dict(b.actor_critic.named_parameters())
    _check_grads(ga, gb, g64)
    torch.testing.assert_close(F.metrics[0], m_ref, rtol=1e-4, atol=1e-6)


def test_wide_step_writes_the_gathered_states_chunk_by_chunk():
    """RowArgs::xg (ppo_wgrad's dW1 operand, [B][S]) holds exactly the minibatch's state rows
    after a step: every chunk's columns, the 4-column tail included."""
    S, H, mb = 516, 192, 33
    a, b = _agents(S, H)
    s, z, lp, adv, ret, perm = _data(2 * mb, S, a)
    idx = perm[:mb].contiguous()
    F = FusedPPO(b, mb, 2, use_graphs=False)
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F.sync_params(args)
    F._fwd_bwd(args)
    torch.cuda.synchronize()
    # carve order (256-B aligned sub-buffers): ..., wg_slab, xg, tile image -- xg ends where the
    # tile image starts
    al = lambda k: (k + 63) // 64 * 64  # noqa: E731
    ws = F.workspace.view(torch.float32)
    end = F._tile_off // 4
    xg = ws[end - al(mb * S):end - al(mb * S) + mb * S].view(mb, S)
    assert torch.equal(xg, s[idx])


@pytest.mark.parametrize("graphs", [False, True])
@pytest.mark.parametrize("S,H", [(300, 256), (600, 128)])
def test_wide_fused_update_matches_torch_update(S, H, graphs):
    n, nmb = 512, 4
    a, b = _agents(S, H, graphs=graphs, epochs=3)
    s, z, lp, adv, ret, perm = _data(n, S, a)
    mb = n // nmb
    rows_a = a._run_epochs(s, z, lp, adv, ret, [perm[i * mb:(i + 1) * mb] for i in range(nmb)])
    F = FusedPPO(b, mb, nmb, use_graphs=graphs)
    assert F._tile_off is not None
    rows_b = F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    torch.cuda.synchronize()
    steps = 3 * nmb
    for (k, va), (_, vb) in zip(a.actor_critic.state_dict().items(),
                                b.actor_critic.state_dict().items()):
        # as test_fused_update_matches_torch_update: Adam normalises each element's step, so
        # bound the worst case by the largest possible move and ask nearly all to agree closely
        d = (va - vb).abs()
        assert d.max().item() <= 2 * 3e-4 * steps, k
        assert (d > 2e-5).float().mean().item() < 0.05, (k, d.max().item())
    torch.testing.assert_close(rows_b, rows_a, rtol=5e-3, atol=5e-5)
    assert int(F.counters[0]) == steps


@pytest.mark.parametrize("S,H", [(260, 64), (300, 256), (1024, 512)])
def test_wide_adam_rewrites_tile_image_as_a_rebuild(S, H):
    """After an update's Adam steps the weight tile image equals hwy_ppo_sync_params' rebuild
    from the new params bit for bit, W1's zero padding to whole k blocks included."""
    a, b = _agents(S, H)
    n, nmb = 128, 2
    s, z, lp, adv, ret, perm = _data(n, S, a)
    F = FusedPPO(b, n // nmb, nmb, use_graphs=False)
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    torch.cuda.synchronize()
    nb = _tile_image_floats(S, H) * 4
    assert F._tile_off is not None and F._tile_off + nb <= F.workspace.numel()
    img = F.workspace[F._tile_off:F._tile_off + nb].clone()
    F.sync_params(F._args(s, z, lp, adv, ret, perm.data_ptr()))
    torch.cuda.synchronize()
    assert torch.equal(F.workspace[F._tile_off:F._tile_off + nb], img)


@pytest.mark.parametrize("S,H,B", [(300, 256, 1), (300, 256, 333), (600, 384, 100),
                                   (1024, 512, 64)])
def test_wide_fused_act_matches_actor_critic_act(S, H, B):
    """hwy_ppo_act vs ActorCritic.act with the same generator draws, with noise and
    deterministic; at H = 256 the call streams a weight tile image (the compact kernel)."""
    from hwy.ppo_native import act_supported, act_tiles, fused_act, flat_params

    a, b = _agents(S, H)
    assert act_supported(S, H, 2) and b._act_fused_ok(torch.empty(1, S, device=DEV))
    s = torch.randn(B, S, device=DEV)
    g1 = torch.Generator(device=DEV).manual_seed(7)
    g2 = torch.Generator(device=DEV).manual_seed(7)
    with torch.no_grad():
        ref = a.actor_critic.act(s, generator=g1)
        got = fused_act(b, s, generator=g2)
        ref_d = a.actor_critic.act(s, deterministic=True)
        got_d = fused_act(b, s, deterministic=True)
    for r, g in zip(ref, got):
        torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)
    for r, g in zip(ref_d, got_d):
        torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)
    if H == 256:
        assert act_tiles(b, flat_params(b)[0], S, H) is not None
    # select_action on the batched path goes through the kernel
    b.generator = torch.Generator(device=DEV).manual_seed(3)
    out = b.select_action(s)
    assert out[0].shape == (B, 2) and bool(torch.all(out[0].abs() <= 1))


@pytest.mark.parametrize("S,H", [(300, 256), (516, 192)])
def test_wide_act_from_tile_image_equals_params_path(S, H):
    """After a fused update acting streams the update's tile image; with the image retired it
    reads the params rows (H = 256: a rebuilt image, the compact kernel either way).  The same
    weights act to the same bits on both paths, and the compact kernel's head is the minibatch
    step's: re-evaluating acted rows gives a ratio of exactly 1 on every row."""
    from hwy.ppo_native import fused_act

    a, b = _agents(S, H)
    n = 256
    s, z, lp, adv, ret, perm = _data(n, S, a)
    F = FusedPPO(b, n, 1, use_graphs=False)
    b._fused = F
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    assert F.current_tiles(F.flat) is not None
    x = torch.randn(n, S, device=DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(5)  # noqa: E731
    with torch.no_grad():
        got_t = fused_act(b, x, generator=gen())
        saved = F._tiles_version
        F._tiles_version = None
        got_p = fused_act(b, x, generator=gen())
        F._tiles_version = saved
    for t_, p_ in zip(got_t, got_p):
        assert torch.equal(t_, p_)
    if H == 256:
        _, pre, logp, _ = got_t
        idx = torch.arange(n, device=DEV, dtype=torch.int64)
        args = F._args(x, pre.contiguous(), logp.contiguous(), adv, ret, idx.data_ptr())
        F.counters.zero_()
        F._fwd_bwd(args)
        torch.cuda.synchronize()
        m = F.metrics[0]
        assert m[4].item() == 0.0 and m[5].item() == 0.0, m.tolist()


def test_backend_hip_refuses_states_past_the_bound():
    from ppo.agent import PPOAgent

    ag = PPOAgent(1028, 2, hidden_dim=64, device=DEV, backend="hip")
    with pytest.raises(ValueError, match="<= 1024"):
        ag.select_action(torch.zeros(4, 1028, device=DEV))
    auto = PPOAgent(1028, 2, hidden_dim=64, device=DEV, backend="auto")
    assert not auto._act_fused_ok(torch.zeros(4, 1028, device=DEV))
