"""The fused HIP PPO minibatch step (csrc/ppo_kernels.hip) against torch autograd + torch Adam
running the reference's per-minibatch math (ppo/agent.py:216-252), fp32 tolerance."""

import ctypes

import numpy as np
import pytest
import torch

from hwy.ppo_native import FusedPPO
from ppo_ref_util import (_agents, _check_grads, _data, _fused_relu_masks, _gamma,  # noqa: F401
                          _grad64, _MaskMul, _torch_grad)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


@pytest.mark.parametrize("S,H,mb", [(60, 256, 4096), (60, 64, 256), (120, 512, 256), (136, 128, 128),
                                    (60, 192, 200), (30, 128, 256),  # split-K path (S % 4)
                                    # configs[4]'s learner shapes: N=30 rows of F_out 4 (none /
                                    # RoPE) or 8 (RankPE / DistPE, d 4), hidden 256 / 384 / 512
                                    (120, 384, 4096), (240, 256, 4096), (240, 512, 4096),
                                    # 32-row ppo_rows workgroups (rows >= 8192, H <= 256): the
                                    # bench minibatch, S = 240, ragged last workgroups (8 / 16 rows)
                                    (60, 256, 16384), (240, 256, 8192), (136, 192, 8200),
                                    (60, 64, 8208),
                                    # 16-row tiles at H > 256
                                    (60, 384, 8192), (60, 512, 8192),
                                    # configs[4]'s own minibatch (32,768 envs x T 32 / 32):
                                    # the balanced ppo_wgrad partition at 32,768 rows (H 256:
                                    # 26-32 tiles x 8 slices + extras; H 384: 60 tiles x 4
                                    # slices; H 512: 104 tiles x 2 slices)
                                    (120, 256, 32768), (120, 384, 32768), (120, 512, 32768),
                                    (240, 256, 32768), (240, 384, 32768), (240, 512, 32768),
                                    # 32-row ppo_rows workgroups (4 or 8 waves) at the narrower
                                    # learners, H 64 / 128 / 192, with the balanced wgrad split
                                    (60, 64, 16384), (60, 128, 16384), (136, 192, 16384),
                                    # 64-row ppo_rows_c64 tiles with a ragged last workgroup
                                    # (16 rows), and its 12-block states width (S 180)
                                    (60, 256, 16400), (180, 256, 16400)])
def test_fused_gradient_matches_autograd(S, H, mb):
    """One fused forward/backward against autograd on the same minibatch.  The reference
    gradient is float64 autograd: at S = 240 / H = 512 and 4096 rows torch's own fp32 GEMMs
    are off by up to 1.7e-6 on near-cancelling sums (tools/probe_grad_f64.py, where the
    fused kernel stays within 7e-10), so fp32 torch is no longer the tighter reference; at
    other shapes both fp32 results share the same rounding of the loss head and agree with
    each other better than with float64.  The fused gradient must agree elementwise with one
    of the two and never be further from float64 than torch fp32 is, up to rounding.

    A pre-activation within fp32 rounding of zero can take either ReLU decision in any fp32
    implementation, and one flipped element moves a whole weight-gradient row by its upstream
    gradient (at (60, 512, 8192) one of 8.4 M critic pre-activations moves row 396 of dWc1 by
    3.8e-7 while torch fp32 happens not to flip it).  So the float64 reference takes the fused
    step's own ReLU decisions, each checked to differ from float64's only at such
    rounding-level pre-activations (_fused_relu_masks)."""
    a, b = _agents(S, H)
    n = mb * 2
    s, z, lp, adv, ret, perm = _data(n, S, a)
    idx = perm[:mb].contiguous()
    g_ref, m_ref = _torch_grad(a, s, z, lp, adv, ret, idx)
    F = FusedPPO(b, mb, 2, use_graphs=False)
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
    m = F.metrics[0]
    # policy, value, entropy, loss, clip count, kl
    torch.testing.assert_close(m, m_ref, rtol=1e-4, atol=1e-6)


@pytest.mark.parametrize("graphs", [False, True])
def test_fused_update_matches_torch_update(graphs):
    S, H, n, nmb = 60, 256, 2048, 4
    a, b = _agents(S, H, graphs=graphs, epochs=3)
    s, z, lp, adv, ret, perm = _data(n, S, a)
    mb = n // nmb
    rows_a = a._run_epochs(s, z, lp, adv, ret, [perm[i * mb:(i + 1) * mb] for i in range(nmb)])
    F = FusedPPO(b, mb, nmb, use_graphs=graphs)
    rows_b = F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    torch.cuda.synchronize()
    steps = 3 * nmb
    for (k, va), (_, vb) in zip(a.actor_critic.state_dict().items(), b.actor_critic.state_dict().items()):
        # Adam normalises each element's step (~lr * sign(g) early on), so elements whose
        # gradient is at fp32 noise level may step differently: bound the worst case by the
        # largest possible move and require nearly all elements to agree closely.
        d = (va - vb).abs()
        assert d.max().item() <= 2 * 3e-4 * steps, k
        assert (d > 2e-5).float().mean().item() < 0.05, (k, d.max().item())
    torch.testing.assert_close(rows_b, rows_a, rtol=5e-3, atol=5e-5)
    assert int(F.counters[0]) == steps


@pytest.mark.parametrize("S,H,n,nmb,epochs", [(60, 256, 2048, 4, 3),
                                               # configs[4]'s learner at its own minibatch
                                               (120, 384, 65536, 2, 2)])
def test_fused_update_gradients_match_autograd_every_step(S, H, n, nmb, epochs):
    """Every minibatch step of a 3-epoch fused update (graph path) compared at the gradient
    level: before each step the torch model takes the fused weights, autograd computes the
    reference gradient (ppo/agent.py:216-248) on that step's minibatch, and the fused gradient
    must agree at the single-step tolerance (_check_grads, float64 autograd beside torch fp32).
    Weights never drift apart, so the bound stays as tight as the one-step test over the whole
    trajectory (Adam's own arithmetic is pinned separately by
    test_fused_optimizer_matches_torch_adam_on_identical_grads)."""
    a, b = _agents(S, H, epochs=epochs)
    s, z, lp, adv, ret, perm = _data(n, S, a)
    mb = n // nmb
    F = FusedPPO(b, mb, nmb, use_graphs=False)
    idxs = [perm[i * mb:(i + 1) * mb].contiguous() for i in range(nmb)]
    args = [F._args(s, z, lp, adv, ret, ix.data_ptr()) for ix in idxs]
    F.counters.zero_()
    F.sync_params(args[0])
    pa = dict(a.actor_critic.named_parameters())
    pb = dict(b.actor_critic.named_parameters())
    worst = 0.0
    for step in range(epochs * nmb):
        i = step % nmb
        with torch.no_grad():
            for name in pa:
                pa[name].copy_(pb[name])
        g_ref, m_ref = _torch_grad(a, s, z, lp, adv, ret, idxs[i])
        F._fwd_bwd(args[i])
        torch.cuda.synchronize()
        masks, _ = _fused_relu_masks(F, a, s, idxs[i], mb, H)
        g64 = _grad64(a, s, z, lp, adv, ret, idxs[i], masks)
        worst = max(worst, _check_grads(pa, pb, g64, msg=f"step {step}"))
        torch.testing.assert_close(F.metrics[step], m_ref, rtol=1e-4, atol=1e-6)
        F._opt(args[i])
    assert int(F.counters[0]) == epochs * nmb
    assert worst < 1e-3, worst


@pytest.mark.parametrize("graphs", [False, True])
def test_fused_update_replays_reference_golden(graphs):
    """The reference's own update (tests/golden/ppo_agent.npz 'upd_a': n 256, h64, 2 epochs,
    batch_size 64, generated from ppo/agent.py:196-308) replayed through the PRODUCT path:
    PPOAgent.update_rollout -> hwy_gae -> FusedPPO (the HIP minibatch kernels, HIP graphs when
    graphs=True) with the golden minibatch permutation.  Final weights and metrics match the
    golden at the torch path's tolerance."""
    from agent_util import load
    from ppo.agent import PPOAgent, RolloutBuffer

    g, meta = load()
    name = "upd_a"
    m = meta["agent"][name]
    n, S = m["n"], m["state_dim"]
    agent = PPOAgent(S, 2, lr=m["lr"], epochs=m["epochs"], batch_size=m["batch_size"],
                     hidden_dim=m["hidden_dim"], device=DEV, use_graphs=graphs, backend="hip")
    sd = {k[len(name) + 6:]: torch.as_tensor(g[k]) for k in g.files if k.startswith(f"{name}_init_")}
    agent.actor_critic.load_state_dict(sd)
    buf = RolloutBuffer(n, 1, S, 2, DEV)
    f = lambda k: torch.as_tensor(np.asarray(g[f"{name}_{k}"], np.float32), device=DEV)  # noqa: E731
    buf.states[:n].copy_(f("states").view(n, 1, S))
    buf.actions.copy_(f("actions").view(n, 1, 2))
    buf.pre_tanh.copy_(f("pre_tanh").view(n, 1, 2))
    buf.log_probs.copy_(f("log_probs").view(n, 1))
    buf.values.copy_(f("values").view(n, 1))
    buf.rewards.copy_(f("rewards").view(n, 1))
    buf.dones.copy_(torch.as_tensor(np.asarray(g[f"{name}_dones"], np.uint8), device=DEV).view(n, 1))
    perm = torch.as_tensor(np.asarray(g[f"{name}_perm"], np.int64), device=DEV)
    last = torch.tensor([m["last_value"]], dtype=torch.float32, device=DEV)
    metrics = agent.update_rollout(buf, last, perm=perm)
    assert agent._fused is not None and agent._fused.mb == 64 and agent._fused.nmb == n // 64
    for k, v in agent.actor_critic.state_dict().items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), g[f"{name}_final_{k}"], atol=5e-5,
                                   rtol=5e-5, err_msg=k)
    for k, want in m["metrics"].items():
        assert abs(metrics[k] - want) <= 1e-4 * max(1.0, abs(want)), (k, metrics[k], want)


def _replay_bench_golden(name, backend, graphs):
    """The reference's golden update `name` (tests/golden/ppo_agent_bench.npz) through
    PPOAgent.update_rollout on the GPU: (agent, metrics, arrays, meta)."""
    from agent_util import load
    from ppo.agent import PPOAgent, RolloutBuffer

    g, meta = load(bench=True)
    m = meta["agent"][name]
    n, S = m["n"], m["state_dim"]
    agent = PPOAgent(S, 2, lr=m["lr"], epochs=m["epochs"], batch_size=m["batch_size"],
                     hidden_dim=m["hidden_dim"], device=DEV, use_graphs=graphs, backend=backend)
    sd = {k[len(name) + 6:]: torch.as_tensor(g[k]) for k in g.files if k.startswith(f"{name}_init_")}
    agent.actor_critic.load_state_dict(sd)
    buf = RolloutBuffer(n, 1, S, 2, DEV)
    f = lambda k: torch.as_tensor(np.asarray(g[f"{name}_{k}"], np.float32), device=DEV)  # noqa: E731
    buf.states[:n].copy_(f("states").view(n, 1, S))
    buf.actions.copy_(f("actions").view(n, 1, 2))
    buf.pre_tanh.copy_(f("pre_tanh").view(n, 1, 2))
    buf.log_probs.copy_(f("log_probs").view(n, 1))
    buf.values.copy_(f("values").view(n, 1))
    buf.rewards.copy_(f("rewards").view(n, 1))
    buf.dones.copy_(torch.as_tensor(np.asarray(g[f"{name}_dones"], np.uint8), device=DEV).view(n, 1))
    perm = torch.as_tensor(np.asarray(g[f"{name}_perm"], np.int64), device=DEV)
    last = torch.tensor([m["last_value"]], dtype=torch.float32, device=DEV)
    metrics = agent.update_rollout(buf, last, perm=perm)
    return agent, metrics, g, m


def _rel_err(agent, g, name):
    """Per parameter: ||W - W_ref|| / ||W_ref|| against the golden final weights."""
    out = {}
    for k, v in agent.actor_critic.state_dict().items():
        want = np.asarray(g[f"{name}_final_{k}"], np.float64)
        d = v.detach().cpu().numpy().astype(np.float64) - want
        out[k] = float(np.linalg.norm(d) / max(np.linalg.norm(want), 1e-30))
    return out


_TORCH_GPU_DRIFT = {}


@pytest.mark.parametrize("name,graphs", [("upd_c1", False), ("upd_c1", True), ("upd_c2", True),
                                         ("upd_c4", True)])
def test_fused_update_replays_reference_golden_bench(name, graphs):
    """The reference's own update at the benched learners (generated by
    tests/golden/make_golden.py bench from ppo/agent.py:196-308): 2,048 samples, 8 epochs x 32
    minibatches of 64 = 256 Adam steps, at sd 60 / h256 (configs[1]'s cell), sd 120 / h256
    (configs[2]) and sd 120 / h512 (configs[4]), replayed through the PRODUCT path
    (update_rollout -> hwy_gae -> FusedPPO's HIP kernels, HIP graphs when graphs=True).

    Over 256 Adam steps any fp32 implementation drifts from the reference's CPU run: Adam
    normalises each element's step, so rounding-level gradient differences move near-zero
    elements by up to lr per step, and a clip decision that flips on one sample changes that
    sample's gradient outright.  On the CPU this build's torch learner replays the golden bit for
    bit (test_agent_golden.py); PyTorch's own fp32 GPU learner (backend='torch': the reference's
    algorithm on hipBLASLt GEMMs) drifts like the fused path (relative weight error up to 1e-2
    at h512, tools/probe_golden_bench.py).  So the bound is relative to that drift, measured in
    the same test: per parameter the fused path's relative error is at most 3x PyTorch-GPU's plus
    2e-3, the whole model's at most 3x plus 1e-3 and below 5e-2, and every metric within 3x
    PyTorch-GPU's deviation plus 1e-4 relative (clip fraction: 3x plus 2 / 2,048 samples)."""
    if name not in _TORCH_GPU_DRIFT:
        ta, tm, g, m = _replay_bench_golden(name, "torch", False)
        assert getattr(ta, "_fused", None) is None
        _TORCH_GPU_DRIFT[name] = (_rel_err(ta, g, name),
                                  {k: abs(tm[k] - w) for k, w in m["metrics"].items()})
    t_err, t_met = _TORCH_GPU_DRIFT[name]
    agent, metrics, g, m = _replay_bench_golden(name, "hip", graphs)
    F = agent._fused
    assert F is not None and F.mb == 64 and F.nmb == m["n"] // 64
    assert int(F.counters[0]) == m["epochs"] * (m["n"] // 64)
    f_err = _rel_err(agent, g, name)
    for k, e in f_err.items():
        assert e <= 3 * t_err[k] + 2e-3, (k, e, t_err[k])
    tot_f = float(np.sqrt(np.mean(np.square(list(f_err.values())))))
    tot_t = float(np.sqrt(np.mean(np.square(list(t_err.values())))))
    assert tot_f <= 3 * tot_t + 1e-3 and tot_f < 5e-2, (tot_f, tot_t)
    for k, want in m["metrics"].items():
        slack = 2.0 / m["n"] if k == "clip_fraction" else 1e-4 * max(1.0, abs(want))
        assert abs(metrics[k] - want) <= 3 * t_met[k] + slack, (k, metrics[k], want, t_met[k])


def test_ragged_update_rollout_replays_reference_golden():
    """'upd_b' (n 130, batch_size 50: minibatches 50 / 50 / 30) through update_rollout: the
    reference's get_batches partition with its short last minibatch is kept (no sample is
    dropped) and the result matches the golden."""
    from agent_util import load
    from ppo.agent import PPOAgent, RolloutBuffer

    g, meta = load()
    name = "upd_b"
    m = meta["agent"][name]
    n, S = m["n"], m["state_dim"]
    agent = PPOAgent(S, 2, lr=m["lr"], epochs=m["epochs"], batch_size=m["batch_size"],
                     hidden_dim=m["hidden_dim"], device=DEV, use_graphs=False)
    assert agent.minibatch_sizes(n) == [50, 50, 30]
    sd = {k[len(name) + 6:]: torch.as_tensor(g[k]) for k in g.files if k.startswith(f"{name}_init_")}
    agent.actor_critic.load_state_dict(sd)
    buf = RolloutBuffer(n, 1, S, 2, DEV)
    f = lambda k: torch.as_tensor(np.asarray(g[f"{name}_{k}"], np.float32), device=DEV)  # noqa: E731
    buf.states[:n].copy_(f("states").view(n, 1, S))
    buf.pre_tanh.copy_(f("pre_tanh").view(n, 1, 2))
    buf.log_probs.copy_(f("log_probs").view(n, 1))
    buf.values.copy_(f("values").view(n, 1))
    buf.rewards.copy_(f("rewards").view(n, 1))
    buf.dones.copy_(torch.as_tensor(np.asarray(g[f"{name}_dones"], np.uint8), device=DEV).view(n, 1))
    perm = torch.as_tensor(np.asarray(g[f"{name}_perm"], np.int64), device=DEV)
    last = torch.tensor([m["last_value"]], dtype=torch.float32, device=DEV)
    metrics = agent.update_rollout(buf, last, perm=perm)
    for k, v in agent.actor_critic.state_dict().items():
        np.testing.assert_allclose(v.detach().cpu().numpy(), g[f"{name}_final_{k}"], atol=5e-5,
                                   rtol=5e-5, err_msg=k)
    for k, want in m["metrics"].items():
        assert abs(metrics[k] - want) <= 1e-4 * max(1.0, abs(want)), (k, metrics[k], want)


def test_fused_rebuild_carries_adam_state():
    """Changing the minibatch geometry rebuilds FusedPPO; Adam's moments and step count carry
    over: a rebuilt instance continues exactly where the old one stopped."""
    S, H = 60, 64
    a, b = _agents(S, H)
    s, z, lp, adv, ret, perm = _data(512, S, a)
    b.num_minibatches = 4
    F1 = b._fused_for(128, 4, 512)
    F1.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    m1, v1, t1 = F1.m.clone(), F1.v.clone(), int(F1.counters[0])
    F2 = b._fused_for(256, 2, 512)
    assert F2 is not F1
    torch.cuda.synchronize()
    assert int(F2.counters[0]) == t1 == 8
    assert torch.equal(F2.m, m1) and torch.equal(F2.v, v1)


def test_fused_graph_recaptures_on_hyperparameter_change():
    """The epoch graph bakes lr / eps_clip / coefficients into its kernel arguments: changing
    them between updates recaptures, so the graph path equals the eager path after the change."""
    S, H, n, nmb = 60, 64, 512, 4
    outs = []
    for graphs in (False, True):
        a, b = _agents(S, H, graphs=graphs)
        s, z, lp, adv, ret, perm = _data(n, S, a)
        F = FusedPPO(b, n // nmb, nmb, use_graphs=graphs)
        F.run(s, z, lp, adv, ret, perm)
        for grp in b.optimizer.param_groups:
            grp["lr"] = 1e-3
        b.eps_clip, b.entropy_coef = 0.1, 0.02
        F.run(s, z, lp, adv, ret, perm)
        torch.cuda.synchronize()
        outs.append(F.flat.clone())
    assert torch.equal(outs[0], outs[1])


def test_fused_optimizer_matches_torch_adam_on_identical_grads():
    """clip_grad_norm_(0.5) + torch.optim.Adam vs the fused optimizer kernel, same gradients."""
    S, H = 60, 128
    a, b = _agents(S, H)
    F = FusedPPO(b, 128, 1, use_graphs=False)
    pa = dict(a.actor_critic.named_parameters())
    pb = dict(b.actor_critic.named_parameters())
    opt = torch.optim.Adam(a.actor_critic.parameters(), lr=3e-4)  # default (non-capturable) path
    g = torch.Generator(device=DEV).manual_seed(5)
    args = F._args(*([torch.zeros(1, device=DEV)] * 5), 0)
    args.grads_modified = 1
    for t in range(1, 6):
        scale = 0.2 if t % 2 else 3.0  # alternate un-clipped / clipped steps
        for name, p in pa.items():
            gr = torch.randn(p.shape, device=DEV, generator=g) * scale
            p.grad = gr.clone()
            pb[name].grad.copy_(gr)
        torch.nn.utils.clip_grad_norm_(a.actor_critic.parameters(), 0.5)
        opt.step()
        F.counters[0] = t
        F._opt(args)
        torch.cuda.synchronize()
        for name in pa:
            torch.testing.assert_close(pb[name], pa[name], rtol=1e-5, atol=1e-7, msg=name)
    # the weight tile image the row kernel reads was rewritten by every Adam step: a step from it
    # equals a step from a freshly rebuilt image, bit for bit
    s, z, lp, adv, ret, perm = _data(256, S, a)
    idx = perm[:128].contiguous()
    fa = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F._fwd_bwd(fa)
    g_adam = F.grads.clone()
    F.sync_params(fa)
    F._fwd_bwd(fa)
    torch.cuda.synchronize()
    assert torch.equal(F.grads, g_adam)


def _tile_image_floats(S, H):
    """TileGeom.total (csrc/ppo_kernels.hip tile_geom / rows_blocks): W1's forward image and six
    H x H images, in 1-KB blocks, K zero-padded to whole ring groups."""
    qh = H // 64
    nw = 8 if qh % 2 == 0 else 4
    d = 4 if H // nw // 16 <= 4 else 2
    hb = -(-(H // 16) // d) * d
    sb = -(-(-(-S // 16)) // d) * d
    g = H // 16
    return g * sb * 256 + 6 * g * hb * 256


@pytest.mark.parametrize("S,H", [(60, 256), (200, 320), (136, 512), (120, 192), (60, 64)])
def test_adam_rewrites_tile_image_as_a_rebuild(S, H):
    """ppo_adam_tiles rewrites the weight tile image block by block (forward blocks lane-linear,
    backward blocks through an LDS transpose, W1 blocks wholly past S left alone): after the
    update's Adam steps the image equals hwy_ppo_sync_params' rebuild from the new params, bit
    for bit, zero padding included.  (200, 320): a two-deep ring, so W1's 13 live blocks sit in
    a 14-block image while the Adam workgroup spans 16."""
    a, b = _agents(S, H)
    n, nmb = 512, 2
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


def test_fused_state_roundtrip_to_torch_optimizer(tmp_path):
    S, H = 60, 64
    a, b = _agents(S, H)
    s, z, lp, adv, ret, perm = _data(512, S, a)
    F = FusedPPO(b, 128, 4, use_graphs=False)
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    b._fused = F
    p = str(tmp_path / "ck.pth")
    b.save(p)
    ck = torch.load(p, weights_only=True)
    assert set(ck) == {"model", "optimizer"}
    st = ck["optimizer"]["state"]
    assert len(st) == 13 and float(st[0]["step"]) == 2 * 4
    # a fresh torch agent can resume from it
    from ppo.agent import PPOAgent

    c = PPOAgent(S, 2, hidden_dim=H, device=DEV, backend="torch")
    c.load(p)
    for (k, v1), (_, v2) in zip(b.actor_critic.state_dict().items(), c.actor_critic.state_dict().items()):
        assert torch.equal(v1, v2), k


@pytest.mark.parametrize("S,H,B", [(60, 256, 4096), (60, 64, 100), (120, 512, 333), (136, 192, 64)])
def test_fused_act_matches_actor_critic_act(S, H, B):
    """hwy_ppo_act vs ActorCritic.act (ppo/agent.py:86-95) with the same generator draws."""
    from hwy.ppo_native import fused_act

    a, b = _agents(S, H)
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
    # select_action on the batched path goes through the kernel
    b.generator = torch.Generator(device=DEV).manual_seed(3)
    out = b.select_action(s)
    assert out[0].shape == (B, 2) and bool(torch.all(out[0].abs() <= 1))


@pytest.mark.parametrize("S,H", [(60, 256), (120, 192)])
def test_fused_act_from_tile_image_equals_params_path(S, H):
    """After a fused update the acting kernel streams the update's weight tile image
    (hwy_ppo_tile_image_offset).  A torch-side parameter write (load_state_dict) retires the
    image; acting then rebuilds it from the params (hwy_ppo_sync_params), so the same weights act
    to the same bits on either side of a checkpoint reload -- at H = 256 always through
    ppo_act_c, whose head is the minibatch step's -- and a fresh agent holding those
    weights acts to the same bits too."""
    from hwy.ppo_native import fused_act

    a, b = _agents(S, H)
    n, nmb = 1024, 4
    s, z, lp, adv, ret, perm = _data(n, S, a)
    F = FusedPPO(b, n // nmb, nmb, use_graphs=False)
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())
    assert b._fused is F  # run() registers the instance that took the Adam state over
    flat = F.flat
    assert F.current_tiles(flat) is not None
    x = torch.randn(777, S, device=DEV)
    with torch.no_grad():
        got_t = fused_act(b, x, generator=torch.Generator(device=DEV).manual_seed(5))
        F._tiles_version = None  # retired image (at H = 256 rebuilt from the params by the act)
        got_p = fused_act(b, x, generator=torch.Generator(device=DEV).manual_seed(5))
    # H = 256 acts through ppo_act_c from a rebuilt image; other widths read the params rows with
    # the same kernel as the tile-image path
    assert (F.current_tiles(flat) is not None) == (H == 256)
    for t_, p_ in zip(got_t, got_p):
        assert torch.equal(t_, p_)
    # checkpoint round trip: load_state_dict retires the image, acting is bit-identical after it
    sd = {k: v.clone() for k, v in b.actor_critic.state_dict().items()}
    b.actor_critic.load_state_dict(sd)
    assert F.current_tiles(flat) is None
    with torch.no_grad():
        got_l = fused_act(b, x, generator=torch.Generator(device=DEV).manual_seed(5))
    for t_, l_ in zip(got_t, got_l):
        assert torch.equal(t_, l_)
    # a fresh agent (no FusedPPO yet) with the same weights: same kernel, same bits
    c, _ = _agents(S, H)
    c.actor_critic.load_state_dict(sd)
    with torch.no_grad():
        got_c = fused_act(c, x, generator=torch.Generator(device=DEV).manual_seed(5))
        ref = c.actor_critic.act(x, deterministic=True)
        det = fused_act(c, x, deterministic=True)
    for t_, c_ in zip(got_t, got_c):
        assert torch.equal(t_, c_)
    for r, g in zip(ref, det):
        torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)


@pytest.mark.parametrize("S,B", [(60, 16384), (120, 20000), (60, 4096), (120, 1000)])
def test_compact_act_kernel(S, B):
    """ppo_act_c (H 256, tile image in step; 32-row tiles from two per CU, else 16): against
    ActorCritic.act with the same draws and against ppo_act on the params path; and its head is
    the minibatch step's, so re-evaluating the acted rows in a fused step gives a ratio of
    exactly 1 on every row (KL and clip count exactly 0)."""
    from hwy.ppo_native import fused_act

    H, n = 256, min(B, 16384)
    a, b = _agents(S, H)
    s, z, lp, adv, ret, perm = _data(n, S, a)
    F = FusedPPO(b, n, 1, use_graphs=False)
    b._fused = F
    F.run(s, z, lp, adv.clone(), ret.clone(), perm.clone())  # the tile image follows params now
    assert F.current_tiles(F.flat) is not None
    a.actor_critic.load_state_dict(b.actor_critic.state_dict())
    x = torch.randn(B, S, device=DEV)
    gen = lambda: torch.Generator(device=DEV).manual_seed(7)  # noqa: E731
    with torch.no_grad():
        ref = a.actor_critic.act(x, generator=gen())
        got = fused_act(b, x, generator=gen())
        saved = F._tiles_version
        F._tiles_version = None  # the 16-row kernel from the flat params
        got_p = fused_act(b, x, generator=gen())
        F._tiles_version = saved
        got_d = fused_act(b, x, deterministic=True)
        ref_d = a.actor_critic.act(x, deterministic=True)
    for r, g, p_ in zip(ref, got, got_p):
        torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)
        torch.testing.assert_close(g, p_, rtol=1e-4, atol=2e-5)
    for r, g in zip(ref_d, got_d):
        torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)
    if B == n:
        _, pre, logp, _ = got
        idx = torch.arange(n, device=DEV, dtype=torch.int64)
        args = F._args(x, pre.contiguous(), logp.contiguous(), adv, ret, idx.data_ptr())
        F.counters.zero_()
        F._fwd_bwd(args)
        torch.cuda.synchronize()
        m = F.metrics[0]
        assert m[4].item() == 0.0 and m[5].item() == 0.0, m.tolist()


def test_rollout_noise_value_and_dones_helpers():
    """Pre-drawn rollout noise (RolloutBuffer.draw_noise, one draw per rollout) gives the same
    sample through the kernel and ActorCritic.act; agent.value is the critic's V(s);
    finish_dones = terminated | truncated."""
    from ppo.agent import RolloutBuffer

    S, H, T, E = 60, 256, 3, 300
    a, b = _agents(S, H)
    buf = RolloutBuffer(T, E, S, 2, DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    buf.draw_noise(g)
    g2 = torch.Generator(device=DEV).manual_seed(11)
    assert torch.equal(buf.noise, torch.randn(T, E, 2, generator=g2, device=DEV))
    s = torch.randn(E, S, device=DEV)
    with torch.no_grad():
        ref = a.actor_critic.act(s, noise=buf.noise[1])
        got = b.select_action(s, noise=buf.noise[1])
        for r, x in zip(ref, got):
            torch.testing.assert_close(x, r, rtol=1e-4, atol=2e-5)
        torch.testing.assert_close(b.value(s), a.actor_critic.forward(s)[2].squeeze(-1),
                                   rtol=1e-4, atol=2e-5)
    with pytest.raises(ValueError):
        b.select_action(s, noise=buf.noise[1][:, :1])
    buf.terminated.copy_(torch.randint(0, 2, (T, E), device=DEV, dtype=torch.uint8))
    buf.truncated.copy_(torch.randint(0, 2, (T, E), device=DEV, dtype=torch.uint8))
    buf.finish_dones()
    assert torch.equal(buf.dones, buf.terminated | buf.truncated)


def test_adam_state_hands_over_between_fused_and_eager_updates():
    """an update whose minibatches come out unequal runs the eager torch path; the
    Adam moments and step count pass from FusedPPO to agent.optimizer before it and back after
    it.  A fused / eager / fused sequence lands where three eager torch updates land (fp32
    tolerance); a lost hand-over restarts Adam's bias correction and moves every weight by
    ~lr."""
    from ppo.agent import RolloutBuffer

    S, H, T, E = 60, 64, 16, 32
    a, b = _agents(S, H, epochs=2)
    g = torch.Generator(device=DEV).manual_seed(3)
    buf = RolloutBuffer(T, E, S, 2, DEV)
    buf.states.copy_(torch.randn(buf.states.shape, device=DEV, generator=g))
    with torch.no_grad():
        _, zz, lp, v = a.actor_critic.act(buf.states[:T].reshape(T * E, S), generator=g)
    buf.pre_tanh.copy_(zz.view(T, E, 2))
    buf.log_probs.copy_((lp + 0.05 * torch.randn(lp.shape, device=DEV, generator=g)).view(T, E))
    buf.values.copy_(v.view(T, E))
    buf.rewards.copy_(torch.randn(T, E, device=DEV, generator=g))
    buf.dones.copy_((torch.rand(T, E, device=DEV, generator=g) < 0.05).to(torch.uint8))
    last = torch.randn(E, device=DEV, generator=g)
    n = T * E
    for nmb in (4, 3, 4):  # 512 rows: 4 x 128 (fused), 171/171/170 (eager), 4 x 128 (fused)
        perm = torch.randperm(n, device=DEV, generator=g)
        for ag in (a, b):
            ag.num_minibatches = nmb
            ag.update_rollout(buf, last, perm=perm.clone())
    torch.cuda.synchronize()
    assert b._fused is not None and b._adam_owner == "fused"
    assert int(b._fused.counters[0]) == 2 * (4 + 3 + 4)
    for (k, va), (_, vb) in zip(a.actor_critic.state_dict().items(), b.actor_critic.state_dict().items()):
        d = (va - vb).abs()
        assert (d > 2e-5).float().mean().item() < 0.05, (k, d.max().item())


def test_act_after_graph_replayed_reference_updates():
    """the reference path's update() replays a captured torch learner, which writes the
    parameters in place without bumping their version counters.  Batched acting at H = 256 runs
    ppo_act_c from a cached weight tile image, so that image must be retired by every such update
    (agent._torch_param_writes) or acting would use the previous update's weights."""
    from hwy.ppo_native import fused_act
    from ppo.agent import PPOAgent

    S, H = 60, 256
    torch.manual_seed(3)
    ag = PPOAgent(S, 2, lr=1e-3, epochs=2, batch_size=64, hidden_dim=H, device=DEV,
                  use_graphs=True, backend="hip")
    x = torch.randn(512, S, device=DEV)
    with torch.no_grad():
        fused_act(ag, x, deterministic=True)  # builds the acting-only tile image
    rng = np.random.default_rng(0)
    for _ in range(3):
        before = [p.detach().clone() for p in ag.actor_critic.parameters()]
        for i in range(256):
            s = rng.standard_normal(S).astype(np.float32)
            a, z, lp, v = ag.select_action(s)
            ag.memory.store(s, a, z, float(rng.standard_normal()), s, lp, i % 50 == 49, v)
        ag.update(0.0)
        moved = max(float((p.detach() - b).abs().max())
                    for p, b in zip(ag.actor_critic.parameters(), before))
        assert moved > 1e-4  # the update wrote the weights
        with torch.no_grad():
            ref = ag.actor_critic.act(x, deterministic=True)
            got = fused_act(ag, x, deterministic=True)
        for r, g in zip(ref, got):
            torch.testing.assert_close(g, r, rtol=1e-4, atol=2e-5)
