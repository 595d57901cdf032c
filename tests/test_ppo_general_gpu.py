"""The general path of hwy_ppo_forward_backward / hwy_ppo_optimizer (csrc/ppo_kernels.hip: 11
launches of gemm64 / gemm64v, ppo_head, split-K slabs, ppo_reduce, the flat ppo_adam) at state
widths outside the fused bound, S % 4 != 0 or S > 1,024, against float64 autograd; and the flat
ppo_adam with write_tiles on fused shapes whose buffers are not 16-byte aligned.  Every criterion
is one the fused path's tests apply (test_ppo_edges_gpu.py, test_ppo_fused_gpu.py), unchanged.
The cases (ppo_ref_util.GENERAL_CASES) are drawn on the CPU; test_ppo_general_inputs.py checks,
without a GPU, that they are well conditioned and which K loops each reaches.  Every test prints
its measured figures (pytest -s)."""

import ctypes

import pytest
import torch

from hwy.native import check, lib, stream_ptr
from hwy.ppo_native import FusedPPO, PpoArgs, PpoDims, _bind, param_layout
from ppo_ref_util import (GENERAL_CASES, GENERAL_EXACT_CASES, GENERAL_NORM_CASES, _agents,
                          _check_grads, _data, _fused_relu_masks, _grad64, _torch_grad, case_id,
                          case_kwargs, edge_case)
import test_ppo_edges_gpu as edges  # its tests are called below on the general cases

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _no_tile_image(S, H, B):
    """The shape takes the general path: the library keeps no weight tile image for it
    (FusedPPO._tile_off is None is this call answering -1), for the tests below whose FusedPPO
    is built inside the edge test they call."""
    d = PpoDims(B, S, H, 2)
    return _bind(lib()).hwy_ppo_tile_image_offset(ctypes.byref(d)) == -1


# ------------------------------------------------------------------ gradient parity grid
@pytest.mark.parametrize("c", GENERAL_CASES, ids=case_id)
def test_general_gradient_matches_autograd(c):
    """One forward/backward per case against float64 autograd with the step's own ReLU decisions
    (each checked against float64 within the derived fp32 bound) and torch fp32, and the metrics
    row against torch fp32's (test_ppo_edges_gpu._parity)."""
    S, H, B = c[:3]
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, **case_kwargs(c))
    F = FusedPPO(b, B, 1, use_graphs=False)
    assert F._tile_off is None
    edges._fused_step(F, F._args(s, z, lp, adv, ret, idx.data_ptr()))
    worst = edges._parity(F, a, b, s, z, lp, adv, ret, idx)
    print(f"\nGENERAL grad {case_id(c)} error / gradient scale {worst:.3e}"
          f" clip count {int(F.metrics[0, 4])} of {B}")


# ------------------------------------------------------------------ exact checks, in-kernel norm
@pytest.mark.parametrize("c", GENERAL_EXACT_CASES, ids=case_id)
def test_general_zero_signal_gives_exactly_zero_gradients(c):
    """test_ppo_edges_gpu's zero-signal test on the general path: stale split-K slabs or bias
    partials of the ordinary step before it would show."""
    assert _no_tile_image(*c[:3])
    edges.test_zero_signal_gives_exactly_zero_gradients(c)


@pytest.mark.parametrize("c", GENERAL_EXACT_CASES, ids=case_id)
def test_general_dead_units_have_exactly_zero_gradients(c):
    """test_ppo_edges_gpu's dead-unit test on the general path (columns dead_columns(H))."""
    assert _no_tile_image(*c[:3])
    edges.test_dead_units_have_exactly_zero_gradients(c)


@pytest.mark.parametrize("mgn", [0.5, 100.0], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("c", GENERAL_NORM_CASES, ids=case_id)
def test_general_clip_coefficient_from_in_kernel_norm(c, mgn):
    """test_ppo_edges_gpu's criterion for the clip coefficient, here from ppo_reduce's norm
    partials (nred up to 5,287) and applied by the flat ppo_adam."""
    assert _no_tile_image(*c[:3])
    edges.test_clip_coefficient_from_in_kernel_norm(c, mgn)


# ------------------------------------------------------------------ multi-step update
def _start(S, H, n, epochs, graphs):
    a, b = _agents(S, H, graphs=graphs, epochs=epochs)
    return (a, b) + _data(n, S, a)


@pytest.mark.parametrize("S,H", [(75, 128), (1028, 64)], ids=lambda v: str(v))
def test_general_update_gradients_match_autograd_every_step(S, H):
    """test_ppo_fused_gpu.test_fused_update_gradients_match_autograd_every_step's scheme on the
    general path (n 512, 4 minibatches, 2 epochs): before each step the torch model takes the
    stepped weights, and that step's gradient meets _check_grads and its metrics row torch's."""
    n, nmb, epochs = 512, 4, 2
    a, b, s, z, lp, adv, ret, perm = _start(S, H, n, epochs, False)
    mb = n // nmb
    F = FusedPPO(b, mb, nmb, use_graphs=False)
    assert F._tile_off is None
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
        _, m_ref = _torch_grad(a, s, z, lp, adv, ret, idxs[i])
        F._fwd_bwd(args[i])
        torch.cuda.synchronize()
        masks, _ = _fused_relu_masks(F, a, s, idxs[i], mb, H)
        g64 = _grad64(a, s, z, lp, adv, ret, idxs[i], masks)
        worst = max(worst, _check_grads(pa, pb, g64, msg=f"step {step}"))
        torch.testing.assert_close(F.metrics[step], m_ref, rtol=1e-4, atol=1e-6)
        F._opt(args[i])
    torch.cuda.synchronize()
    assert int(F.counters[0]) == epochs * nmb
    print(f"\nGENERAL update {S}-{H} worst error / gradient scale over {epochs * nmb} steps"
          f" {worst:.3e}")
    assert worst < 1e-3, worst


@pytest.mark.parametrize("S,H", [(75, 128), (1028, 64)], ids=lambda v: str(v))
def test_general_update_graph_equals_eager(S, H):
    """FusedPPO.run on the general path, captured (the second run replays the epoch graph) and
    eager, from the same start: weights, Adam moments and metrics rows are bit-identical after
    each of two updates."""
    n, nmb, epochs = 512, 4, 2
    outs = []
    for graphs in (False, True):
        a, b, s, z, lp, adv, ret, perm = _start(S, H, n, epochs, graphs)
        F = FusedPPO(b, n // nmb, nmb, use_graphs=graphs)
        assert F._tile_off is None
        runs = []
        for _ in range(2):
            rows = F.run(s, z, lp, adv, ret, perm)
            torch.cuda.synchronize()
            runs.append([t.clone() for t in (F.flat, F.m, F.v, rows)])
        assert int(F.counters[0]) == 2 * epochs * nmb
        assert (F._graphs is not None) == graphs
        outs.append(runs)
    for eager, graph in zip(*outs):
        for name, te, tg in zip(("flat", "m", "v", "metrics"), eager, graph):
            assert torch.equal(te, tg), name
    assert not torch.equal(outs[0][0][0], outs[0][1][0])  # the second update moved the weights


# ------------------------------------------------------------------ the flat Adam kernel
def test_general_optimizer_matches_torch_adam_on_identical_grads():
    """test_ppo_fused_gpu.test_fused_optimizer_matches_torch_adam_on_identical_grads' scheme at
    S 75 / H 128: ppo_sumsq + the flat ppo_adam (59,653 elements, the last workgroup partial)
    against clip_grad_norm_(0.5) + torch.optim.Adam on the same gradients over five steps
    alternating unclipped / clipped."""
    S, H = 75, 128
    a, b = _agents(S, H)
    F = FusedPPO(b, 128, 1, use_graphs=False)
    assert F._tile_off is None and F.flat.numel() == 59653 and F.flat.numel() % 512 != 0
    pa = dict(a.actor_critic.named_parameters())
    pb = dict(b.actor_critic.named_parameters())
    opt = torch.optim.Adam(a.actor_critic.parameters(), lr=3e-4)
    g = torch.Generator(device=DEV).manual_seed(5)
    args = F._args(*([torch.zeros(1, device=DEV)] * 5), 0)
    args.grads_modified = 1
    for t in range(1, 6):
        # 59,653 standard normals have norm 244: 1e-3 of it stays below max_grad_norm, 3 x clips
        scale = 1e-3 if t % 2 else 3.0
        for name, p in pa.items():
            gr = torch.randn(p.shape, device=DEV, generator=g) * scale
            p.grad = gr.clone()
            pb[name].grad.copy_(gr)
        n = float(torch.nn.utils.clip_grad_norm_(a.actor_critic.parameters(), 0.5))
        assert (n > 0.5) == (t % 2 == 0), (t, n)
        opt.step()
        F.counters[0] = t
        F._opt(args)
        torch.cuda.synchronize()
        for name in pa:
            torch.testing.assert_close(pb[name], pa[name], rtol=1e-5, atol=1e-7, msg=name)


# ------------------------------------------------------------------ unaligned buffers, fused shapes
class _OptLearner:
    """Hand-built hwy_ppo_args for optimizer-only calls on a fused shape: params, grads and the
    Adam moments start `shift` floats into their allocations; the workspace is aligned."""

    def __init__(self, S, H, shift, flat0):
        self.L = _bind(lib())
        self.dims = PpoDims(64, S, H, 2)
        n = flat0.numel()
        self.bufs = [torch.zeros(n + 4, device=DEV) for _ in range(4)]  # keep the allocations
        self.flat, self.grads, self.m, self.v = (t[shift:shift + n] for t in self.bufs)
        self.flat.copy_(flat0)
        self.counters = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.metrics = torch.zeros(1, 6, device=DEV)
        ws = self.L.hwy_ppo_workspace_bytes(ctypes.byref(self.dims))
        self.off = int(self.L.hwy_ppo_tile_image_offset(ctypes.byref(self.dims)))
        assert ws > 0 and self.off >= 0  # a fused shape
        self.workspace = torch.zeros(int(ws), dtype=torch.uint8, device=DEV)
        assert self.workspace.data_ptr() % 256 == 0
        a = self.args = PpoArgs()
        a.dims = self.dims
        a.params, a.grads = self.flat.data_ptr(), self.grads.data_ptr()
        a.adam_m, a.adam_v = self.m.data_ptr(), self.v.data_ptr()
        a.counters, a.metrics = self.counters.data_ptr(), self.metrics.data_ptr()
        a.workspace = self.workspace.data_ptr()
        a.eps_clip, a.value_coef, a.entropy_coef, a.max_grad_norm = 0.2, 0.5, 0.005, 0.5
        a.lr, a.beta1, a.beta2, a.adam_eps = 3e-4, 0.9, 0.999, 1e-8
        a.grads_modified = 1  # ppo_sumsq + Adam: one float at a time on these buffers
        self.sync()

    def pointers(self):
        a = self.args
        return (a.params, a.grads, a.adam_m, a.adam_v)

    def sync(self):
        check(self.L.hwy_ppo_sync_params(ctypes.byref(self.args), stream_ptr()),
              "hwy_ppo_sync_params")

    def step(self, t, g):
        self.grads.copy_(g)
        self.counters[0] = t
        check(self.L.hwy_ppo_optimizer(ctypes.byref(self.args), stream_ptr()), "hwy_ppo_optimizer")

    def image(self):
        return self.workspace[self.off:]  # the image is the workspace's last sub-buffer


@pytest.mark.parametrize("S,H", [(60, 64), (200, 320), (136, 512)], ids=lambda v: str(v))
def test_unaligned_buffers_take_flat_adam_with_the_same_bits(S, H):
    """On a fused shape whose params / grads / m / v are not 16-byte aligned hwy_ppo_optimizer runs
    the flat ppo_adam, which rewrites the weight tile image element by element (write_tiles).
    Three optimizer-only steps (grads_modified = 1) of seeded gradients, unclipped and clipped:
    after each, (a) the image equals hwy_ppo_sync_params' rebuild from the new parameters on a
    second workspace, bit for bit and padding included, and (b) params, m and v equal those of the
    same steps on 16-byte-aligned buffers, which run ppo_adam_tiles, bit for bit."""
    _, numel = param_layout(S, H)
    g = torch.Generator(device=DEV).manual_seed(1000 * H + S)
    flat0 = torch.randn(numel, device=DEV, generator=g) * 0.05
    un, al = _OptLearner(S, H, 1, flat0), _OptLearner(S, H, 0, flat0)
    assert all(p % 16 == 4 for p in un.pointers()), [p % 16 for p in un.pointers()]
    # adam_tiles_ok: a fused shape, S % 4 == 0, all four bases 16-byte aligned
    assert S % 4 == 0 and all(p % 16 == 0 for p in al.pointers())
    assert torch.equal(un.image(), al.image()) and bool(un.image().view(torch.float32).any())
    for t in range(1, 4):
        # norm 0.1 (unclipped) on steps 1 and 3, 3 sqrt(numel) (clipped) on step 2
        grad = torch.randn(numel, device=DEV, generator=g) * (3.0 if t == 2 else 0.1 / numel ** 0.5)
        assert (float(grad.norm()) > 0.5) == (t == 2)
        before = un.flat.clone()
        un.step(t, grad)
        al.step(t, grad)
        torch.cuda.synchronize()
        assert not torch.equal(un.flat, before)
        rebuilt = _OptLearner(S, H, 0, un.flat)  # a second workspace, synced from the new params
        torch.cuda.synchronize()
        same = un.image().view(torch.int32) == rebuilt.image().view(torch.int32)
        assert bool(same.all()), (t, int((~same).sum()))
        assert torch.equal(al.image(), rebuilt.image()), t
        for name, tu, ta in (("params", un.flat, al.flat), ("m", un.m, al.m), ("v", un.v, al.v)):
            assert torch.equal(tu.view(torch.int32), ta.view(torch.int32)), (
                t, name, (tu.double() - ta.double()).abs().max().item())
    print(f"\nGENERAL unaligned {S}-{H}: image, params, m, v bit-identical over 3 steps")
