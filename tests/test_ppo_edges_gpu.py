"""The solo fused PPO step and the acting kernels (csrc/ppo_kernels.hip, ppo_rows_body.inc)
against float64 autograd / the float64 model where the grouped and mixed-width tests only assert
bit equality with the solo call: hidden widths 320 and 448 (TW 5 / 7, the two-deep weight ring),
S and B edges, wide fused states (S 260 / 300: 256 < S <= 1,024), the general path's scalar GEMMs
at S 75 / 30 (test_ppo_general_gpu.py covers that path), inputs on which 20-80 % of the rows are
clipped, non-default log_std and coefficients, and the clip coefficient from the in-kernel
gradient norm.  The inputs
are drawn on the CPU (ppo_ref_util.edge_case); test_ppo_edge_inputs.py checks, without a GPU,
that they are well conditioned.  Every test prints its measured figures (pytest -s)."""

import ctypes

import pytest
import torch

from hwy.native import check, lib, stream_ptr
from hwy.ppo_native import (_PARAM_ORDER, FusedPPO, PpoActArgs, PpoArgs, PpoDims, _bind, act_tiles,
                            flat_params, fused_act)
from ppo_ref_util import (ACT_CASES, EXACT_CASES, GRAD_CASES, GRAD_GENERAL_SHAPES, NORM_CASES, U32,
                          _check_grads, _fused_relu_masks, _grad64, _torch_grad, act64, act_case,
                          case_id, case_kwargs, dead_columns, edge_case)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TINY = 2.0 ** -126  # smallest normal binary32


def _err_over(got, want, unit):
    """|got - want| / unit per element.  Only where 0 < |want| < TINY, below the normal range
    (gradual underflow and flush to zero are both fp32 there, neither has relative precision),
    an absolute error of TINY counts as none; where want is zero, got must be zero."""
    err = (got - want).abs()
    sub = want.abs() < TINY
    ok = err <= TINY * (want != 0)
    return torch.where(sub, torch.where(ok, 0.0, float("inf")), err / unit.clamp_min(TINY))


def _fused_step(F, args):
    """One sync_params + forward/backward writing metrics row 0, as
    test_fused_gradient_matches_autograd runs it."""
    F.counters.zero_()
    F.sync_params(args)
    F._fwd_bwd(args)
    torch.cuda.synchronize()


def _parity(F, a, b, s, z, lp, adv, ret, idx):
    """The fused gradient in b's .grad against float64 autograd with the fused step's own ReLU
    decisions and torch fp32 (_check_grads), and the metrics row against torch fp32's."""
    B, H = F.mb, F.H
    _, m_ref = _torch_grad(a, s, z, lp, adv, ret, idx)
    masks, _ = _fused_relu_masks(F, a, s, idx, B, H)
    g64 = _grad64(a, s, z, lp, adv, ret, idx, masks)
    worst = _check_grads(dict(a.actor_critic.named_parameters()),
                         dict(b.actor_critic.named_parameters()), g64)
    torch.testing.assert_close(F.metrics[0], m_ref, rtol=1e-4, atol=1e-6)
    return worst


# ------------------------------------------------------------------ gradient parity grid
@pytest.mark.parametrize("c", GRAD_CASES, ids=case_id)
def test_edge_gradient_matches_autograd(c):
    """One fused forward/backward per case against float64 autograd (see
    test_fused_gradient_matches_autograd for the criterion).  Every case has at most 130 rows:
    16-row tiles and the unbalanced ppo_wgrad partition whatever the CU count."""
    S, H, B = c[:3]
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, **case_kwargs(c))
    F = FusedPPO(b, B, 1, use_graphs=False)
    # the cases labelled general, and only those, have no tile image: the label names the path
    assert (F._tile_off is None) == (c[:3] in GRAD_GENERAL_SHAPES)
    _fused_step(F, F._args(s, z, lp, adv, ret, idx.data_ptr()))
    worst = _parity(F, a, b, s, z, lp, adv, ret, idx)
    print(f"\nEDGE grad {case_id(c)} fused error / gradient scale {worst:.3e}"
          f" clip count {int(F.metrics[0, 4])} of {B}")


@pytest.mark.parametrize("c", EXACT_CASES, ids=case_id)
def test_zero_signal_gives_exactly_zero_gradients(c):
    """adv = 0 and value_coef = 0 on a workspace that has just run an ordinary step of the same
    case (stale partials would show): dlogp = -adv * wsel * ratio / B is zero on every row and
    the entropy's derivative with respect to log_std is one, so every gradient element is exactly
    0.0 and log_std's is exactly -entropy_coef (as fp32).  The policy loss is exactly zero, as
    torch fp32's; the clip count (an integer; no ratio is within 1e-4 of the clip bounds) equals
    torch's, the KL matches at the metrics tolerance (no two fp32 sums of it are bit equal)."""
    S, H, B = c[:3]
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, **case_kwargs(c))
    F = FusedPPO(b, B, 1, use_graphs=False)
    _fused_step(F, F._args(s, z, lp, adv, ret, idx.data_ptr()))
    pb = dict(b.actor_critic.named_parameters())
    assert all(bool(p.grad.any()) for p in pb.values())  # the ordinary step wrote every gradient
    adv.zero_()
    a.value_coef = b.value_coef = 0.0
    _fused_step(F, F._args(s, z, lp, adv, ret, idx.data_ptr()))
    _, m_ref = _torch_grad(a, s, z, lp, adv, ret, idx)
    for name, p in pb.items():
        if name == "log_std":
            want = torch.full((2,), -b.entropy_coef, dtype=torch.float32, device=DEV)
            assert torch.equal(p.grad, want), (p.grad.tolist(), -b.entropy_coef)
        else:
            assert not bool(p.grad.any()), (name, p.grad.abs().max().item())
    m = F.metrics[0]
    assert m[0].item() == 0.0 and m_ref[0].item() == 0.0, (m.tolist(), m_ref.tolist())
    assert m[4].item() == m_ref[4].item(), (m.tolist(), m_ref.tolist())
    torch.testing.assert_close(m[5], m_ref[5], rtol=1e-4, atol=1e-6)
    print(f"\nEDGE zero-signal {case_id(c)} clip count {int(m[4])} of {B}")


@pytest.mark.parametrize("c", EXACT_CASES, ids=case_id)
def test_dead_units_have_exactly_zero_gradients(c):
    """shared.0.bias[j] = -1e3 for j the first unit, the first of the second wave and the last:
    unit j of h1 is off on every row, so row j of dW1, db1[j] and column j of dW2 are exactly
    zero, and the rest still passes _check_grads.  The workspace has just run a step with those
    units live (bias 0), so partials left over from it would show."""
    S, H, B = c[:3]
    dead = dead_columns(H)
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, dead=dead, **case_kwargs(c))
    F = FusedPPO(b, B, 1, use_graphs=False)
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    pb = dict(b.actor_critic.named_parameters())
    bias = pb["shared.0.bias"]
    with torch.no_grad():
        for j in dead:
            bias[j] = 0.0
    _fused_step(F, args)
    for j in dead:
        assert bool(pb["shared.0.weight"].grad[j].any()) and bool(pb["shared.2.weight"].grad[:, j].any())
    with torch.no_grad():
        for j in dead:
            bias[j] = -1e3
    _fused_step(F, args)
    for j in dead:
        assert not bool(pb["shared.0.weight"].grad[j].any()), j
        assert pb["shared.0.bias"].grad[j].item() == 0.0, j
        assert not bool(pb["shared.2.weight"].grad[:, j].any()), j
    worst = _parity(F, a, b, s, z, lp, adv, ret, idx)
    print(f"\nEDGE dead-units {case_id(c)} columns {dead} fused error / gradient scale {worst:.3e}")


# ------------------------------------------------------------------ in-kernel gradient norm
def _ulp(x):
    return torch.nextafter(x.abs(), torch.full_like(x, float("inf"))) - x.abs()


@pytest.mark.parametrize("mgn", [0.5, 100.0], ids=["clipped", "unclipped"])
@pytest.mark.parametrize("c", NORM_CASES, ids=case_id)
def test_clip_coefficient_from_in_kernel_norm(c, mgn):
    """The grads_modified == 0 optimizer path: ppo_wgrad / ppo_wsum (ppo_reduce on the general
    path) leave the gradient's sum of squares in norm_part and adam_scalars turns it into the clip
    coefficient c = min(1, max_grad_norm / (N + 1e-6)).  After one step from zeroed Adam state
    adam_m = (1 - beta1) c g and adam_v = (1 - beta2) (c g)^2 for the fused gradient g, which pins
    c, and with it the norm, per element (beta1, beta2 as the fp32 values the kernel is given;
    1 - beta is exact in fp32 for both).

    Clipped (max_grad_norm 0.5): against the float64 expressions with the float64 norm N64 of g,
    relative error at most 8 * 2^-24 + e_norm per element of m (the roundings of c, c g and the
    product) and twice that for v, where e_norm = max(4 |N_torch32 - N64| / N64, 2^-20): the
    fused norm may be 4 x as far from float64 as clip_grad_norm_'s own fp32 norm of the same g.
    A missed or doubled tile partial moves the norm by 1e-3 or more.
    Unclipped (max_grad_norm 100): c is exactly 1, so m and v equal the same fp32 expressions
    evaluated on the device, (1 - beta1) g and ((1 - beta2) g) g, within 1 ulp.
    Either way the new parameters match torch.optim.Adam after clip_grad_norm_ on the same g.
"""
    S, H, B = c[:3]
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, **case_kwargs(c))
    a.max_grad_norm = b.max_grad_norm = mgn
    F = FusedPPO(b, B, 1, use_graphs=False)
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    assert args.grads_modified == 0
    F.m.zero_()
    F.v.zero_()
    _fused_step(F, args)
    g = F.grads.clone()
    F._opt(args)
    torch.cuda.synchronize()
    assert int(F.counters[0]) == 1
    # torch: clip_grad_norm_ + Adam on the same gradient (a holds the same initial weights)
    pa = dict(a.actor_critic.named_parameters())
    pb = dict(b.actor_critic.named_parameters())
    for name, off in zip(_PARAM_ORDER, F.offs):
        p = pa[name]
        p.grad = g[off:off + p.numel()].view_as(p).clone()
    opt = torch.optim.Adam(a.actor_critic.parameters(), lr=3e-4)
    n32 = float(torch.nn.utils.clip_grad_norm_(a.actor_critic.parameters(), mgn))
    opt.step()
    g64 = g.double()
    n64 = g64.norm().item()
    b1, b2 = ctypes.c_float(0.9).value, ctypes.c_float(0.999).value
    assert (args.beta1, args.beta2) == (b1, b2)
    m_got, v_got = F.m.double(), F.v.double()
    # the fused norm as the step used it, from the coefficient on the 1,000 largest elements
    top = g64.abs().topk(min(1000, g64.numel())).indices
    c_fused = (m_got[top] / ((1.0 - b1) * g64[top])).median().item()
    if mgn == 0.5:
        assert n64 > mgn, n64
        c64 = mgn / (n64 + 1e-6)
        m_exp = (1.0 - b1) * c64 * g64
        v_exp = (1.0 - b2) * (c64 * g64) ** 2
        e_torch = abs(n32 - n64) / n64
        e_fused = abs((mgn / c_fused - 1e-6) - n64) / n64
        e_norm = max(4.0 * e_torch, 2.0 ** -20)
        tol = 8 * U32 + e_norm
        r_m = _err_over(m_got, m_exp, m_exp.abs())
        r_v = _err_over(v_got, v_exp, v_exp.abs())
        msg = (f"norm error over N64: fused {e_fused:.3e} torch fp32 {e_torch:.3e}; worst relative "
               f"error m {r_m.max().item():.3e} (bound {tol:.3e}) v {r_v.max().item():.3e} "
               f"(bound {2 * tol:.3e}); N64 {n64:.6f}")
        print(f"\nEDGE norm {case_id(c)} clipped {msg}")
        assert r_m.max().item() <= tol, msg
        assert r_v.max().item() <= 2 * tol, msg
    else:
        assert n64 < 0.5 * mgn and abs(c_fused - 1.0) < 1e-6, (n64, c_fused)
        one = torch.ones((), device=DEV)
        omb1 = one - torch.tensor(0.9, device=DEV)  # fp32, exact
        omb2 = one - torch.tensor(0.999, device=DEV)
        m_ref = omb1 * g
        v_ref = (omb2 * g) * g
        d_m = _err_over(F.m, m_ref, _ulp(m_ref))
        d_v = _err_over(F.v, v_ref, _ulp(v_ref))
        msg = f"worst distance in ulp: m {d_m.max().item():.2f} v {d_v.max().item():.2f}; N64 {n64:.6f}"
        print(f"\nEDGE norm {case_id(c)} unclipped {msg}")
        assert d_m.max().item() <= 1.0 and d_v.max().item() <= 1.0, msg
    for name in pa:
        torch.testing.assert_close(pb[name], pa[name], rtol=1e-5, atol=1e-7, msg=name)


# ------------------------------------------------------------------ acting parity
def _tile_image(S, H, flat):
    """A weight tile image of `flat` (hwy_ppo_sync_params on a workspace of its own)."""
    L = _bind(lib())
    d = PpoDims(64, S, H, 2)
    ws = torch.zeros(int(L.hwy_ppo_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8, device=DEV)
    a = PpoArgs()
    a.dims = d
    a.params, a.workspace = flat.data_ptr(), ws.data_ptr()
    check(L.hwy_ppo_sync_params(ctypes.byref(a), stream_ptr()), "hwy_ppo_sync_params")
    return ws, ws.data_ptr() + int(L.hwy_ppo_tile_image_offset(ctypes.byref(d)))


def _act_direct(agent, s, noise, tiles):
    """hwy_ppo_act itself: from the params rows (tiles None) or from a tile image."""
    flat = flat_params(agent)[0]
    B, S = s.shape
    H = agent.actor_critic.shared[0].weight.shape[0]
    out = (torch.empty(B, 2, device=DEV), torch.empty(B, 2, device=DEV),
           torch.empty(B, device=DEV), torch.empty(B, device=DEV))
    a = PpoActArgs()
    a.dims = PpoDims(B, S, H, 2)
    a.states, a.params = s.data_ptr(), flat.data_ptr()
    a.noise = None if noise is None else noise.data_ptr()
    a.action, a.pre_tanh, a.logp, a.value = (t.data_ptr() for t in out)
    a.tiles = tiles
    check(_bind(lib()).hwy_ppo_act(ctypes.byref(a), stream_ptr()), "hwy_ppo_act")
    return out


@pytest.mark.parametrize("S,H,B", ACT_CASES, ids=lambda v: str(v))
def test_act_matches_float64_model(S, H, B):
    """hwy_ppo_act against ActorCritic.act on the float64 copy of the model, with the same noise
    (clamped to [-2, 2]) and deterministic, at the acting tolerance (rtol 1e-4, atol 2e-5) on
    action, pre-tanh, log-prob and value: through fused_act (ppo_act on the params
    rows; at H = 256 ppo_act_c from an acting-only tile image, so there the params rows run
    through a direct call) and from a tile image built by hwy_ppo_sync_params (H = 256:
    ppo_act_c)."""
    b, s, noise = act_case(S, H, B)
    ref, ref_d = act64(b, s, noise)
    flat = flat_params(b)[0]
    assert (act_tiles(b, flat, S, H) is not None) == (H == 256)
    ws, image = _tile_image(S, H, flat)
    worst = 0.0
    with torch.no_grad():
        runs = {"fused_act": (fused_act(b, s, noise=noise), fused_act(b, s, deterministic=True)),
                "tile image": (_act_direct(b, s, noise, image), _act_direct(b, s, None, image))}
        if H == 256:  # fused_act took an image too: the params rows only through a direct call
            runs["params rows"] = (_act_direct(b, s, noise, None), _act_direct(b, s, None, None))
    torch.cuda.synchronize()
    for path, (got, got_d) in runs.items():
        for r, g in zip(ref + ref_d, got + got_d):
            r = r.to(DEV)
            worst = max(worst, ((g.double() - r).abs() / (2e-5 + 1e-4 * r.abs())).max().item())
            torch.testing.assert_close(g.double(), r, rtol=1e-4, atol=2e-5, msg=lambda m: f"{path}: {m}")
    print(f"\nEDGE act {S}-{H}-{B} worst error / (2e-5 + 1e-4 |ref|) {worst:.3e}")
