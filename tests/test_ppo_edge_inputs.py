"""Conditions on the inputs of test_ppo_edges_gpu.py, checked without a GPU from the float64
reference alone: the cases are drawn with CPU generators (ppo_ref_util.edge_case / act_case), so
what holds here holds for the bits the GPU tests see.  These are conditions on the inputs, met by
the seeds in ppo_ref_util.GRAD_CASES, not tolerances of the kernels."""

import pytest
import torch

from ppo_ref_util import (ACT_CASES, COEFS, EXACT_CASES, GRAD_CASES, LOG_STDS, NORM_CASES, _grad64,
                          _grads_agree, _ratio64, _torch_grad, act64, act_case, case_id,
                          case_kwargs, dead_columns, edge_case)

CPU = torch.device("cpu")


def check_grad_inputs(c, dead=()):
    """Every condition on one gradient case; returns the figures (fp32-vs-float64 error over the
    gradient scale, clipped share, float64 gradient norm)."""
    S, H, B = c[:3]
    kw = case_kwargs(c)
    a, _, s, z, lp, adv, ret, idx = edge_case(S, H, B, device=CPU, dead=dead, **kw)
    assert float(z.abs().max()) <= 3.0
    # torch fp32 autograd against plain float64 autograd: no ReLU decision of the case sits at
    # rounding level either (a flipped unit moves a whole weight-gradient row past the bound)
    _torch_grad(a, s, z, lp, adv, ret, idx)
    g64 = _grad64(a, s, z, lp, adv, ret, idx)
    err = _grads_agree(dict(a.actor_critic.named_parameters()), g64)
    r = _ratio64(a, s, z, lp, idx)
    eps = kw["eps_clip"]
    # no clip decision at rounding level: 1e-4 is 100 x the fp32 error of the ratio
    margin = torch.minimum((r - (1 + eps)).abs(), (r - (1 - eps)).abs()).min().item()
    assert margin > 1e-4, margin
    share = ((r - 1).abs() > eps).double().mean().item()
    if B >= 32 and kw["sigma"] > 0.05:
        assert 0.2 <= share <= 0.8, share
        av = adv[idx].double()
        for pos in (av > 0, av < 0):
            for out in (r > 1 + eps, r < 1 - eps):
                assert int((pos & out).sum()) >= 1, "an (advantage sign, clip side) cell is empty"
    norm = torch.sqrt(sum((g * g).sum() for g in g64.values())).item()
    return dict(err=err, share=share, norm=norm, margin=margin)


def test_settings_reach_the_new_widths():
    """Every log_std and every (eps_clip, value_coef, entropy_coef) setting appears at H 256, 320
    and 448 at least once; the shapes are distinct."""
    assert len({c[:3] for c in GRAD_CASES}) == len(GRAD_CASES)
    for H in (256, 320, 448):
        assert {c[3] for c in GRAD_CASES if c[1] == H} == set(range(len(LOG_STDS))), H
        assert {c[4] for c in GRAD_CASES if c[1] == H} == set(range(len(COEFS))), H
    assert all(c[2] <= 130 for c in GRAD_CASES)


@pytest.mark.parametrize("c", GRAD_CASES, ids=case_id)
def test_gradient_case_inputs(c):
    f = check_grad_inputs(c)
    if c in NORM_CASES:  # the clipped step of the in-kernel norm test really clips
        assert f["norm"] > 0.5, f["norm"]


@pytest.mark.parametrize("c", EXACT_CASES, ids=case_id)
def test_dead_unit_case_inputs(c):
    """The dead-unit variant is a case of its own (its old_logp is drawn with the units off): the
    same conditions, and in float64 the dead units' gradients are exactly zero."""
    S, H, B = c[:3]
    dead = dead_columns(H)
    check_grad_inputs(c, dead=dead)
    a, _, s, z, lp, adv, ret, idx = edge_case(S, H, B, device=CPU, dead=dead, **case_kwargs(c))
    g64 = _grad64(a, s, z, lp, adv, ret, idx)
    for j in dead:
        assert not g64["shared.0.weight"][j].any() and g64["shared.0.bias"][j] == 0
        assert not g64["shared.2.weight"][:, j].any()


@pytest.mark.parametrize("c", EXACT_CASES, ids=case_id)
def test_zero_signal_case_inputs(c):
    """adv = 0 and value_coef = 0: in float64 and in torch fp32 every gradient is exactly zero but
    log_std's, which is -entropy_coef (the entropy's unit derivative; autograd sums B terms of
    1 / B, so up to that sum's rounding)."""
    S, H, B = c[:3]
    a, _, s, z, lp, adv, ret, idx = edge_case(S, H, B, device=CPU, **case_kwargs(c))
    adv.zero_()
    a.value_coef = 0.0
    _torch_grad(a, s, z, lp, adv, ret, idx)
    g64 = _grad64(a, s, z, lp, adv, ret, idx)
    for name, p in a.actor_critic.named_parameters():
        if name == "log_std":  # B terms of 1 / B: -entropy_coef up to the rounding of that sum
            want = torch.full((2,), -a.entropy_coef, dtype=torch.float64)
            torch.testing.assert_close(p.grad.double(), want, rtol=1e-6, atol=0)
            torch.testing.assert_close(g64[name], want, rtol=1e-12, atol=0)
        else:
            assert not p.grad.any() and not g64[name].any(), name


@pytest.mark.parametrize("S,H,B", ACT_CASES, ids=lambda v: str(v))
def test_act_case_inputs(S, H, B):
    """torch fp32 act meets the acting tolerance (rtol 1e-4, atol 2e-5) against the float64 model
    on every acting case, sampled and deterministic, and |z| stays within 3."""
    b, s, noise = act_case(S, H, B, device=CPU)
    ref, ref_d = act64(b, s, noise)
    got = b.actor_critic.act(s, noise=noise)
    got_d = b.actor_critic.act(s, deterministic=True)
    assert float(ref[1].abs().max()) <= 3.0
    for r, g in zip(ref + ref_d, got + got_d):
        torch.testing.assert_close(g.double(), r, rtol=1e-4, atol=2e-5)
