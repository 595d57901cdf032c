"""Shared by tests/test_wgrad_bits_gpu.py and tools/record_wgrad_bits.py: the shapes at which
ppo_wgrad's chunk loop is pinned bit for bit, one fused forward/backward per shape on CPU-drawn
inputs (ppo_ref_util.edge_case), and the SHA-256 digests of what it leaves behind."""

import hashlib
import json
import os

import torch

from ppo_ref_util import (COEFS, LOG_STDS, SIGMA, _check_grads, _fused_relu_masks, _grad64,
                          _torch_grad, edge_case)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_parent_bits.json")

# (S, H, B).  H = 64 has three 128 x 64 tiles.  B 40: one ragged chunk; 64: one whole chunk,
# split 1; 520: 8 slices of 65 rows, one whole chunk plus a 1-row masked one; 1,100: slices of
# 138 rows, ragged third chunk; 1,536: three whole chunks per slice.
SMALL = tuple((S, 64, B) for S in (8, 60) for B in (40, 64, 520, 1100, 1536))
# the bench shape (8 chunks per workgroup), and the balanced partition (two partial slots, the
# extras walking several tiles in one workgroup)
LARGE = ((60, 256, 4096), (60, 256, 16384))
SHAPES = SMALL + LARGE


def shape_id(c):
    return "-".join(str(x) for x in c)


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def norm_partials(F):
    """The fused path's sum-of-squares partials in the workspace: [nh] from ppo_wgrad's head-sum
    workgroups, then 8 per 128 x 64 tile from ppo_wsum.  The workspace is carved in 256-B aligned
    sub-buffers: h1, h2, ac, dac, dh2, dh1, the head partials, then the norm partials (the
    split-K slabs between them are empty on the fused path)."""
    B, S, H = F.mb, F.S, F.H
    al = lambda k: (k + 63) // 64 * 64  # noqa: E731
    off = 4 * al(B * H) + 2 * al(2 * B * H) + al((B + 15) // 16 * (3 * H + 16))
    tm, tn = (H + 127) // 128, (H + 63) // 64
    ntile = (2 * H + 127) // 128 * tn + tm * tn + tm * ((S + 63) // 64)
    n = (3 * H + 9 + 63) // 64 + 8 * ntile
    return F.workspace.view(torch.float32)[off:off + n]


def run_case(c):
    """One sync_params + forward/backward at shape c, checked against float64 autograd with the
    fused step's own ReLU decisions and torch fp32 (test_edge_gradient_matches_autograd's
    criterion) and, for the norm partials, against the gradient's own sum of squares.  Returns
    the digests of the flat gradient, the norm partials and the metrics row."""
    from hwy.ppo_native import FusedPPO

    S, H, B = c
    eps, vc, ec = COEFS[0]
    a, b, s, z, lp, adv, ret, idx = edge_case(S, H, B, log_std=LOG_STDS[0], sigma=SIGMA,
                                              eps_clip=eps, value_coef=vc, entropy_coef=ec, seed=0)
    F = FusedPPO(b, B, 1, use_graphs=False)
    args = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F.counters.zero_()
    F.sync_params(args)
    F._fwd_bwd(args)
    torch.cuda.synchronize()
    got = {"grads": _sha(F.grads), "norm_partials": _sha(norm_partials(F)),
           "metrics": _sha(F.metrics[0])}
    _, m_ref = _torch_grad(a, s, z, lp, adv, ret, idx)
    masks, _ = _fused_relu_masks(F, a, s, idx, B, H)
    g64 = _grad64(a, s, z, lp, adv, ret, idx, masks)
    worst = _check_grads(dict(a.actor_critic.named_parameters()),
                         dict(b.actor_critic.named_parameters()), g64, shape_id(c))
    torch.testing.assert_close(F.metrics[0], m_ref, rtol=1e-4, atol=1e-6)
    # every partial is a sum of squares of gradient elements, each element in exactly one
    n2, p2 = F.grads.double().square().sum().item(), norm_partials(F).double().sum().item()
    assert abs(p2 - n2) <= 1e-5 * n2, (shape_id(c), p2, n2)
    print(f"\nWGRAD bits {shape_id(c)} fused error / gradient scale {worst:.3e}"
          f" sum of partials / |g|^2 - 1 = {p2 / n2 - 1:.2e}")
    return got


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)
