"""Helpers shared by test_attribution.py (CPU) and test_attribution_gpu.py: the plain-loop
restatement of training.routine.attribution_from / attribution_stats, float64 input gradients
under given ReLU decisions, and agents whose first layer reads chosen observation columns only."""

import copy
import math

import numpy as np
import pytest
import torch

from ppo_ref_util import _MaskMul


def attribution_loop(base, grads, alive, F, ego, ranked=True):
    """attribution_from as loops over samples, rows and columns (numpy, float64 sums)."""
    base, grads, alive = (np.asarray(t) for t in (base, grads, alive))
    B, N, _ = base.shape
    Fo = grads.shape[2] // N
    by_row = np.zeros((3, N, Fo))
    by_rank = np.zeros((3, N, Fo))
    count = 0
    for b in range(B):
        if not alive[b]:
            continue
        count += 1
        others = [n for n in range(N) if n != ego]
        present = [n for n in others if any(base[b, n, f] != 0.0 for f in range(F))]
        absent = [n for n in others if n not in present]

        def key(n):
            x, y = float(base[b, n, 0]), float(base[b, n, 1])
            return (math.sqrt(x * x + y * y), n)

        order = [ego] + sorted(present, key=key) + absent
        for k in range(3):
            g = np.abs(grads[k, b].reshape(N, Fo)).astype(np.float64)
            for n in range(N):
                for f in range(Fo):
                    by_row[k, n, f] += g[n, f]
                    by_rank[k, n, f] += g[order[n], f]
    return {"by_row": by_row, "by_rank": by_rank if ranked else None, "count": count}


def stats_loop(sums, F, ego):
    """attribution_stats restated."""
    n = sums["count"]
    by_row = sums["by_row"]
    Fo = by_row.shape[2]
    out = {"samples": n, "by_row": by_row / n if n else np.zeros_like(by_row),
           "by_rank": None if sums["by_rank"] is None
           else (sums["by_rank"] / n if n else np.zeros_like(by_row)),
           "pe_share": None if Fo == F else [], "ego_share": []}
    for k in range(3):
        total = by_row[k].sum()
        if Fo != F:
            out["pe_share"].append(by_row[k][:, F:].sum() / total if total > 0 else None)
        out["ego_share"].append(by_row[k][ego].sum() / total if total > 0 else None)
    return out


def assert_stats_close(got, want, rtol=1e-12):
    assert got["samples"] == want["samples"]
    for key in ("by_row", "by_rank"):
        if want[key] is None:
            assert got[key] is None, key
        else:
            np.testing.assert_allclose(np.asarray(got[key], dtype=np.float64), want[key],
                                       rtol=rtol, atol=0.0, err_msg=key)
    for key in ("pe_share", "ego_share"):
        if want[key] is None:
            assert got[key] is None, key
            continue
        assert len(got[key]) == 3
        for g, w in zip(got[key], want[key]):
            if w is None:
                assert g is None, key
            else:
                assert g == pytest.approx(w, rel=rtol, abs=0.0), (key, g, w)


def masks_of(model, x):
    """The model's own ReLU decisions on x (its dtype's pre-activations > 0), as float64 masks
    in ppo_ref_util's naming."""
    with torch.no_grad():
        z1 = model.shared[0](x)
        z2 = model.shared[2](torch.relu(z1))
        h = torch.relu(z2)
        za, zc = model.actor_mean[0](h), model.critic[0](h)
    return {k: (z > 0).double() for k, z in (("z1", z1), ("z2", z2), ("za", za), ("zc", zc))}


def grads64(model, x, masks):
    """d(mean_0, mean_1, value)/dx in float64 autograd with the four ReLUs replaced by `masks`:
    (3, B, S)."""
    m = copy.deepcopy(model).double().to(x.device)
    m.shared[1], m.shared[3] = _MaskMul(masks["z1"]), _MaskMul(masks["z2"])
    m.actor_mean[1], m.critic[1] = _MaskMul(masks["za"]), _MaskMul(masks["zc"])
    xd = x.double().clone().requires_grad_(True)
    mean, _, value = m(xd)
    outs = (mean[:, 0].sum(), mean[:, 1].sum(), value.sum())
    return torch.stack([torch.autograd.grad(o, xd, retain_graph=True)[0] for o in outs])


def keep_columns(agent, cols):
    """Zero W1 outside the observation columns `cols`, in place and without bumping what a
    later test reads (done before any gradient call)."""
    W1 = agent.actor_critic.shared[0].weight
    keep = torch.zeros(W1.shape[1], dtype=torch.bool, device=W1.device)
    keep[list(cols)] = True
    with torch.no_grad():
        W1.mul_(keep.to(W1.dtype))


def draw_case(B, N, F, Fo, seed):
    """Base rows with ties in distance, absent rows and an all-zero ego row among them, drawn
    gradients and an alive mask with dead samples."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(B, N, F, generator=g)
    base[0, 1, :2] = base[0, 4, :2]            # the same point: ordered by row index
    base[1, 3, 0], base[1, 3, 1] = -base[1, 1, 0], base[1, 1, 1]  # mirrored: the same distance
    base[2, 2:, :] = 0.0                       # absent vehicles
    base[3, 1, :] = 0.0
    base[3, N - 1, :] = 0.0
    base[4, 0, :] = 0.0                        # an all-zero row where the ego may sit
    base[4, 2, :] = 0.0
    base[5, 1, :2] = 0.0                       # distance 0 but present (nonzero velocity)
    grads = torch.randn(3, B, N * Fo, generator=g)
    alive = torch.rand(B, generator=g) > 0.3
    alive[:6] = True
    alive[6] = False
    return base, grads, alive
