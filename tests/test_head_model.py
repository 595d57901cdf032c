"""tests/head_model.py (a float64 model of one row of the PPO loss head, with fp32 error bounds)
and tests/head_cases.py (the case table) against the reference's own expressions, without a GPU:

  * the model equals float64 autograd of ActorCritic.evaluate plus the loss of ppo/agent.py on
    one-row minibatches;
  * the reference in fp32 (PPOAgent(backend="torch") on the CPU) stays inside the model's bounds
    on every row and output, and no row's branch is undetermined: the reference alone meets
    every condition test_head_gpu.py puts on the kernels;
  * the K the reference needs for the squash term (the bound is K 2^-24 / u(z)) is measured on the
    table and on 2,000,001 points of [-14, 14] and is <= 4, half of the model's K = 8;
  * every mistake of head_model.MUTATIONS makes a case fail;
  * the table covers what it claims to.

Every test prints its figures (pytest -s)."""

import os

import numpy as np
import pytest
import torch
from torch.distributions import Normal

import head_cases as hc
import head_model as hm
from ppo.agent import ActorCritic, PPOAgent, _Learner

T = hc.table()
N = len(T)
S, H = 4, 64
U64_OVER_U32 = 2.0 ** -29


def _inputs(rows, dtype):
    t = lambda a: torch.as_tensor(np.asarray(a[rows], np.float64)).to(dtype)  # noqa: E731
    s = torch.as_tensor(hc.selector_states(T.mu[rows], T.val[rows], S)).to(dtype)
    return s, t(T.z), t(T.old), t(T.adv), t(T.ret)


def _ref64(i, stable, own_old=False, eps_override=None):
    """Float64 autograd of the reference's loss on the one-row minibatch i: the 11 outputs of
    head_model.flat_outputs and logp.  `stable`: the squash correction from
    4 e^{-2|z|} / (1 + e^{-2|z|})^2 instead of ActorCritic.evaluate's 1 - tanh^2.  `own_old`:
    old_logp is the row's own new log-prob, so the ratio is exactly 1."""
    li, ci = int(T.ls[i]), int(T.coef[i])
    eps, vc, ec = hc.coefs32(ci)
    if eps_override is not None:
        eps = eps_override
    ac = ActorCritic(S, 2, H).double()
    ac.load_state_dict({k: v.double() for k, v in hc.selector_state_dict(S, H, hc.LOG_STDS[li]).items()})
    s, z, old, adv, ret = _inputs([i], torch.float64)
    if stable:
        mean, std, v = ac(s)
        dist = Normal(mean, std, validate_args=False)
        e = torch.exp(-2.0 * z.abs())
        nlp = (dist.log_prob(z) - torch.log(4.0 * e / (1.0 + e) ** 2 + 1e-6)).sum(-1)
        ent = dist.entropy().sum(-1)
    else:
        nlp, v, ent = ac.evaluate(s, torch.tanh(z), z)
    if own_old:
        old = nlp.detach()
    lr = nlp - old
    r = torch.exp(lr)
    pol = -torch.min(r * adv, torch.clamp(r, 1 - eps, 1 + eps) * adv).mean()
    vl = torch.nn.functional.mse_loss(v.squeeze(-1), ret)
    loss = pol + vc * vl - ec * ent.mean()
    loss.backward()
    clip = (torch.abs(r - 1) > eps).double().sum()
    kl = ((r - 1) - lr).mean()
    p = dict(ac.named_parameters())
    vec = [pol, vl, ent.mean(), loss, clip, kl, *p["actor_mean.2.bias"].grad,
           p["critic.2.bias"].grad[0], *p["log_std"].grad]
    return np.array([float(x.detach()) for x in vec]), float(nlp.detach())


@pytest.fixture(scope="module")
def ref64():
    """(stable vectors [N, 11], stable logp [N]) once for the module."""
    out = [_ref64(i, True) for i in range(N)]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


@pytest.fixture(scope="module")
def ref32():
    """The reference in fp32: PPOAgent(backend="torch") on the CPU, one _Learner step per row
    (no optimizer step); vectors [N, 11] and ActorCritic.evaluate's log-prob [N]."""
    vec, logp = np.zeros((N, 11)), np.zeros(N)
    for (li, ci), rows in T.groups().items():
        ag = PPOAgent(S, 2, hidden_dim=H, device=torch.device("cpu"), backend="torch",
                      use_graphs=False)
        ag.actor_critic.load_state_dict(hc.selector_state_dict(S, H, hc.LOG_STDS[li]))
        ag.eps_clip, ag.value_coef, ag.entropy_coef = hc.coefs32(ci)
        s, z, old, adv, ret = _inputs(rows, torch.float32)
        L = _Learner(ag, len(rows), 1, 1, False)
        L.bind(s, z, old, adv, ret)
        p = dict(ag.actor_critic.named_parameters())
        with torch.no_grad():
            lp, _, _ = ag.actor_critic.evaluate(s, torch.tanh(z), z)
        for k, i in enumerate(rows):
            L.idx.fill_(k)
            L.row.zero_()
            L._fwd_bwd()
            g = [*p["actor_mean.2.bias"].grad, p["critic.2.bias"].grad[0], *p["log_std"].grad]
            vec[i] = [float(x) for x in [*L.metrics[0], *g]]
            logp[i] = float(lp[k])
    return vec, logp


def _model(i, mut=None, **kw):
    R = T.model([i], mut=mut, **kw)
    v, e = hm.flat_outputs(hm.minibatch(R))
    return R, v, e


@pytest.fixture(scope="module")
def model():
    out = [_model(i) for i in range(N)]
    return ([o[0] for o in out], np.stack([o[1] for o in out]), np.stack([o[2] for o in out]))


def _tol64(v, e):
    """1e-12 relative, plus the model's own error analysis at float64's unit roundoff (x 64):
    quantities such as (ratio - 1) - log_ratio cancel and have no relative precision."""
    return 1e-12 * np.abs(v) + 64.0 * U64_OVER_U32 * e


# --------------------------------------------------------------------------- the case table
def test_table_is_reproducible_and_small():
    T2 = hc.build_table()
    for a in ("z", "mu", "val", "ret", "adv", "old"):
        assert np.array_equal(getattr(T, a), getattr(T2, a)), a
    assert 200 <= N <= 400, N
    for a in ("z", "mu", "val", "ret", "adv", "old"):
        assert getattr(T, a).dtype == np.float32 and np.isfinite(getattr(T, a)).all()


def test_table_covers_values_and_branches(model):
    Rs = model[0]
    assert set(T.z.ravel().tolist()) == set(np.float32(hc.Z).tolist())
    signs = np.sign(T.z)
    assert (signs[:, 0] * signs[:, 1] < 0).sum() >= 10  # mixed pairs
    assert set(T.ls.tolist()) == {0, 1, 2, 3} and set(T.coef.tolist()) == {0, 1, 2}
    assert set(T.adv.tolist()) == set(np.float32(hc.ADV).tolist())
    assert set(T.k.ravel().tolist()) == set(hc.ZMU) and set(T.rv.tolist()) == set(hc.RETVAL)
    for d in hc.DELTAS + hc.EDGES:
        assert d in T.delta, d
    ratio = np.array([R.v["ratio"][0] for R in Rs])
    eps = np.array([hc.coefs32(int(c))[0] for c in T.coef])
    pos = np.where(ratio < 1 - eps, 0, np.where(ratio > 1 + eps, 2, 1))
    seen = {(int(p), int(np.sign(a))) for p, a in zip(pos, T.adv)}
    assert seen == {(p, a) for p in (0, 1, 2) for a in (-1, 0, 1)}, seen
    br = {(int(R.v["branch"][0]), int(R.v["inr"][0])) for R in Rs}
    # s1 < s2 and s1 > s2 need a clamped ratio (inr 0); a tie is an unclamped ratio or adv = 0
    assert br == {(0, 0), (1, 0), (2, 0), (2, 1)}, br
    tails = int((np.abs(T.z).max(1) >= 5).sum())
    assert tails >= 40, tails
    assert np.isfinite(ratio).all() and ratio.min() < 1e-12 and ratio.max() > 1e12
    print(f"\nHEAD table: {N} rows, {tails} with |z| >= 5, ratios {ratio.min():.1e} .. {ratio.max():.1e}")


def test_table_has_no_undetermined_row_and_edges_are_just_off_the_bounds(model):
    Rs = model[0]
    assert not any(R.und[0] for R in Rs)
    n = 0
    for i, d in enumerate(T.delta):
        if not isinstance(d, str):
            continue
        R = Rs[i]
        eps = hc.coefs32(int(T.coef[i]))[0]
        bound = 1 - eps if d.startswith("lo") else 1 + eps
        dist = abs(R.v["ratio"][0] - bound) / R.e["ratio"][0]
        assert hc.EDGE_MARGIN <= dist <= 4 * hc.EDGE_MARGIN, (i, d, dist)
        assert bool(R.v["inr"][0]) == d.endswith("_in"), (i, d)
        n += 1
    assert n == len(hc.EDGES) * len(hc.ADV)


# ------------------------------------------------------------- the model against float64 autograd
def test_model_matches_float64_autograd(ref64, model):
    """Against the stable form on every row, and against ActorCritic.evaluate itself where
    float64's 1 - tanh(z)^2 still has its digits (|z| <= 4: relative error below 1e-12)."""
    _, v, e = model
    rv, rlogp = ref64
    worst = float((np.abs(v - rv) / _tol64(rv, e).clip(1e-300)).max())
    assert (np.abs(v - rv) <= _tol64(rv, e)).all(), worst
    mlogp = np.array([R.v["logp"][0] for R in model[0]])
    assert (np.abs(mlogp - rlogp) <= 1e-12 * np.abs(rlogp) + 1e-13).all()
    n = 0
    for i in range(N):
        if np.abs(T.z[i]).max() > 4:
            continue
        ev, elogp = _ref64(i, False)
        assert (np.abs(v[i] - ev) <= _tol64(ev, e[i])).all(), (i, v[i], ev)
        assert abs(mlogp[i] - elogp) <= 1e-12 * abs(elogp) + 1e-13
        n += 1
    print(f"\nHEAD model vs float64 autograd: worst error / tolerance {worst:.3f} over {N} rows,"
          f" {n} of them through ActorCritic.evaluate")


# ---------------------------------------------------------- the reference in fp32 inside the bounds
def test_reference_fp32_is_inside_the_bounds(ref32, model):
    Rs, v, e = model
    rv, rlogp = ref32
    over = np.abs(rv - v) / np.maximum(e, 1e-300)
    over[(rv == v)] = 0.0
    i, k = np.unravel_index(np.argmax(over), over.shape)
    assert over.max() <= 1.0, (int(i), hm.OUTPUT_NAMES[k], rv[i, k], v[i, k], e[i, k])
    mlogp = np.array([R.v["logp"][0] for R in Rs])
    elogp = np.array([R.e["logp"][0] for R in Rs])
    lo = np.abs(rlogp - mlogp) / elogp
    assert lo.max() <= 1.0, (int(lo.argmax()), lo.max())
    print(f"\nHEAD reference fp32 (torch, CPU): worst error / bound {over.max():.3f}"
          f" ({hm.OUTPUT_NAMES[k]}, row {int(i)}), logp {lo.max():.3f}")


def _k_needed(z32):
    """The K that torch's fp32 log1p(-tanh(z)^2 + 1e-6) needs at these points."""
    z = torch.as_tensor(np.array(z32))
    q32 = torch.log1p(-torch.tanh(z).pow(2) + 1e-6).double().numpy()
    z64 = z.double().numpy()
    q64 = np.log(hm.squash_u(z64))
    return np.abs(q32 - q64) * hm.squash_u(z64) / hm.U, np.abs(q32 - q64)


_README = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                       "profiles", "r14", "head", "README.md")
_MARK = "<!-- written by tests/test_head_model.py::test_reference_needs_k_below_4 -->\n"
_END = "<!-- end -->"


def _record(line):
    """The measured K into profiles/r14/head/README.md, between its two markers (left alone
    when the line is already there or the file cannot be written)."""
    try:
        with open(_README) as f:
            text = f.read()
        head, rest = text.split(_MARK)
        new = head + _MARK + line + "\n" + rest[rest.index(_END):]
        if new != text:
            with open(_README, "w") as f:
                f.write(new)
    except (OSError, ValueError):
        pass


def test_reference_needs_k_below_4():
    kt, _ = _k_needed(np.ascontiguousarray(T.z.ravel()))
    grid = np.linspace(-14.0, 14.0, 2_000_001).astype(np.float32)
    kg, err = _k_needed(grid)
    line = (f"Reference K (torch fp32 on the CPU): {kt.max():.3f} on the table,"
            f" {kg.max():.3f} on 2,000,001 points of [-14, 14] (at z = {grid[kg.argmax()]:.4f});"
            f" worst absolute error {err.max():.3e} at z = {grid[err.argmax()]:.4f}")
    print("\nHEAD squash term. " + line)
    _record(line)
    assert max(kt.max(), kg.max()) <= 4.0
    assert hm.K_SQUASH == 8.0 and hm.K_SQUASH < hm.SQUASH_EPS / hm.U


# -------------------------------------------------------------------------------- mutations
def _clip_boundary(mut):
    """eps_clip = 0 and old_logp the row's own log-prob: the ratio is exactly 1 and
    |ratio - 1| > eps is false (ppo/agent.py's strict comparison), in the reference as in the
    model."""
    ref, _ = _ref64(0, True, own_old=True, eps_override=0.0)
    li = int(T.ls[0])
    _, vc, ec = hc.coefs32(int(T.coef[0]))
    R0 = T.model([0])
    R = hm.head_rows(T.mu[[0]], T.val[[0]], T.z[[0]], R0.v["logp"], T.adv[[0]], T.ret[[0]],
                     np.float32(hc.LOG_STDS[li]), 0.0, vc, ec, 1, mut=mut)
    v, e = hm.flat_outputs(hm.minibatch(R))
    assert ref[4] == 0.0
    return bool((np.abs(v - ref) <= _tol64(ref, e) + 1e-15).all())


def test_clip_boundary_case_passes_unmutated():
    assert _clip_boundary(None)


@pytest.mark.parametrize("mut", hm.MUTATIONS)
def test_every_mutation_fails_a_case(mut, ref64, ref32, model):
    """The float64 comparison of test_model_matches_float64_autograd, with the model's mistake
    `mut`: at least one row (for clip_ge: the boundary case) must fail it.  The fp32 bounds see
    it too: the reference's fp32 is outside the mistaken model's bounds on at least one row
    (but for clip_ge, which no fp32 row can show: its ratio would have to be exactly 1 +- eps)."""
    rv, _ = ref64
    r32, _ = ref32
    e = model[2]
    failed = outside = 0
    for i in range(N):
        _, v, em = _model(i, mut)
        failed += int(not (np.abs(v - rv[i]) <= _tol64(rv[i], e[i])).all())
        outside += int((np.abs(r32[i] - v) > em).any())
    if mut == "clip_ge":
        failed += int(not _clip_boundary(mut))
    print(f"\nHEAD mutation {mut}: {failed} failing cases; the reference's fp32 is outside the"
          f" bounds on {outside} rows")
    assert failed >= 1, mut
    assert outside >= 1 or mut == "clip_ge", mut


def test_dropped_eps_is_outside_the_fp32_bounds_at_every_tail_row(ref32, model):
    """The bound's K = 8 is half of 1e-6 / 2^-24: with the 1e-6 dropped from the model, the
    reference's fp32 log-prob is outside the bound on every row with a |z| >= 3."""
    _, rlogp = ref32
    rows = [i for i in range(N) if np.abs(T.z[i]).max() >= 3]
    ratios = []
    for i in rows:
        R = T.model([i], mut="eps_dropped")
        ratios.append(abs(rlogp[i] - R.v["logp"][0]) / R.e["logp"][0])
    print(f"\nHEAD dropped 1e-6: reference fp32 error / bound min {min(ratios):.2f} over {len(rows)} rows")
    assert min(ratios) > 1.0
