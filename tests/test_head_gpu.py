"""The PPO loss head and action sampling of the kernels against tests/head_model.py, row by row,
over the case table of tests/head_cases.py (|z| up to 12, ratios from 1e-13 to 1e13, every clip
branch): the fused row kernels (ppo_rows_body.inc; H = 64, 128, 320, 256 and the 32- and 64-row
tiles), the general path's ppo_head, ppo_act (ppo_act_body.inc) and ppo_act_c
(ppo_act_c_body.inc).

The selector network (head_cases.selector_state_dict) passes state columns 0..2 through as mu0,
mu1 and val bit for bit, so the head's inputs are known exactly; with one live row per minibatch
(the others have adv = 0 and ret = val and add exact zeros) the gradients of actor_mean.2.bias,
critic.2.bias and log_std and the metrics row are that row's own terms, with no summation between
the head and the public buffers.  Every comparison is |kernel - model| <= the model's bound;
test_head_model.py shows on the CPU that the reference's fp32 meets the same bounds, that the
table has no row whose branch is undetermined, and that the bounds see a dropped 1e-6.

Every test prints its worst error over bound (pytest -s)."""

import copy
import ctypes

import numpy as np
import pytest
import torch

import head_cases as hc
import head_model as hm
from hwy.native import check, lib, stream_ptr
from hwy.ppo_native import (_PARAM_ORDER, FusedPPO, PpoActArgs, PpoArgs, PpoDims, _bind, flat_params,
                            fused_act)
from ppo_ref_util import _gamma

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
T = hc.table()
N_NULL = 17


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _agent(S, H, li=0, ci=0):
    from ppo.agent import PPOAgent

    ag = PPOAgent(S, 2, lr=3e-4, epochs=2, hidden_dim=H, device=DEV, use_graphs=False,
                  backend="hip")
    ag.actor_critic.load_state_dict(hc.selector_state_dict(S, H, hc.LOG_STDS[li]))
    ag.eps_clip, ag.value_coef, ag.entropy_coef = hc.coefs32(ci)
    return ag


def _null_rows(li, n=N_NULL):
    """Rows that add exact zeros to every sum but the KL's: adv = 0, ret = val, and old_logp the
    model's own log-prob (ratio 1 to rounding)."""
    j = np.arange(n)
    mu = np.stack([0.25 * (j % 3 + 1), -0.5 - 0.125 * (j % 4)], 1).astype(np.float32)
    sigma = np.exp(np.float32(hc.LOG_STDS[li]).astype(np.float64))
    z = (mu + sigma * np.stack([0.5 - 0.25 * (j % 5), 0.125 * (j % 7) - 0.25], 1)).astype(np.float32)
    val = (1.5 - 0.25 * (j % 6)).astype(np.float32)
    logp = hm.logp_rows(mu, z, np.float32(hc.LOG_STDS[li]))[0]
    return dict(mu=mu, val=val, z=z, old=logp.astype(np.float32), adv=np.zeros(n, np.float32),
                ret=val.copy())


def _pool(live, li):
    """The table rows `live` followed by N_NULL null rows, as arrays."""
    nl = _null_rows(li)
    t = dict(mu=T.mu[live], val=T.val[live], z=T.z[live], old=T.old[live], adv=T.adv[live],
             ret=T.ret[live])
    return {k: np.concatenate([t[k], nl[k]]) for k in t}


class Runner:
    """One FusedPPO of minibatch size B on the selector network; run() steps it over the given
    minibatches of a row pool and returns, per step, the 11 numbers of head_model.flat_outputs
    as the public buffers hold them."""

    def __init__(self, S, H, B):
        self.S, self.H, self.B = S, H, B
        self.ag = _agent(S, H)
        self.F = FusedPPO(self.ag, B, 1, use_graphs=False)
        self.off = dict(zip(_PARAM_ORDER, self.F.offs))

    def set_group(self, li, ci):
        with torch.no_grad():
            self.ag.actor_critic.log_std.copy_(torch.tensor(np.float32(hc.LOG_STDS[li])))
        self.ag.eps_clip, self.ag.value_coef, self.ag.entropy_coef = hc.coefs32(ci)

    def run(self, pool, idx):
        F, B = self.F, self.B
        idx = np.ascontiguousarray(idx, np.int64).reshape(-1, B)
        dev = lambda a: torch.as_tensor(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
        s = dev(hc.selector_states(pool["mu"], pool["val"], self.S))
        z, old, adv, ret = (dev(pool[k]) for k in ("z", "old", "adv", "ret"))
        ix = dev(idx)
        out = torch.zeros(idx.shape[0], 11, device=DEV)
        a = F._args(s, z, old, adv, ret, ix.data_ptr())
        F.sync_params(a)
        g, o = F.grads, self.off
        oa, oc, ol = o["actor_mean.2.bias"], o["critic.2.bias"], o["log_std"]
        for k in range(idx.shape[0]):
            a.idx = ix.data_ptr() + k * B * 8
            F.counters.zero_()
            F._fwd_bwd(a)
            out[k, :6].copy_(F.metrics[0])
            out[k, 6:8].copy_(g[oa:oa + 2])
            out[k, 8:9].copy_(g[oc:oc + 1])
            out[k, 9:11].copy_(g[ol:ol + 2])
        torch.cuda.synchronize()
        return out.double().cpu().numpy()


def _expect(pool, idx, li, ci, B, mut=None):
    eps, vc, ec = hc.coefs32(ci)
    R = hm.head_rows(pool["mu"][idx], pool["val"][idx], pool["z"][idx], pool["old"][idx],
                     pool["adv"][idx], pool["ret"][idx], np.float32(hc.LOG_STDS[li]), eps, vc, ec,
                     B, mut=mut)
    v, e = hm.flat_outputs(hm.minibatch(R))
    return R, v, e


def _over(got, v, e):
    """|got - v| / e per output; an output with bound 0 (the clip count) must be equal."""
    d = np.abs(got - v)
    return np.where(d == 0, 0.0, d / np.maximum(e, 1e-300))


def _sweep(S, H, label):
    """Every table row as a one-row minibatch, and the position sweep on a 20-row subset: one
    live row at tile position p of a B = 16 (p = 0..15) or B = 17 (p = 0, 16) minibatch."""
    worst, where = 0.0, None
    # one-row minibatches on which the kernel is outside the bounds of a model with a mistake
    # (the 1e-6 dropped: counted on rows with |z| >= 3 only); clip_ge needs a ratio of exactly
    # 1 +- eps, which no fp32 row can promise, and stays with the CPU's boundary case
    seen = {m: 0 for m in hm.MUTATIONS if m != "clip_ge"}
    if S % 4 == 0:  # first: the selector network hands mu and val through bit for bit
        s = torch.as_tensor(hc.selector_states(T.mu, T.val, S)).to(DEV)
        _, z_d, lp_d, v_d = _act_direct(_agent(S, H), s, None, None)
        assert np.array_equal(z_d.cpu().numpy(), T.mu) and np.array_equal(v_d.cpu().numpy(), T.val)
        assert not bool(lp_d.any())
    runs = [(1, [(i, 0) for i in range(len(T))])]
    sub = hc.sweep_subset(T)
    runs.append((16, [(i, p) for i in sub for p in range(16)]))
    runs.append((17, [(i, p) for i in sub for p in (0, 16)]))
    for B, steps in runs:
        Rn = Runner(S, H, B)
        for (li, ci), rows in T.groups().items():
            rs = set(rows)
            mine = [(i, p) for i, p in steps if i in rs]
            if not mine:
                continue
            live = sorted({i for i, _ in mine})
            pool = _pool(live, li)
            nl = len(live)
            idx = np.zeros((len(mine), B), np.int64)
            for k, (i, p) in enumerate(mine):
                idx[k] = nl + (np.arange(B) + k) % N_NULL
                idx[k, p] = live.index(i)
            Rn.set_group(li, ci)
            got = Rn.run(pool, idx)
            for k, (i, p) in enumerate(mine):
                R, v, e = _expect(pool, idx[k], li, ci, B)
                assert not R.und.any(), (label, i)
                ov = _over(got[k], v, e)
                if ov.max() > worst:
                    worst, where = float(ov.max()), (B, i, p, hm.OUTPUT_NAMES[int(ov.argmax())])
                assert ov.max() <= 1.0, (label, B, i, p, hm.OUTPUT_NAMES[int(ov.argmax())],
                                         got[k].tolist(), v.tolist(), e.tolist())
                for mut in seen if B == 1 else ():
                    if mut == "eps_dropped" and np.abs(T.z[i]).max() < 3:
                        continue
                    _, vm, em = _expect(pool, idx[k], li, ci, B, mut=mut)
                    seen[mut] += int(_over(got[k], vm, em).max() > 1.0)
    print(f"\nHEAD {label}: worst error / bound {worst:.3f} at (B, row, position, output) {where};"
          f" the model without the 1e-6 fails {seen['eps_dropped']} rows with |z| >= 3; rows failing"
          f" under the model's other mistakes: {seen}")
    assert all(n >= 1 for n in seen.values()), seen


@pytest.mark.parametrize("H", [64, 128, 320, 256])
def test_fused_rows_head_pointwise(H):
    """The fused row kernels: two 4-wave widths (64, 320), an 8-wave width (128) and the compact
    kernel of H = 256."""
    _sweep(4, H, f"fused rows H={H}")


def test_general_path_head_pointwise():
    """S = 5 is no multiple of 4: the general path, whose loss head is ppo_head."""
    _sweep(5, 64, "general path (ppo_head) S=5 H=64")


@pytest.mark.parametrize("H,tile", [(64, 32), (320, 16), (256, 32), (256, 64)])
def test_large_launch_scattered_live_rows(H, tile):
    """One launch at B = 32 x CUs (32-row tiles at H <= 256) and, for H = 256, at
    B = 64 x CUs + 16 (64-row tiles, the last one ragged): 8 live rows at scattered positions,
    the last tile included; every other row is null."""
    B = 64 * _cus() + 16 if tile == 64 else 32 * _cus()
    (li, ci), rows = max(T.groups().items(), key=lambda kv: len(kv[1]))
    order = sorted(rows, key=lambda i: -float(np.abs(T.z[i]).max()))
    live = order[:4] + order[-4:]
    pos = [0, 15, 16, tile + 1, B // 2 + 3, B - 17, B - 16, B - 1]
    nl = _null_rows(li)
    pool = {k: nl[k][np.arange(B) % N_NULL].copy() for k in nl}
    idx = (B - 1 - np.arange(B)).astype(np.int64)  # the minibatch reads the pool backwards
    for i, p in zip(live, pos):
        for k, src in (("mu", T.mu), ("val", T.val), ("z", T.z), ("old", T.old), ("adv", T.adv),
                       ("ret", T.ret)):
            pool[k][idx[p]] = src[i]
    Rn = Runner(4, H, B)
    Rn.set_group(li, ci)
    got = Rn.run(pool, idx)[0]
    R, v, e = _expect(pool, idx, li, ci, B)
    assert not R.und.any()
    ov = _over(got, v, e)
    print(f"\nHEAD large launch H={H} B={B}: worst error / bound {ov.max():.3f}"
          f" ({hm.OUTPUT_NAMES[int(ov.argmax())]})")
    assert ov.max() <= 1.0, (got.tolist(), v.tolist(), e.tolist())


# ------------------------------------------------------------------------------------ acting
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


def _act_inputs(li, B):
    """B acting rows under log_std pair li: mu and val from the table (cycled), the noise
    unclamped and chosen so that z lands on the table's z of the same row; every fifth row's
    noise is +-5.5 instead."""
    j = np.arange(B) % len(T)
    mu, val = T.mu[j], T.val[j]
    sigma = np.exp(np.float32(hc.LOG_STDS[li]).astype(np.float64))
    noise = ((T.z[j].astype(np.float64) - mu) / sigma).astype(np.float32)
    k = np.arange(B)
    noise[k % 5 == 4, 0] = 5.5
    noise[k % 5 == 4, 1] = -5.5
    noise[k % 10 == 9] *= -1.0
    return mu, val, noise


def _check_act(label, li, mu, val, noise, got, got_d):
    act, z, lp, v = (t.double().cpu().numpy() for t in got)
    act_d, z_d, lp_d, v_d = (t.cpu().numpy() for t in got_d)
    ls = np.float32(hc.LOG_STDS[li])
    z_ref, e_z, _ = hm.act_rows(mu, noise, ls)
    o_real = _over(z, z_ref, e_z).max()  # from the real exp(log_std): a third rounding, printed
    # the scale is an fp32 in the reference and in the kernels: one value per component, within
    # 1 ulp of exp(log_std), from which every row of the launch is within 2 roundings
    o_z, which = 0.0, []
    for c in range(2):
        per = []
        for sc in hm.scale_candidates(ls[c]):
            zr, ez, _ = hm.act_rows(mu[:, c], noise[:, c], ls[c], scale=sc)
            per.append(_over(z[:, c], zr, ez).max())
        o_z = max(o_z, min(per))
        which.append((0, -1, 1)[int(np.argmin(per))])
    t64 = np.tanh(z)
    o_t = (np.abs(act - t64) / hm.ulp32(t64)).max()
    logp, e_lp = hm.act_logp(mu, z, ls)
    o_lp = _over(lp, logp, e_lp)
    tail = np.abs(z).max(1) >= 3
    logp_m, e_m = hm.act_logp(mu, z, ls, mut="eps_dropped")
    blind = int((_over(lp, logp_m, e_m)[tail] > 1.0).sum())
    print(f"\nHEAD act {label} log_std {hc.LOG_STDS[li]}: z error / 2 roundings {o_z:.3f} (scale"
          f" {which} ulp from exp rounded; {o_real:.3f} from the real exp), action"
          f" {o_t:.2f} ulp from tanh, logp error / bound {o_lp.max():.3f}, max |z| {np.abs(z).max():.1f};"
          f" the model without the 1e-6 fails {blind} of {int(tail.sum())} rows with |z| >= 3")
    assert np.array_equal(v, val.astype(np.float64)) and np.array_equal(v_d, val)
    assert o_z <= 1.0
    assert o_t <= 4.0 and np.abs(act).max() <= 1.0
    assert o_lp.max() <= 1.0, (int(o_lp.argmax()), z[o_lp.argmax()])
    assert blind >= 1
    assert np.array_equal(z_d, mu) and not lp_d.any()
    assert (np.abs(act_d.astype(np.float64) - np.tanh(mu.astype(np.float64)))
            <= 4.0 * hm.ulp32(np.tanh(mu.astype(np.float64)))).all()


@pytest.mark.parametrize("H", [64, 320])
def test_act_pointwise(H):
    """hwy_ppo_act (ppo_act) from the params rows and from a tile image: the sampled z within 2
    roundings of mu + scale noise, scale the fp32 exp(log_std) (the same for every row; correctly
    rounded or a neighbour: against the real exp the MI355X measures 1.31 x 2 roundings, the
    third rounding being the scale's own), the action within 4 ulp of tanh(z) and inside [-1, 1],
    the log-prob within the model's bound at the kernel's own z, the value and the deterministic
    z bit for bit mu, the deterministic log-prob 0."""
    B = len(T) + 9  # 257: 16 whole tiles and one row
    for li in range(len(hc.LOG_STDS)):
        ag = _agent(4, H, li)
        flat = flat_params(ag)[0]
        ws, image = _tile_image(4, H, flat)
        mu, val, noise = _act_inputs(li, B)
        s = torch.as_tensor(hc.selector_states(mu, val, 4)).to(DEV)
        nz = torch.as_tensor(noise).to(DEV)
        for label, tiles in (("params rows", None), ("tile image", image)):
            got, got_d = _act_direct(ag, s, nz, tiles), _act_direct(ag, s, None, tiles)
            torch.cuda.synchronize()
            _check_act(f"H={H} {label}", li, mu, val, noise, got, got_d)


@pytest.mark.parametrize("big", [False, True], ids=["B17", "past32"])
def test_act_c_pointwise(big):
    """ppo_act_c (H = 256 from a tile image) at B = 17 (16-row tiles, one ragged) and past its
    32-row threshold of 64 x CUs rows (ragged too)."""
    B = 64 * _cus() + 17 if big else 17
    for li in range(len(hc.LOG_STDS)):
        ag = _agent(4, 256, li)
        flat = flat_params(ag)[0]
        ws, image = _tile_image(4, 256, flat)
        mu, val, noise = _act_inputs(li, B)
        if not big:  # 17 rows: the tails of the table instead of its head
            j = np.argsort(-np.abs(T.z).max(1), kind="stable")[:B]
            mu, val = T.mu[j], T.val[j]
            sigma = np.exp(np.float32(hc.LOG_STDS[li]).astype(np.float64))
            noise = ((T.z[j].astype(np.float64) - mu) / sigma).astype(np.float32)
            noise[3], noise[16] = (5.5, -5.5), (-5.5, 5.5)
        s = torch.as_tensor(hc.selector_states(mu, val, 4)).to(DEV)
        nz = torch.as_tensor(noise).to(DEV)
        got, got_d = _act_direct(ag, s, nz, image), _act_direct(ag, s, None, image)
        torch.cuda.synchronize()
        _check_act(f"ppo_act_c B={B}", li, mu, val, noise, got, got_d)


# --------------------------------------------------------------------- acting and the update agree
def _step_on(ag, s, z, lp, adv, ret):
    """One fused forward/backward of `ag`'s weights over all rows; the metrics row."""
    B = s.shape[0]
    F = FusedPPO(ag, B, 1, use_graphs=False)
    idx = torch.arange(B, device=DEV)
    a = F._args(s, z, lp, adv, ret, idx.data_ptr())
    F.counters.zero_()
    F.sync_params(a)
    F._fwd_bwd(a)
    torch.cuda.synchronize()
    return F.metrics[0].double().cpu().numpy()


@pytest.mark.parametrize("S,H", [(4, 64), (4, 320), (4, 256), (5, 64)],
                         ids=["H64", "H320", "H256", "general"])
def test_round_trip_selector_is_exact(S, H):
    """Rows sampled by hwy_ppo_act on the selector network, tail rows included, go back unchanged
    into one step with the same parameters (S = 5: the general path, its fifth state column and
    weight column zero).  mu is exact in both kernels and the squash term is a function of z's
    bits, so acting's log-prob and the update's are the same number: KL exactly 0, clip count 0,
    and the policy term exactly -mean(adv) (adv in {+-1, +-0.5}: the mean is exact)."""
    B = 64
    for li in range(len(hc.LOG_STDS)):
        mu, val, noise = _act_inputs(li, B)
        act_ag = _agent(4, H, li)
        s4 = torch.as_tensor(hc.selector_states(mu, val, 4)).to(DEV)
        with torch.no_grad():
            _, z, lp, v = fused_act(act_ag, s4, noise=torch.as_tensor(noise).to(DEV))
        assert int((z.abs().amax(1) >= 5).sum()) >= 8
        ag = act_ag if S == 4 else _agent(S, H, li)
        s = s4 if S == 4 else torch.as_tensor(hc.selector_states(mu, val, S)).to(DEV)
        adv = torch.tensor([1.0, -1.0, 0.5, -0.5, 1.0, 0.5, 1.0], device=DEV).repeat(10)[:B].contiguous()
        m = _step_on(ag, s, z.contiguous(), lp.contiguous(), adv, v.contiguous())
        want = -float(adv.double().mean())
        print(f"\nHEAD round trip S={S} H={H} log_std {hc.LOG_STDS[li]}: kl {m[5]!r} clip {m[4]!r}"
              f" policy {m[0]!r} (-mean adv {want!r}) max |z| {float(z.abs().max()):.1f}")
        assert m[5] == 0.0 and m[4] == 0.0 and m[0] == want, m.tolist()


def _mu_bounds(ag, s):
    """mu and val of a random network in float64, and the per-row bound of an fp32 evaluation of
    mu in any order: e = gamma_(K+1) (|W| |x| + |b|) + |W| e_x layer by layer, as
    ppo_ref_util._fused_relu_masks propagates it."""
    m = copy.deepcopy(ag.actor_critic).double()
    x = s.double()
    e = torch.zeros_like(x)
    with torch.no_grad():
        def lin(layer, x, e, relu):
            W, b = layer.weight, layer.bias
            y = x @ W.T + b
            ey = _gamma(W.shape[1] + 1) * (x.abs() @ W.abs().T + b.abs()) + e @ W.abs().T
            return (y.clamp_min(0) if relu else y), ey

        h, e = lin(m.shared[0], x, e, True)
        h, e = lin(m.shared[2], h, e, True)
        a, ea = lin(m.actor_mean[0], h, e, True)
        mu, emu = lin(m.actor_mean[2], a, ea, False)
    return mu.cpu().numpy(), emu.cpu().numpy()


@pytest.mark.parametrize("H", [64, 256])
@pytest.mark.parametrize("log_std", [(-0.4, 0.3), (-2.0, 1.0)], ids=["ls0", "ls1"])
def test_round_trip_random_network_is_bounded(H, log_std):
    """The same round trip on an ordinary random network (CPU-initialised, S = 60, B = 512,
    unclamped noise): the two kernels' mu differ from float64's by at most e_mu each, so the
    update's log_ratio is at most twice the model's log-prob bound (fed dmu = e_mu) from 0; the
    KL is inside what that allows and no row is clipped."""
    from ppo.agent import PPOAgent

    S, B = 60, 512
    torch.manual_seed(0)
    ref = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=torch.device("cpu"), backend="torch")
    with torch.no_grad():
        ref.actor_critic.log_std.copy_(torch.tensor(log_std))
    g = torch.Generator().manual_seed(7919)
    s = torch.randn(B, S, generator=g).to(DEV).contiguous()
    noise = torch.randn(B, 2, generator=g).to(DEV).contiguous()
    ag = PPOAgent(S, 2, lr=3e-4, epochs=2, hidden_dim=H, device=DEV, use_graphs=False, backend="hip")
    ag.actor_critic.load_state_dict(ref.actor_critic.state_dict())
    with torch.no_grad():
        _, z, lp, v = fused_act(ag, s, noise=noise)
    tails = int((z.abs().amax(1) >= 3).sum())
    assert tails >= 10, tails
    adv = torch.randn(B, generator=g).to(DEV).contiguous()
    m = _step_on(ag, s, z.contiguous(), lp.contiguous(), adv, v.contiguous())
    mu, emu = _mu_bounds(ag, s)
    zz = z.double().cpu().numpy()
    _, e_lp, *_ = hm.logp_rows(mu, zz, np.float32(log_std), dmu=emu)
    x = 2.0 * e_lp + hm.U * np.abs(lp.double().cpu().numpy())
    # (expf(x) - 1) - x in fp32: expf's 2u and the two subtractions on top of the exact value
    row = (np.expm1(x) - x) + 3.0 * hm.U * np.exp(x) + 2.0 * hm.U * x
    bound = float(row.mean()) * (1.0 + _gamma(B))
    print(f"\nHEAD round trip random H={H} log_std {log_std}: kl {m[5]:.3e} bound {bound:.3e}"
          f" clip {m[4]:.0f}; {tails} rows with |z| >= 3, max |z| {np.abs(zz).max():.1f}")
    assert m[4] == 0.0
    assert abs(m[5]) <= bound
