"""Reference helpers of the fused PPO parity tests: agents and inputs, the float64 autograd
reference taking the fused step's own ReLU decisions, the gradient criterion (_check_grads), and
the CPU-drawn edge cases shared by test_ppo_edge_inputs.py (input conditions, no GPU) and
test_ppo_edges_gpu.py (the kernels against float64), and the general path's cases with their
split-K plans (test_ppo_general_inputs.py, test_ppo_general_gpu.py), and the host plan of the
fused path restated with the shapes of the memory tests (test_ppo_memory_inputs.py,
test_ppo_memory_gpu.py)."""

import copy

import torch

DEV = torch.device("cuda", 0)


def _agents(S, H, backend_b="hip", seed=0, **kw):
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    a = PPOAgent(S, 2, lr=3e-4, epochs=kw.get("epochs", 2), hidden_dim=H, device=DEV,
                 use_graphs=False, backend="torch")
    b = PPOAgent(S, 2, lr=3e-4, epochs=kw.get("epochs", 2), hidden_dim=H, device=DEV,
                 use_graphs=kw.get("graphs", False), backend=backend_b)
    b.actor_critic.load_state_dict(a.actor_critic.state_dict())
    with torch.no_grad():
        a.actor_critic.log_std.copy_(torch.tensor([-0.4, 0.3]))
        b.actor_critic.log_std.copy_(torch.tensor([-0.4, 0.3]))
    return a, b


def _data(n, S, agent, seed=1):
    g = torch.Generator(device=DEV).manual_seed(seed)
    s = torch.randn(n, S, device=DEV, generator=g)
    with torch.no_grad():
        _, z, lp, v = agent.actor_critic.act(s, generator=g)
    lp = lp + 0.05 * torch.randn(n, device=DEV, generator=g)  # ratios != 1, some clipped
    adv = torch.randn(n, device=DEV, generator=g)
    ret = v + torch.randn(n, device=DEV, generator=g)
    perm = torch.randperm(n, device=DEV, generator=g)
    return s, z.contiguous(), lp.contiguous(), adv, ret, perm


class _MaskMul(torch.nn.Module):
    """ReLU with its decisions given: z * mask."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, z):
        return z * self.mask


U32 = 2.0 ** -24  # binary32 unit roundoff


def _gamma(k):
    """Higham's gamma_k = k u / (1 - k u): the relative bound of any k-term fp32 sum/product
    evaluation order (MFMA accumulation included; fp32 products of fp32 inputs are exact)."""
    return k * U32 / (1.0 - k * U32)


def _fused_relu_masks(F, agent, s, idx, mb, H):
    """The fused step's own ReLU decisions for the four hidden layers, from its workspace rows
    (h1, h2 post-ReLU; dac, which is zero wherever [a1 | c1]'s ReLU is off), each checked
    against float64: a decision may differ from float64's only where the float64
    pre-activation z lies within the per-element fp32 error bound of that element,
    e = gamma_(K+1) (|W| |x| + |b|) + |W| e_x   (float64; K the fan-in, e_x the bound of the
    layer's input, propagated through the 1-Lipschitz ReLU; e_x = 0 for the states).
    Any fp32 evaluation order can land on either side of zero inside that bound and none can
    outside it.  Returns the masks and the number of such rounding-level flips."""
    import copy

    ws = F.workspace.view(torch.float32)  # carve order: h1, h2, ac, dac (256-B aligned)
    al = lambda k: (k + 63) // 64 * 64  # noqa: E731
    n = mb * H
    h1 = ws[0:n].view(mb, H).double()
    h2 = ws[al(n):al(n) + n].view(mb, H).double()
    o = 2 * al(n) + al(2 * n)
    dac = ws[o:o + 2 * n].view(mb, 2 * H).double()
    m = copy.deepcopy(agent.actor_critic).double()
    x = s.double()[idx]
    with torch.no_grad():
        W1, b1 = m.shared[0].weight, m.shared[0].bias
        W2, b2 = m.shared[2].weight, m.shared[2].bias
        Wa, ba = m.actor_mean[0].weight, m.actor_mean[0].bias
        Wc, bc = m.critic[0].weight, m.critic[0].bias
        z1 = x @ W1.T + b1
        e1 = _gamma(W1.shape[1] + 1) * (x.abs() @ W1.abs().T + b1.abs())
        a1 = z1.clamp_min(0)
        z2 = a1 @ W2.T + b2
        e2 = _gamma(H + 1) * (a1.abs() @ W2.abs().T + b2.abs()) + e1 @ W2.abs().T
        a2 = z2.clamp_min(0)
        za = a2 @ Wa.T + ba
        ea = _gamma(H + 1) * (a2.abs() @ Wa.abs().T + ba.abs()) + e2 @ Wa.abs().T
        zc = a2 @ Wc.T + bc
        ec = _gamma(H + 1) * (a2.abs() @ Wc.abs().T + bc.abs()) + e2 @ Wc.abs().T
    pre = {"z1": (z1, e1), "z2": (z2, e2), "za": (za, ea), "zc": (zc, ec)}
    ma = torch.where(dac[:, :H] != 0, 1.0, (za > 0).double())
    mc = torch.where(dac[:, H:] != 0, 1.0, (zc > 0).double())
    # rows whose actor / critic upstream gradient is nonzero: there dac == 0 means "ReLU off"
    live_a = (dac[:, :H] != 0).any(1, keepdim=True)
    live_c = (dac[:, H:] != 0).any(1, keepdim=True)
    ma = torch.where(live_a & (dac[:, :H] == 0), 0.0, ma)
    mc = torch.where(live_c & (dac[:, H:] == 0), 0.0, mc)
    masks = {"z1": (h1 > 0).double(), "z2": (h2 > 0).double(), "za": ma, "zc": mc}
    flips = 0
    for k, mk in masks.items():
        z, e = pre[k]
        diff = mk != (z > 0).double()
        flips += int(diff.sum())
        if diff.any():
            excess = (z[diff].abs() - e[diff]).max().item()
            assert excess <= 0.0, (k, int(diff.sum()), excess)
    return masks, flips


def _grad64(agent, s, z, lp, adv, ret, idx, masks=None):
    """The same minibatch loss and gradient (ppo/agent.py:216-248) in float64 autograd;
    `masks` (from _fused_relu_masks) replaces the four ReLUs by those decisions."""
    import copy

    import torch.nn.functional as Fn
    from torch.distributions import Normal

    ag = agent
    m = copy.deepcopy(ag.actor_critic).double()
    if masks is not None:
        m.shared[1], m.shared[3] = _MaskMul(masks["z1"]), _MaskMul(masks["z2"])
        m.actor_mean[1], m.critic[1] = _MaskMul(masks["za"]), _MaskMul(masks["zc"])
    s, z, lp, adv, ret = (t.double()[idx] for t in (s, z, lp, adv, ret))
    mean, std, v = m(s)
    dist = Normal(mean, std, validate_args=False)
    nlp = (dist.log_prob(z) - torch.log1p(-torch.tanh(z).pow(2) + 1e-6)).sum(-1)
    r = torch.exp(nlp - lp)
    loss = (-torch.min(r * adv, torch.clamp(r, 1 - ag.eps_clip, 1 + ag.eps_clip) * adv).mean()
            + ag.value_coef * Fn.mse_loss(v.squeeze(-1), ret)
            - ag.entropy_coef * dist.entropy().sum(-1).mean())
    loss.backward()
    return {n: p.grad for n, p in m.named_parameters()}


def _torch_grad(agent, s, z, lp, adv, ret, idx):
    from ppo.agent import _Learner

    L = _Learner(agent, s.shape[0], idx.numel(), 1, False)
    L.bind(s, z, lp, adv, ret)
    L.idx.copy_(idx)
    L._fwd_bwd()
    return L.flat_grad.clone(), L.metrics[0].clone()


def _check_grads(ga, gb, g64, msg=""):
    """Fused gradients (gb) against float64 autograd (g64) and torch fp32 (ga): elementwise
    agreement with float64 or with torch fp32 (whichever the fp32 rounding of the shape
    allows), and never further from float64 than torch fp32 is, up to rounding.  Returns the
    largest fused error relative to each parameter's gradient scale."""
    worst = 0.0
    for name, pa in ga.items():
        ref = g64[name]
        t32 = pa.grad.double()
        scale = max(ref.abs().max().item(), 1e-3)
        got = gb[name].grad.double()
        ok64 = torch.allclose(got, ref, rtol=1e-3, atol=2e-5 * scale)
        ok32 = torch.allclose(got, t32, rtol=1e-3, atol=2e-5 * scale)
        e_fused = (got - ref).abs().max().item()
        e_torch = (t32 - ref).abs().max().item()
        assert ok64 or ok32, (msg, name, e_fused, e_torch)
        assert e_fused <= 2 * e_torch + 2e-5 * scale, (msg, name, e_fused, e_torch)
        worst = max(worst, e_fused / scale)
    return worst


# ------------------------------------------------------------------ CPU-drawn edge cases
WIDTHS = (64, 128, 192, 256, 320, 384, 448, 512)
LOG_STDS = ((-0.4, 0.3), (-1.5, 0.5), (-2.0, 1.0))
COEFS = ((0.2, 0.5, 0.005), (0.1, 1.0, 0.02), (0.3, 0.25, 0.0))  # eps_clip, value, entropy
SIGMA = 0.25  # of the old_logp perturbation: 20-80 % of the rows clipped at eps_clip 0.1-0.3

# (S, H, B, LOG_STDS index, COEFS index, seed).  The seeds are the smallest at which the inputs
# meet every condition of test_ppo_edge_inputs.py.
GRAD_CASES = (
    # every width at 40 rows: 16 + 16 + 8 rows of tiles, one partial 64-row wgrad chunk
    (60, 64, 40, 0, 0, 0), (60, 128, 40, 1, 1, 0), (60, 192, 40, 2, 2, 0), (60, 256, 40, 2, 2, 0),
    (60, 320, 40, 0, 1, 0), (60, 384, 40, 0, 2, 0), (60, 448, 40, 1, 0, 0), (60, 512, 40, 2, 1, 0),
    # the two-deep weight ring (TW 5 / 7) with a padded W1 image
    (200, 320, 72, 1, 2, 0), (200, 448, 72, 2, 1, 1), (4, 320, 17, 2, 0, 0),
    (252, 448, 130, 0, 2, 3),
    # S edges: one padded 16-block, whole blocks, whole 64-column wgrad tiles, kMaxRowS
    (4, 64, 17, 1, 2, 0), (16, 128, 16, 2, 0, 0), (20, 256, 33, 0, 0, 0), (64, 192, 64, 0, 1, 0),
    (68, 384, 72, 1, 1, 1), (252, 512, 130, 0, 2, 3), (256, 64, 130, 2, 1, 0),
    (256, 128, 130, 1, 0, 0), (256, 256, 72, 1, 1, 0), (256, 512, 40, 2, 2, 1),
    # B edges: below / at / past one 16-row tile and one 64-row chunk; 130 = two 65-row slices
    (60, 256, 1, 0, 0, 0), (60, 256, 15, 1, 1, 0), (60, 256, 16, 2, 2, 0), (60, 256, 17, 0, 1, 0),
    (60, 256, 63, 1, 2, 0), (60, 256, 65, 2, 0, 0), (60, 256, 130, 0, 1, 5),
    # the general path through scalar gemm64 (S % 4 != 0); GENERAL_CASES below holds the rest
    (75, 128, 50, 1, 0, 0), (75, 320, 40, 1, 0, 0), (30, 64, 17, 2, 1, 0),
    # wide fused states (256 < S <= 1,024, S % 4 == 0): the row kernels' chunked first layer
    (260, 256, 72, 0, 2, 0), (300, 512, 130, 1, 1, 0),
)
# the GRAD_CASES shapes labelled general above: exactly these have no tile image
# (FusedPPO._tile_off is None), which test_edge_gradient_matches_autograd asserts
GRAD_GENERAL_SHAPES = frozenset({(75, 128, 50), (75, 320, 40), (30, 64, 17)})
_BY_SHAPE = {c[:3]: c for c in GRAD_CASES}
# the exact checks (zero signal, dead units) and the in-kernel gradient norm run at these
EXACT_CASES = tuple(_BY_SHAPE[k] for k in ((60, 320, 40), (200, 448, 72), (60, 256, 40),
                                           (75, 128, 50)))
NORM_CASES = tuple(_BY_SHAPE[k] for k in [(60, H, 40) for H in WIDTHS]
                   + [(200, 320, 72), (256, 128, 130), (60, 256, 130), (75, 128, 50)])
# acting: every width x S in {one padded block, the flagship, kMaxRowS} x B in {1, 17}, and the
# two-deep ring widths with a padded W1 image over more than one workgroup's rows
ACT_CASES = tuple((S, H, B) for H in WIDTHS for S in (4, 60, 256) for B in (1, 17)) + (
    (200, 320, 100), (200, 448, 100))


# ------------------------------------------------------------------ the general path
# Shapes outside the fused bound (S % 4 != 0 or S > 1,024): 11 gemm64 / gemm64v launches, ppo_head,
# split-K slabs, ppo_reduce and the flat ppo_adam (test_ppo_general_inputs.py: the conditions on
# the inputs and what each row reaches, without a GPU; test_ppo_general_gpu.py: the kernels).
# Same row format as GRAD_CASES; the seeds are the smallest at which the inputs meet every
# condition of test_ppo_general_inputs.py.  These have up to 1,000 rows, so they stay out of
# GRAD_CASES (16-row tiles at every CU count hold only up to 130).
GENERAL_CASES = (
    # ---- dW1 and the first layer through scalar gemm64 (S % 4 != 0)
    (1, 64, 17, 0, 1, 0),        # a single k in the first layer; dW1 has one column
    (33, 128, 40, 1, 2, 2),      # one live k in the second 32-deep K-step of the first layer
    (63, 192, 72, 2, 0, 0),      # dW1's 64-column tile, one column short of full
    (65, 256, 130, 0, 2, 0),     # dW1's second column tile holds one column
    (130, 320, 72, 1, 1, 1),     # S % 4 == 2, three column tiles of dW1
    (25, 64, 1000, 2, 1, 0),     # 32 slabs of 32 rows, the last holding 8: ppo_reduce sums 32
    (258, 512, 300, 1, 0, 0),    # dW1: scalar chunks of 64 (prefetch taken); vector 160 and 96
    (75, 512, 300, 0, 0, 0),     # the same plan at the five-feature width
    (130, 512, 1000, 2, 2, 1),   # chunks above 64 rows on all three weight gradients
    # ---- gemm64v with K = S / N = S and gathered operand rows (S > 1,024, S % 4 == 0)
    (1028, 64, 17, 2, 0, 0),     # 16 K-tiles and one float4; one partial chunk of 17 rows
    (1028, 256, 72, 1, 0, 0),    # ... and 16 whole column tiles of dW1 plus 4 columns
    (1088, 128, 130, 0, 1, 0),   # whole K-tiles and whole column tiles only
    (1100, 512, 130, 1, 2, 0),   # S % 64 == 12; dW1 in one chunk of 160 rows
    (1028, 512, 300, 2, 1, 0),   # dW1 in one chunk of 320 rows: five gathered K-tiles, prefetched
    (1028, 384, 520, 0, 2, 0),   # odd H / 64; chunks of 192 / 96 / 288 rows
)
_GENERAL_BY_SHAPE = {c[:3]: c for c in GENERAL_CASES}
# the exact checks (zero signal, dead units): every split-K GEMM with more than one K-tile per
# chunk, scalar and vector dW1
GENERAL_EXACT_CASES = tuple(_GENERAL_BY_SHAPE[k] for k in ((258, 512, 300), (1028, 256, 72)))
# the in-kernel norm: every row whose float64 gradient norm is above 0.5, so that max_grad_norm
# 0.5 clips (the others: 0.24 - 0.50); ppo_reduce's norm partials at nred up to 5,287
GENERAL_NORM_CASES = tuple(_GENERAL_BY_SHAPE[k] for k in (
    (1, 64, 17), (33, 128, 40), (63, 192, 72), (130, 320, 72), (258, 512, 300), (1028, 64, 17),
    (1028, 256, 72), (1088, 128, 130), (1100, 512, 130), (1028, 512, 300)))

K_STEP, V_K = 32, 64  # K-tile depth of gemm64 (kKStep) and of gemm64v (kVK)


def split_for(tiles, K):
    """csrc/ppo_kernels.hip split_for: workgroups along K for `tiles` output tiles."""
    return min(max(1, 256 // max(tiles, 1)), -(-K // K_STEP))


def chunk_for(K, split):
    """csrc/ppo_kernels.hip chunk_for: rows per split-K chunk, whole 32-deep K-steps."""
    return -(-(-(-K // split)) // K_STEP) * K_STEP


def general_plan(S, H, B):
    """carve()'s split-K plan of the general path's three weight-gradient GEMMs (K = B):
    'ac' d[Wa1;Wc1] (2H x H), '2' dW2 (H x H), '1' dW1 (H x S).  Per GEMM: `slabs`, `kchunk`,
    `lens` (rows of each chunk), `vector` (launch_gemm takes gemm64v: M and N multiples of 4,
    which the H x H ones always are and dW1 is when S % 4 == 0) and `ktile`, that kernel's
    K-tile."""
    t = lambda n: -(-n // 64)  # noqa: E731
    out = {}
    for name, tiles, vec in (("ac", t(2 * H) * t(H), True), ("2", t(H) * t(H), True),
                             ("1", t(H) * t(S), S % 4 == 0)):
        c = chunk_for(B, split_for(tiles, B))
        s = -(-B // c)
        out[name] = dict(slabs=s, kchunk=c, lens=[min(c, B - z * c) for z in range(s)],
                         vector=vec, ktile=V_K if vec else K_STEP)
    return out


# ------------------------------------------------------------------ the host plan, restated
# What csrc/ppo_kernels.hip decides on the host for a shape and a chip (rows_tile, fused_ok,
# rows_blocks, tile_geom, carve with its balanced weight-gradient partition, hwy_ppo_act's kernel
# choice), restated for the memory tests: test_ppo_memory_inputs.py checks without a GPU that
# MEMORY_* below reach every addressing path at the full MI355X (256 CUs, 8 XCDs) and that
# workspace_sizes adds up to hwy_ppo_workspace_bytes; test_ppo_memory_gpu.py asserts the same
# with the device's own CU count.
MAX_ROW_S, MAX_FUSED_S = 256, 1024   # kMaxRowS, kMaxFusedS
WG_TM, WG_TN = 128, 64               # ppo_wgrad's output tile
WG_PART = WG_TM * WG_TN + WG_TM      # kWgPart: floats per partial tile (+ bias sums)
HEAD_ROWS, RED_THREADS = 16, 256     # kHeadRows, kRedThreads
FULL_CHIP = (256, 8)                 # CUs, XCDs of an unpartitioned MI355X


def fused_ok(S, H):
    return S % 4 == 0 and S <= MAX_FUSED_S and H % 64 == 0 and 64 <= H <= 512


def rows_tile(B, H, S, cus):
    """Minibatch rows per ppo_rows workgroup."""
    if H > 256 or S > MAX_ROW_S:
        return 16
    if H == 256 and B >= 64 * cus:
        return 64
    return 32 if B >= 32 * cus else 16


def row_waves(H):
    """Waves of the row and act kernels: 8 when H / 64 is even, else 4."""
    return 8 if (H // 64) % 2 == 0 else 4


def ring_depth(H):
    return 4 if H // row_waves(H) // 16 <= 4 else 2


def rows_blocks(S, H):
    """(sb, hb): 16-deep k blocks of W1's image and of an H x H image, whole ring groups."""
    D = ring_depth(H)
    return -(-(-(-S // 16)) // D) * D, -(-(H // 16) // D) * D


def tile_image_floats(S, H):
    """TileGeom.total: W1's forward image and six H x H images in 1-KB blocks."""
    sb, hb = rows_blocks(S, H)
    g = H // 16
    return g * sb * 256 + 6 * g * hb * 256


def ppo_numel(S, H):
    return H * S + H + 3 * (H * H + H) + 2 * H + 2 + 2 + H + 1


def wgrad_plan(S, H, B, cus, xcds, fill=1.5):
    """carve()'s ppo_wgrad partition: tiles, row slices per tile (split) and whether the
    balanced partition (two partial-tile slots) is on."""
    import math

    tmh, tnh = -(-H // WG_TM), -(-H // WG_TN)
    tac, t2, t1 = -(-2 * H // WG_TM) * tnh, tmh * tnh, tmh * -(-S // WG_TN)
    ntile, nh = tac + t2 + t1, (3 * H + 9 + 63) // 64

    def plan(sp):
        P, nck = cus // sp, (-(-B // sp) + 63) // 64
        q = dict(split=sp, bal=0, wm=0, tpe=0, cost=nck)
        if ntile >= 16 and P - ntile >= 2 and nck >= 16:
            E = P - ntile
            tpe = -(-ntile // E)
            m = math.ceil(tpe * (nck + fill) / (1.0 + tpe))
            if m < nck:
                q.update(bal=1, wm=m, tpe=tpe, cost=m)
        return q

    cap = max(1, min(xcds, 8, cus // ntile, (B + 63) // 64))
    best = plan(1)
    for sp in range(cap, 0, -1):
        if xcds % sp == 0:
            best = plan(sp)
            break
    for sp in range(2, min(8, max(1, (B + 63) // 64)) + 1):
        if xcds % sp == 0:
            continue
        q = plan(sp)
        if q["bal"] and q["cost"] < 0.85 * best["cost"] and (not best["bal"] or q["cost"] < best["cost"]):
            best = q
    best.update(ntile=ntile, nh=nh, nslot=2 if best["bal"] else 1,
                grid=best["split"] * (cus // best["split"]) if best["bal"]
                else ntile * best["split"] + nh)
    return best


WORK_REGIONS = ("h1", "h2", "ac", "dac", "dh2", "dh1", "head_part", "slab_ac", "bias_ac", "slab_2",
                "bias_2", "slab_1", "bias_1", "norm_part", "wg_slab", "xg", "wtile")


def workspace_sizes(S, H, B, cus=FULL_CHIP[0], xcds=FULL_CHIP[1]):
    """carve()'s 17 sub-buffers in floats, in WORK_REGIONS order, before the rounding of each to
    64 floats.  All of them are float arrays (struct Work): the workspace holds no address."""
    fused = fused_ok(S, H)
    g = general_plan(S, H, B)
    sa, s2, s1 = (0, 0, 0) if fused else (g["ac"]["slabs"], g["2"]["slabs"], g["1"]["slabs"])
    nhead, HP = -(-B // HEAD_ROWS), 3 * H + 16
    nred = -(-ppo_numel(S, H) // RED_THREADS)
    w = wgrad_plan(S, H, B, cus, xcds)
    n1 = -(-B // rows_tile(B, H, S, cus))
    nred2 = w["nh"] + w["ntile"] * (WG_TM * WG_TN // 1024)
    return [B * H, B * H, 2 * B * H, 2 * B * H, B * H, B * H,
            (max(nhead, n1) if fused else nhead) * HP,
            sa * 2 * H * H, sa * 2 * H, s2 * H * H, s2 * H, s1 * H * S, s1 * H,
            max(nred, nred2) if fused else nred,
            w["ntile"] * w["split"] * w["nslot"] * WG_PART if fused else 0,
            B * S if fused else 0, tile_image_floats(S, H) if fused else 0]


def workspace_floats(S, H, B, cus=FULL_CHIP[0], xcds=FULL_CHIP[1]):
    return sum(-(-n // 64) * 64 for n in workspace_sizes(S, H, B, cus, xcds))


def act_kernel(S, H, B, tiles, cus):
    """The kernel hwy_ppo_act / hwy_ppo_value_masked launch: (body, rows per workgroup)."""
    if tiles and H == 256:
        return ("ppo_act_c", 32 if S <= MAX_ROW_S and B >= 64 * cus else 16)
    return ("ppo_act_tiles" if tiles else "ppo_act_params", 16)


def memory_paths(S, H, B, cus=FULL_CHIP[0], xcds=FULL_CHIP[1]):
    """The addressing paths the minibatch step of (S, H, B) takes on a chip, as tags."""
    if not fused_ok(S, H):
        g = general_plan(S, H, B)
        t = {"general", "adam-flat", "gemm-vector" if g["1"]["vector"] else "gemm-scalar"}
        if any(p["slabs"] > 1 for p in g.values()):
            t.add("split-k")
        if any(p["lens"][-1] != p["kchunk"] for p in g.values()):
            t.add("ragged-slab")
        return t
    rt, w = rows_tile(B, H, S, cus), wgrad_plan(S, H, B, cus, xcds)
    sb, _ = rows_blocks(S, H)
    t = {f"rows{rt}", f"waves{row_waves(H)}", f"ring{ring_depth(H)}", "adam-tiles"}
    if S > MAX_ROW_S:
        t.add("wide")
    if S == MAX_FUSED_S and H == 512:
        t.add("widest")
    if B % rt:
        t.add("ragged-tile")
    if B % 64:
        t.add("ragged-chunk")
    if S % 16:
        t.add("w1-pad-columns")
    if 16 * sb - S >= 16:
        t.add("w1-pad-block")
    if w["split"] > 1:
        t.add("slices")
    if w["bal"]:
        t.add("balanced")
    return t


# (B, S, H) of the memory tests: the smallest shapes reaching each path, with the tags each must
# carry (test_ppo_memory_inputs.py).  The two large ones depend on the chip's CU count.
MEMORY_FUSED = (
    ((1, 4, 64), {"rows16", "waves4", "ragged-tile", "w1-pad-columns"}),
    ((17, 60, 64), {"rows16", "ragged-tile", "ragged-chunk"}),
    ((100, 60, 128), {"rows16", "waves8", "ragged-tile", "ragged-chunk", "slices"}),
    ((129, 200, 320), {"ring2", "w1-pad-block", "waves4", "slices"}),
    ((65, 120, 192), {"waves4", "ring4", "ragged-chunk"}),
    ((48, 60, 448), {"waves4", "ring2"}),
    ((72, 260, 256), {"wide", "rows16", "waves8"}),
    ((64, 1024, 512), {"wide", "widest", "ring4", "waves8"}),
)
MEMORY_GENERAL = (
    ((33, 30, 64), {"general", "gemm-scalar", "split-k", "ragged-slab", "adam-flat"}),
    ((64, 75, 128), {"general", "gemm-scalar", "split-k"}),
    ((16, 1028, 64), {"general", "gemm-vector", "adam-flat"}),
)


def memory_large(cus):
    """The 32-row tiles and the 64-row tiles with the balanced partition: B just past each
    threshold, ragged in its last tile."""
    return (((32 * cus + 5, 60, 128), {"rows32", "ragged-tile", "slices"}),
            ((64 * cus + 37, 60, 256), {"rows64", "ragged-tile", "balanced", "slices"}))


# acting (B, S, H): the step's fused shapes, and ppo_act_c at a ragged B in both tile heights
def memory_act(cus):
    return tuple(c for c, _ in MEMORY_FUSED) + ((1000, 120, 256), (64 * cus + 5, 60, 256))


MEMORY_PATHS = frozenset({
    "rows16", "rows32", "rows64", "waves4", "waves8", "ring2", "ring4", "wide", "widest",
    "ragged-tile", "ragged-chunk", "w1-pad-columns", "w1-pad-block", "slices", "balanced",
    "adam-tiles", "general", "gemm-scalar", "gemm-vector", "split-k", "ragged-slab", "adam-flat"})


def case_id(c):
    return "-".join(str(x) for x in c[:3])


def case_kwargs(c):
    """edge_case's keyword arguments of a GRAD_CASES row."""
    eps, vc, ec = COEFS[c[4]]
    return dict(log_std=LOG_STDS[c[3]], sigma=SIGMA, eps_clip=eps, value_coef=vc,
                entropy_coef=ec, seed=c[5])


def dead_columns(H):
    """Hidden units the dead-unit check switches off: the first, the first of the row kernels'
    second wave (H / NW columns per wave, 8 waves when H / 64 is even, else 4), the last."""
    return (0, H // (8 if (H // 64) % 2 == 0 else 4), H - 1)


def edge_case(S, H, B, *, log_std, sigma, eps_clip, value_coef, entropy_coef, seed, device=DEV,
              dead=()):
    """A minibatch of B rows out of n = 2B, drawn with CPU generators only and then moved to
    `device`, so a machine with a GPU and one without see the same bits: the weights come from
    PPOAgent's CPU initialisation, and whatever passes through the model (the sample z, old_logp,
    the value in ret) is computed in float64 and rounded to fp32 once, which does not depend on
    the machine's fp32 GEMM.  z is sampled from the policy and clamped to [-3, 3]
    (log1p(-tanh(z)^2 + 1e-6) is ill-conditioned in fp32 beyond), old_logp is
    ActorCritic.evaluate of the clamped z plus sigma * randn.  `dead`: units of the first hidden
    layer whose bias is set to -1e3 before anything is drawn.
    Returns (a, b, s, z, lp, adv, ret, idx): the torch-backend and hip-backend agents, both with
    the given log_std and coefficients, the n-row inputs, and the minibatch's row indices."""
    from ppo.agent import PPOAgent

    def agent(dev, backend):
        ag = PPOAgent(S, 2, lr=3e-4, epochs=2, hidden_dim=H, device=dev, use_graphs=False,
                      backend=backend)
        ag.eps_clip, ag.value_coef, ag.entropy_coef = eps_clip, value_coef, entropy_coef
        return ag

    torch.manual_seed(seed)
    ref = agent(torch.device("cpu"), "torch")
    with torch.no_grad():
        ref.actor_critic.log_std.copy_(torch.tensor(log_std))
        for j in dead:
            ref.actor_critic.shared[0].bias[j] = -1e3
    g = torch.Generator().manual_seed(seed + 7919)
    n = 2 * B
    s = torch.randn(n, S, generator=g)
    m64 = copy.deepcopy(ref.actor_critic).double()
    with torch.no_grad():
        mean, std, v = m64(s.double())
        z = (mean + std * torch.randn(n, 2, generator=g).double()).clamp(-3.0, 3.0).float()
        lp, _, _ = m64.evaluate(s.double(), torch.tanh(z.double()), z.double())
        lp = (lp + sigma * torch.randn(n, generator=g).double()).float()
        adv = torch.randn(n, generator=g)
        ret = (v.squeeze(-1) + torch.randn(n, generator=g).double()).float()
        perm = torch.randperm(n, generator=g)
    a, b = agent(device, "torch"), agent(device, "hip")
    for ag in (a, b):
        ag.actor_critic.load_state_dict(ref.actor_critic.state_dict())
    s, z, lp, adv, ret, perm = (t.to(device).contiguous() for t in (s, z, lp, adv, ret, perm))
    return a, b, s, z, lp, adv, ret, perm[:B].contiguous()


def _ratio64(agent, s, z, lp, idx):
    """The minibatch rows' probability ratios in float64."""
    m = copy.deepcopy(agent.actor_critic).double()
    s, z, lp = (t.double()[idx] for t in (s, z, lp))
    with torch.no_grad():
        nlp, _, _ = m.evaluate(s, torch.tanh(z), z)
    return torch.exp(nlp - lp)


def _grads_agree(ga, g64):
    """_check_grads' elementwise criterion for torch fp32 (ga: named parameters with .grad)
    against float64: rtol 1e-3, atol 2e-5 * scale.  Returns the worst error relative to scale."""
    worst = 0.0
    for name, pa in ga.items():
        ref = g64[name]
        scale = max(ref.abs().max().item(), 1e-3)
        got = pa.grad.double()
        err = (got - ref).abs().max().item()
        assert torch.allclose(got, ref, rtol=1e-3, atol=2e-5 * scale), (name, err, scale)
        worst = max(worst, err / scale)
    return worst


def act_case(S, H, B, seed=0, device=DEV):
    """Acting inputs drawn on the CPU: the hip-backend agent (CPU-initialised weights, log_std
    (-0.4, 0.3)), B states and the sampling noise clamped to [-2, 2], which keeps |z| <= 3
    (std <= 1.35) without excluding any row."""
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    ref = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=torch.device("cpu"), backend="torch")
    with torch.no_grad():
        ref.actor_critic.log_std.copy_(torch.tensor([-0.4, 0.3]))
    g = torch.Generator().manual_seed(seed + 7919)
    s = torch.randn(B, S, generator=g)
    noise = torch.randn(B, 2, generator=g).clamp(-2.0, 2.0)
    b = PPOAgent(S, 2, lr=3e-4, hidden_dim=H, device=device, use_graphs=False, backend="hip")
    b.actor_critic.load_state_dict(ref.actor_critic.state_dict())
    return b, s.to(device).contiguous(), noise.to(device).contiguous()


def act64(agent, s, noise):
    """ActorCritic.act on the float64 copy of the model: (sampled with `noise`, deterministic),
    each (action, pre_tanh, log_prob, value)."""
    m = copy.deepcopy(agent.actor_critic).double()
    dbl = lambda out: tuple(t.double() for t in out)  # noqa: E731  (act's zero log-prob is fp32)
    return (dbl(m.act(s.double(), noise=noise.double())),
            dbl(m.act(s.double(), deterministic=True)))
