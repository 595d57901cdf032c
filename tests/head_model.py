"""A float64 model of one row of the PPO loss head and of action sampling, with a forward-error
bound for an fp32 evaluation of every output.  Plain numpy; it shares no code with the kernels
(csrc/ppo_rows_body.inc, ppo_head, ppo_act_body.inc, ppo_act_c_body.inc) or with ppo/agent.py.

Per row the head takes mu[2], val (the network's outputs), z[2] (the stored pre-tanh action),
old_logp, adv, ret; per case log_std[2], eps_clip, value_coef, entropy_coef and the minibatch
size B.  Every input is taken as the exact real number its fp32 holds.

    logp      = sum_i  -(z_i - mu_i)^2 / (2 var_i) - log_std_i - log sqrt(2 pi) - q(z_i)
    q(z)      = log(1 - tanh(z)^2 + 1e-6),  1 - tanh^2 = 4 e^{-2|z|} / (1 + e^{-2|z|})^2
    ratio     = exp(logp - old_logp),  kl = (ratio - 1) - log_ratio,  clip = |ratio - 1| > eps
    policy    = -min(ratio adv, clamp(ratio, 1 - eps, 1 + eps) adv),  value = (val - ret)^2
    dlogp     = -(adv / B) wsel ratio,  wsel from torch's min / clamp backward (ties split evenly)
    dmu_i     = dlogp (z_i - mu_i) / var_i,  dls_i = dlogp ((z_i - mu_i)^2 / var_i - 1)
    dv        = value_coef 2 (val - ret) / B

Bounds.  u = 2^-24 per arithmetic operation, 2u for a library function (exp, log: 1 ulp).  The
squash term's bound is K u / u(z), u(z) = 1 - tanh(z)^2 + 1e-6, K = 8: an absolute error of
K u in the argument of the logarithm (tanh a few ulp off, its square, the sum), below the
1e-6 / u = 16.8 at which the model could no longer see the 1e-6.  The gaussian terms' bounds
follow their operation counts, and everything downstream propagates them to first order with the
exact expm1 for the ratio.  `dmu` / `dval` are absolute bounds of mu and val themselves (0 when
the network passes them through exactly).

A row is `undetermined` when its float64 ratio lies within its own bound of 1 - eps or 1 + eps,
or when s1 == s2 versus not depends on an error of that size: an fp32 evaluation may then take
either branch, and no pointwise comparison applies.  The bound is taken as the interval
[ratio e^-e, ratio e^e] of the log_ratio's bound e: where both |z| saturate, e is near 1 and
the symmetric ratio (e^e - 1) would reach below zero.

`mut` names one deliberate mistake (MUTATIONS); tests use it to show that a check can fail."""

import numpy as np

U = 2.0 ** -24
K_SQUASH = 8.0
SQUASH_EPS = 1e-6
LOG_SQRT_2PI = 0.5 * np.log(2.0 * np.pi)

MUTATIONS = (
    "eps_dropped",        # 1e-6 dropped
    "eps_in_square",      # 1 - (|tanh| - 1e-6)^2
    "log_sqrt_2pi_1pct",  # LOG_SQRT_2PI off by 1 %
    "var_for_2var",       # d^2 / var in the log-prob
    "clip_ge",            # clip count with >=
    "tie_full",           # a tie passes gradient 1 to each side instead of 1/2
    "inr_ignored",        # the s1 > s2 branch passes the gradient whatever the clamp did
    "kl_neg_log_ratio",   # KL as -log_ratio
    "dls_no_minus_1",     # dlog_std without the - 1
    "dv_no_2",            # dv without the factor 2
    "entropy_sign",       # the entropy term added to the loss
)


def one_minus_tanh2(z):
    """1 - tanh(z)^2, relative error a few 2^-53 at any z (no cancellation)."""
    e = np.exp(-2.0 * np.abs(z))
    return 4.0 * e / (1.0 + e) ** 2


def squash_u(z):
    """u(z) = 1 - tanh(z)^2 + 1e-6, the argument of the correction's logarithm."""
    return one_minus_tanh2(z) + SQUASH_EPS


def squash(z, mut=None, K=K_SQUASH):
    """(q, bound): the correction log(u(z)) and K u / u(z)."""
    w = one_minus_tanh2(z)
    if mut == "eps_dropped":
        arg = w
    elif mut == "eps_in_square":
        t = np.sqrt(np.maximum(1.0 - w, 0.0))  # |tanh|
        arg = w + 2.0 * SQUASH_EPS * t - SQUASH_EPS ** 2
    else:
        arg = w + SQUASH_EPS
    return np.log(arg), K * U / squash_u(z)


def gamma(k):
    return k * U / (1.0 - k * U)


def _pow2(B):
    return B & (B - 1) == 0


class Rows:
    """v[name], e[name]: value and fp32 forward-error bound per row; und: undetermined rows."""

    def __init__(self):
        self.v, self.e, self.und = {}, {}, None

    def put(self, name, v, e):
        self.v[name], self.e[name] = v, e


def logp_rows(mu, z, log_std, dmu=0.0, mut=None, K=K_SQUASH):
    """The squashed Gaussian's log-prob of z[n, 2] under mean mu[n, 2] and log_std ([2] or
    [n, 2]): (logp, bound, d, e_d, var, e_dd)."""
    mu, z = np.asarray(mu, np.float64), np.asarray(z, np.float64)
    ls = np.broadcast_to(np.asarray(log_std, np.float64), mu.shape)
    var = np.exp(ls) ** 2
    d = z - mu
    e_d = U * np.abs(d) + dmu
    e_dd = 2.0 * np.abs(d) * e_d + e_d ** 2 + U * d * d
    g = d * d / (var if mut == "var_for_2var" else 2.0 * var)
    # var = expf(ls)^2: 2u of expf twice and the product; one more for 2 var's quotient
    e_g = e_dd / (2.0 * var) + 7.0 * U * g
    C = LOG_SQRT_2PI * (1.01 if mut == "log_sqrt_2pi_1pct" else 1.0)
    lp = -g - ls - C
    # logf(expf(ls)): expf's 2u relative is 2u absolute in the logarithm, logf's own 2u |ls|
    e_lsc = 3.0 * U * (1.0 + np.abs(ls))
    e_lp = e_g + e_lsc + U * LOG_SQRT_2PI + U * (np.abs(g + ls) + np.abs(lp))
    q, e_q = squash(z, mut, K)
    term = lp - q
    logp = term.sum(-1)
    e = (e_lp + e_q).sum(-1) + U * (np.abs(term).sum(-1) + np.abs(logp))
    return logp, e, d, e_d, var, e_dd


def head_rows(mu, val, z, old_logp, adv, ret, log_std, eps_clip, value_coef, entropy_coef, B,
              dmu=0.0, dval=0.0, mut=None, K=K_SQUASH):
    """Every per-row output of the loss head for n rows of a minibatch of B rows."""
    f = lambda x: np.asarray(x, np.float64)  # noqa: E731
    val, old, adv, ret = f(val), f(old_logp), f(adv), f(ret)
    eps = float(eps_clip)
    R = Rows()
    logp, e_logp, d, e_d, var, e_dd = logp_rows(mu, z, log_std, dmu, mut, K)
    R.put("logp", logp, e_logp)
    lr = logp - old
    e_lr = e_logp + U * np.abs(lr)
    R.put("log_ratio", lr, e_lr)
    ratio = np.exp(lr)
    e_ratio = ratio * (np.expm1(e_lr) + 3.0 * U)
    R.put("ratio", ratio, e_ratio)
    lo, hi = 1.0 - eps, 1.0 + eps
    inr = ((ratio >= lo) & (ratio <= hi)).astype(np.float64)
    # the ratios an fp32 evaluation can give: the bound of log_ratio through exp, as an interval
    # (below the ratio it ends at ratio e^-e, above zero however wide e is); lo, hi and
    # ratio - 1 are themselves rounded
    r_lo = ratio * np.exp(-e_lr) * (1.0 - 3.0 * U) - 4.0 * U
    r_hi = ratio + e_ratio + 4.0 * U
    und = ((r_lo <= lo) & (lo <= r_hi)) | ((r_lo <= hi) & (hi <= r_hi))
    dev = np.abs(ratio - 1.0)
    clip = (dev >= eps if mut == "clip_ge" else dev > eps).astype(np.float64)
    R.put("clip", clip, np.zeros_like(clip))
    s1, s2 = ratio * adv, np.clip(ratio, lo, hi) * adv
    lt, gt, tie = s1 < s2, s1 > s2, s1 == s2
    # s1 == s2 versus not: a clamped ratio differs from its bound by more than its interval
    # (above), so only the products' own roundings could still make them equal
    und |= (inr == 0) & (adv != 0) & (np.abs(s1 - s2) <= 4.0 * U * (np.abs(s1) + np.abs(s2)))
    w_gt = 1.0 if mut == "inr_ignored" else inr
    w_tie = (1.0 + inr) if mut == "tie_full" else 0.5 * (1.0 + inr)
    wsel = np.where(lt, 1.0, np.where(gt, w_gt, w_tie))
    R.v["wsel"], R.v["inr"] = wsel, inr
    R.v["branch"] = np.where(lt, 0, np.where(gt, 1, 2))
    pol = -np.minimum(s1, s2)
    e_sel = np.where(pol == -s1, e_ratio, 2.0 * U)
    R.put("policy", pol, e_sel * np.abs(adv) + U * np.abs(pol))
    kl = -lr if mut == "kl_neg_log_ratio" else (ratio - 1.0) - lr
    R.put("kl", kl, e_ratio + U * np.abs(ratio - 1.0) + e_lr + U * np.abs(kl))
    dvr = val - ret
    e_dvr = U * np.abs(dvr) + dval
    R.put("value", dvr * dvr, 2.0 * np.abs(dvr) * e_dvr + e_dvr ** 2 + U * dvr * dvr)
    invB = 1.0 / B
    rB = 0.0 if _pow2(B) else U
    dlogp = -invB * adv * wsel * ratio
    e_dlogp = np.abs(adv) * wsel * e_ratio * invB + (4.0 * U + rB) * np.abs(dlogp)
    R.put("dlogp", dlogp, e_dlogp)
    dl, el = dlogp[:, None], e_dlogp[:, None]
    dmu_ = dl * d / var
    R.put("dmu", dmu_, el * np.abs(d) / var + np.abs(dl) * e_d / var + 16.0 * U * np.abs(dmu_))
    t = d * d / var
    e_t = e_dd / var + 7.0 * U * t
    inner = t if mut == "dls_no_minus_1" else t - 1.0
    # autograd reaches the - 1 through log(exp(log_std)): 1 to a few roundings
    e_inner = e_t + 4.0 * U * (t + 1.0)
    dls = dl * inner
    R.put("dls", dls, el * np.abs(inner) + np.abs(dl) * e_inner + 8.0 * U * np.abs(dls))
    vc = float(value_coef)
    dv = vc * (1.0 if mut == "dv_no_2" else 2.0) * dvr * invB
    R.put("dv", dv, vc * 2.0 * invB * e_dvr + (4.0 * U + rB) * np.abs(dv))
    R.und = und
    R.B, R.coefs, R.mut = B, (eps, vc, float(entropy_coef)), mut
    R.log_std = np.asarray(log_std, np.float64)
    return R


def _sum(v, e, axis=0):
    """An fp32 sum of the terms in any order: (sum, sum of the bounds + gamma_(n-1) sum |v|),
    n the number of nonzero terms (adding an exact zero rounds nothing)."""
    n = int(np.max(np.count_nonzero(v, axis=axis))) if v.size else 0
    return v.sum(axis), e.sum(axis) + gamma(max(n - 1, 0)) * np.abs(v).sum(axis)


def minibatch(R):
    """What one step over exactly these B rows leaves in the public buffers: the metrics row
    (policy_loss, value_loss, entropy, loss, clip count, approx_kl) and the gradients of
    actor_mean.2.bias [2], critic.2.bias and log_std [2], each (value, bound)."""
    B = R.B
    assert R.v["logp"].shape[0] == B
    eps, vc, ec = R.coefs
    invB = 1.0 / B
    rB = U if _pow2(B) else 2.0 * U  # the product with 1/B, and 1/B's own rounding
    out = {}

    def mean(name):
        s, e = _sum(R.v[name], R.e[name])
        return s * invB, e * invB + rB * abs(s * invB)

    out["policy_loss"] = mean("policy")
    out["value_loss"] = mean("value")
    out["approx_kl"] = mean("kl")
    out["clip"] = (R.v["clip"].sum(), 0.0)
    ls = np.broadcast_to(R.log_std, (2,)) if R.log_std.ndim == 1 else R.log_std[0]
    ent = float((0.5 + LOG_SQRT_2PI + ls).sum())
    e_ent = float((3.0 * U * (1.0 + np.abs(ls))).sum()) + 4.0 * U * (abs(ent) + 2.0 * (0.5 + LOG_SQRT_2PI))
    out["entropy"] = (ent, e_ent)
    p, v = out["policy_loss"], out["value_loss"]
    sgn = 1.0 if R.mut == "entropy_sign" else -1.0
    loss = p[0] + vc * v[0] + sgn * ec * ent
    out["loss"] = (loss, p[1] + vc * v[1] + ec * e_ent
                   + 4.0 * U * (abs(p[0]) + vc * abs(v[0]) + ec * abs(ent) + abs(loss)))
    out["g_ba2"] = _sum(R.v["dmu"], R.e["dmu"])
    out["g_bc2"] = _sum(R.v["dv"], R.e["dv"])
    s, e = _sum(R.v["dls"], R.e["dls"])
    g = s + sgn * ec  # d(-ec mean entropy) / d log_std = -ec
    # the kernels subtract ec once; autograd sums B terms of ec / B
    out["g_ls"] = (g, e + gamma(B + 1) * ec + U * np.abs(g))
    return out


METRIC_ORDER = ("policy_loss", "value_loss", "entropy", "loss", "clip", "approx_kl")


def flat_outputs(mb):
    """minibatch()'s outputs as two vectors of 11: the six metrics, g_ba2[2], g_bc2, g_ls[2]."""
    v = [mb[k][0] for k in METRIC_ORDER] + list(mb["g_ba2"][0]) + [mb["g_bc2"][0]] + list(mb["g_ls"][0])
    e = [mb[k][1] for k in METRIC_ORDER] + list(mb["g_ba2"][1]) + [mb["g_bc2"][1]] + list(mb["g_ls"][1])
    return np.asarray(v, np.float64), np.asarray(e, np.float64)


OUTPUT_NAMES = METRIC_ORDER + ("g_ba2[0]", "g_ba2[1]", "g_bc2", "g_ls[0]", "g_ls[1]")


# ------------------------------------------------------------------------------------ acting
def act_rows(mu, noise, log_std, scale=None):
    """Sampling: z = mu + exp(log_std) noise and its bound of 2 roundings (the product and the
    sum); action = tanh(z).  `scale`: the fp32 scale to use for exp(log_std) (scale_candidates)."""
    mu, noise = np.asarray(mu, np.float64), np.asarray(noise, np.float64)
    sigma = np.exp(np.asarray(log_std, np.float64)) if scale is None else np.asarray(scale, np.float64)
    sn = sigma * noise
    z = mu + sn
    return z, U * (np.abs(sn) + np.abs(z)), np.tanh(z)


def scale_candidates(log_std):
    """The fp32 values a 1-ulp expf can return for one log_std: exp correctly rounded and its
    two neighbours.  The scale is an fp32 number in the reference (log_std.exp()) as in the
    kernels, so "2 roundings" of the sample count from it, not from the real exp."""
    c = np.float32(np.exp(np.float64(log_std)))
    return (float(c), float(np.nextafter(c, np.float32(0))), float(np.nextafter(c, np.float32(np.inf))))


def act_logp(mu, z, log_std, mut=None, K=K_SQUASH):
    """Acting's log-prob as a function of the z it stored: the head's logp of the same z."""
    logp, e, *_ = logp_rows(mu, z, log_std, 0.0, mut, K)
    return logp, e


def ulp32(x):
    """The fp32 spacing at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, np.float64)).astype(np.float32)).astype(np.float64)
