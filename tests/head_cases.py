"""The case table of the loss-head tests (test_head_model.py on the CPU, test_head_gpu.py on the
kernels) and the selector network that hands a table row's mu and val to the head exactly.

The table is drawn on the CPU with a fixed numpy seed; every stored number is an fp32.  A row
holds mu[2], val, z[2], old_logp, adv, ret and the indices of its log_std pair and coefficient
triple.  old_logp is the float64 model's log-prob plus delta, rounded once.  Rows whose branch
the model cannot determine at the drawn delta (tail rows, whose ratio bound is wide) move to
delta +-5 and then +-30; test_head_model.py asserts that none is left undetermined."""

import numpy as np

import head_model as hm

Z = (0.0, 0.5, -0.5, 2.9, -2.9, 3.1, -3.1, 4.0, -4.0, 5.0, -5.0, 6.0, -6.0, 7.5, -7.5, 8.5, -8.5,
     9.5, -9.5, 12.0, -12.0)
Z_MODERATE = Z[:5]
Z_TAIL = Z[9:]
LOG_STDS = ((-0.4, 0.3), (-2.0, 1.0), (0.0, 0.0), (-5.0, 2.0))
ZMU = (0.0, 0.1, -0.1, 1.0, -1.0, 4.0, -4.0)  # z - mu in units of sigma
DELTAS = (0.0, 1e-3, -1e-3, 1.0, -1.0, 5.0, -5.0, 30.0, -30.0)
EDGES = ("lo_in", "lo_out", "hi_in", "hi_out")  # the ratio just inside / outside a clip bound
ADV = (1.0, -1.0, 0.0, 1e-3, -1e-3, 50.0, -50.0)
RETVAL = (0.0, 1e-3, -1e-3, 10.0, -10.0)
VALS = (0.25, -1.5, 3.0, 0.0)
COEFS = ((0.2, 0.5, 0.005), (0.1, 1.0, 0.02), (0.3, 0.25, 0.0))  # ppo_ref_util.COEFS
NUDGE = 2.0 ** -7  # a mu or val that would be 0: one unit of each +- pair of the selector is on
EDGE_MARGIN = 4.0  # the edge rows' distance from the clip bound, in ratio bounds

f32 = lambda x: np.asarray(x, np.float32)  # noqa: E731


def coefs32(ci):
    """The coefficient triple as the fp32 values the kernels are handed."""
    return tuple(float(np.float32(c)) for c in COEFS[ci])


class Table:
    """Arrays over the rows: mu [n, 2], val, z [n, 2], old, adv, ret (fp32), ls, coef (indices),
    delta (the spec each row ended up with: a float or an EDGES name), k and rv (the drawn
    (z - mu) / sigma and ret - val)."""

    def __len__(self):
        return self.z.shape[0]

    def model(self, rows, B=1, mut=None, K=hm.K_SQUASH, old=None):
        """head_rows of the given rows, which must share log_std and coefficients."""
        rows = np.asarray(rows)
        li, ci = int(self.ls[rows[0]]), int(self.coef[rows[0]])
        assert (self.ls[rows] == li).all() and (self.coef[rows] == ci).all()
        eps, vc, ec = coefs32(ci)
        return hm.head_rows(self.mu[rows], self.val[rows], self.z[rows],
                            self.old[rows] if old is None else old, self.adv[rows], self.ret[rows],
                            f32(LOG_STDS[li]), eps, vc, ec, B, mut=mut, K=K)

    def groups(self):
        """{(ls index, coef index): row indices}."""
        out = {}
        for i in range(len(self)):
            out.setdefault((int(self.ls[i]), int(self.coef[i])), []).append(i)
        return out


def _old_for(T, i, spec):
    """old_logp (fp32) of row i for a delta spec."""
    R = T.model([i], old=np.zeros(1))
    logp = R.v["logp"][0]
    if not isinstance(spec, str):
        return np.float32(logp + spec)
    eps = coefs32(int(T.coef[i]))[0]
    bound = 1.0 - eps if spec.startswith("lo") else 1.0 + eps
    inward = (spec == "lo_in") or (spec == "hi_out")  # the ratio above the bound
    x = 0.0
    for _ in range(3):  # the bound depends (weakly) on old itself
        old = logp - np.log(bound * (1.0 + x if inward else 1.0 - x))
        Rk = T.model([i], old=np.array([float(np.float32(old))]))
        rel = Rk.e["ratio"][0] / Rk.v["ratio"][0]
        x = (EDGE_MARGIN + 1.0) * rel + 8.0 * hm.U * (1.0 + abs(old))  # old's own rounding
    return np.float32(old)


def build_table(seed=14):
    rng = np.random.RandomState(seed)
    pick = lambda seq: seq[rng.randint(len(seq))]  # noqa: E731
    specs = []

    def add(z0, z1, li=None, k0=None, k1=None, delta=None, adv=None, rv=None, ci=None):
        specs.append(dict(
            z=(z0, z1), li=rng.randint(4) if li is None else li,
            k=(pick(ZMU) if k0 is None else k0, pick(ZMU) if k1 is None else k1),
            delta=pick(DELTAS) if delta is None else delta, adv=pick(ADV) if adv is None else adv,
            rv=pick(RETVAL) if rv is None else rv, ci=rng.randint(3) if ci is None else ci,
            val=pick(VALS)))

    for j, zv in enumerate(Z):  # every z value under every log_std, in either component
        for li in range(4):
            other = pick(Z)
            add(*((zv, other) if (j + li) % 2 == 0 else (other, zv)), li=li)
    for d in DELTAS + EDGES:  # every delta with every advantage, away from the tails
        for a in ADV:
            add(pick(Z_MODERATE), pick(Z_MODERATE), delta=d, adv=a)
    for k in ZMU:
        for li in range(4):
            add(pick(Z[:9]), pick(Z[:9]), li=li, k0=k)
    for rv in RETVAL:
        for ci in range(3):
            add(pick(Z[:9]), pick(Z[:9]), rv=rv, ci=ci)
    for _ in range(30):  # both components in the tails
        add(pick(Z_TAIL), pick(Z_TAIL))

    n = len(specs)
    T = Table()
    T.z = f32([s["z"] for s in specs])
    T.k = np.array([s["k"] for s in specs])  # as drawn: (z - mu) / sigma and ret - val
    T.rv = np.array([s["rv"] for s in specs])
    T.ls = np.array([s["li"] for s in specs])
    T.coef = np.array([s["ci"] for s in specs])
    sigma = np.exp(np.array([LOG_STDS[s["li"]] for s in specs], np.float64))
    mu = f32(T.z.astype(np.float64) - np.array([s["k"] for s in specs]) * sigma)
    T.mu = np.where(mu == 0, np.float32(NUDGE), mu)
    val = f32([s["val"] for s in specs])
    T.val = np.where(val == 0, np.float32(NUDGE), val)
    T.ret = f32(T.val.astype(np.float64) + np.array([s["rv"] for s in specs]))
    T.adv = f32([s["adv"] for s in specs])
    T.old = np.zeros(n, np.float32)
    T.delta = []
    for i, s in enumerate(specs):
        spec = s["delta"]
        sign = -1.0 if (not isinstance(spec, str) and spec < 0) else 1.0
        for cand in (spec, 5.0 * sign, 30.0 * sign):
            T.old[i] = _old_for(T, i, cand)
            if not T.model([i]).und[0]:
                break
        T.delta.append(cand)
    return T


_TABLE = None


def table():
    """The one table, built once per process and never written to."""
    global _TABLE
    if _TABLE is None:
        _TABLE = build_table()
        for a in (_TABLE.z, _TABLE.mu, _TABLE.val, _TABLE.ret, _TABLE.adv, _TABLE.old):
            a.setflags(write=False)
    return _TABLE


def sweep_subset(T, n=20):
    """The rows of the tile-position sweep: the first of each (log_std, coefficients) group, then
    the rows with the largest |z| and the edge rows, up to n."""
    first = [g[0] for g in T.groups().values()]
    edges = [i for i, d in enumerate(T.delta) if isinstance(d, str)][:4]
    tails = list(np.argsort(-np.abs(T.z).max(1), kind="stable")[:n])
    out = []
    for i in first + edges + tails:
        if i not in out:
            out.append(int(i))
    return out[:n]


# ------------------------------------------------------------------------- selector network
def selector_state_dict(S, H, log_std):
    """ActorCritic weights under which mu0 = s[0], mu1 = s[1] and val = s[2] bit for bit: every
    product is a value times +-1 and every sum adds zeros (units 0..5 carry relu(+-s[0..2])
    through the trunk and both towers unchanged)."""
    import torch

    z = lambda *shape: torch.zeros(*shape)  # noqa: E731
    W1 = z(H, S)
    for k in range(3):
        W1[2 * k, k], W1[2 * k + 1, k] = 1.0, -1.0
    eye = z(H, H)
    for j in range(6):
        eye[j, j] = 1.0
    wa2, wc2 = z(2, H), z(1, H)
    wa2[0, 0], wa2[0, 1] = 1.0, -1.0
    wa2[1, 2], wa2[1, 3] = 1.0, -1.0
    wc2[0, 4], wc2[0, 5] = 1.0, -1.0
    return {
        "shared.0.weight": W1, "shared.0.bias": z(H),
        "shared.2.weight": eye.clone(), "shared.2.bias": z(H),
        "actor_mean.0.weight": eye.clone(), "actor_mean.0.bias": z(H),
        "actor_mean.2.weight": wa2, "actor_mean.2.bias": z(2),
        "log_std": torch.tensor(np.asarray(log_std, np.float32)),
        "critic.0.weight": eye.clone(), "critic.0.bias": z(H),
        "critic.2.weight": wc2, "critic.2.bias": z(1),
    }


def selector_states(mu, val, S):
    """State rows [n, S] carrying mu and val in columns 0..2, zeros elsewhere."""
    s = np.zeros((mu.shape[0], S), np.float32)
    s[:, :2], s[:, 2] = mu, val
    return s
