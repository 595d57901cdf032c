"""A float64 numpy restatement of hwy_lidar's rule (include/hwy.h), independent of the kernel.

Plain numpy on the packed state [NFIELDS, E, 64] that hwy_export_state (or the oracle) hands out,
one env at a time, every ray against every body at once.  It shares no code with csrc/.

The Philox draws (dropout, range noise) are integers and float32 sums of 24-bit uniforms: exact,
through tests/rng_model.py.  Everything geometric carries a bound, derived here and not tuned to
the kernel.  A value is an `R`: the float64 value `v` and a bound `e` on how far the rule's
float32 evaluation can be from it.

  * a stored float32 word, a spec float (as float32) and an integer are exact (e = 0);
  * each float32 operation adds U |result| = 2^-24 |result| to what its operands carry, scaled
    by what the operation does to them (|b| e_a + |a| e_b for a product, e_a / |b| + |a / b| e_b
    / |b| for a quotient, e_a + e_b for a sum) -- unless its operands are exact and its float64
    result is a float32 number: then the float32 operation gives that very number, e = 0;
  * each device sin / cos adds SINCOS_ABS = 2e-7 absolute, the bound
    test_kernels_gpu.py::test_device_math_accuracy_against_libm pins on [-20, 20] (relative 2e-7
    or absolute 1e-7); at an argument of exactly 0 the device gives sin = 0 and cos = 1 exactly
    (test_lidar_gpu.py checks that), so the unaligned ray 0 and a heading-0 body are exact;
  * theta itself is float32 arithmetic on exact operands, which numpy's float32 reproduces bit
    for bit, and so are ox = xe - x_k and oy = ye - y_k.

Decisions are taken with a margin of TOL = 2 times the bound (first-order propagation drops the
products of two errors), and with no margin where the bound is 0.  Per (ray, body) pair the slab
test ends as HIT (hit and counted, whatever the rounding), MISS (no counted hit, whatever the
rounding) or MAYBE.  An axis whose direction component d_a cannot be told from 0 is taken as
unbounded when the origin is inside the slab by the margin and the ends lie beyond the range
either way, as a miss when the origin is outside by the margin and the ends lie beyond the range,
and leaves the pair MAYBE otherwise.  A cell is *undecided* when hit versus no hit, the winning
vehicle or the winning sub-ray could change within the margins: when a MAYBE pair or another HIT
pair can reach below the winner's distance plus its margin (an exact tie of two exact distances
is decided by the rule's tie order, not undecided).  Undecided cells are left out of a
comparison, and so is what depends on them (`seen` of the vehicles involved, the env's counts).

``mistake`` turns one deliberate misreading of the rule on (tests/test_lidar_model.py).
"""

from __future__ import annotations

import numpy as np

import rng_model as rm
from hwy import _abi
from hwy._abi import LidarSpec

F32 = np.float32
U = 2.0 ** -24
SINCOS_ABS = 2e-7
TOL = 2.0
SALT = 0x4C494441
HALF_U, HALF_W = 2.5, 1.0
MISS, HIT, MAYBE = 0, 1, 2
# a direction component within NEAR margins of 0 is not divided by: beyond that the quotient's
# relative error is below 1 / 16 and the first-order bound holds within TOL
NEAR = 8.0
MISTAKES = ("extents_swapped", "no_tout_test", "tie_highest", "half_cell", "align_ignored",
            "vel_along_heading", "range_after_noise", "drop_by_ray", "farthest_wins",
            "inside_negative")


def _f32_exact(v):
    with np.errstate(over="ignore", invalid="ignore"):
        return np.asarray(v, np.float64).astype(F32).astype(np.float64) == v


class R:
    """value and float32 error bound, elementwise numpy float64 (module docstring)"""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, R) else R(x)

    @staticmethod
    def _rounded(v, e):
        return R(v, np.where((e == 0) & _f32_exact(v), 0.0, e + U * np.abs(v)))

    def __add__(self, o):
        o = R.of(o)
        return R._rounded(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = R.of(o)
        return R._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = R.of(o)
        return R._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = R.of(o)
        with np.errstate(divide="ignore", invalid="ignore"):
            r = self.v / o.v
            return R._rounded(r, self.e / np.abs(o.v) + np.abs(r) * o.e / np.abs(o.v))

    def __neg__(self):
        return R(-self.v, self.e)

    def m(self):
        """the margin a decision on this value keeps"""
        return TOL * self.e


def _sincos(angle32):
    """(sin, cos) of float32 angles as R: libm in float64, the device's bound, exact at 0"""
    a = np.asarray(angle32, np.float64)
    e = np.where(a == 0.0, 0.0, SINCOS_ABS)
    return R(np.sin(a), e), R(np.cos(a), e)


def _pick(a: R, b: R, take_a):
    """min or max of a and b given `take_a` (which one the float64 values select): where the
    selection is clear of the margins the selected one's bound, else the larger of the two"""
    with np.errstate(invalid="ignore"):
        clear = np.abs(a.v - b.v) > a.m() + b.m()
    both_exact = (a.e == 0) & (b.e == 0)
    e_sel = np.where(take_a, a.e, b.e)
    return R(np.where(take_a, a.v, b.v), np.where(clear | both_exact, e_sel, np.maximum(a.e, b.e)))


def _axis(o: R, d: R, H, range_m):
    """one axis of the slab test: (lo, hi, state) with state 0 = an interval [lo, hi] (possibly
    infinite), 1 = empty for certain (or ends beyond the range either way: no counted hit), 2 =
    cannot be told"""
    with np.errstate(divide="ignore", invalid="ignore"):
        t1, t2 = (R(-H) - o) / d, (R(H) - o) / d
    lo = _pick(t1, t2, t1.v <= t2.v)
    hi = _pick(t1, t2, t1.v > t2.v)
    state = np.zeros(o.v.shape, np.int8)
    exact0 = (d.e == 0) & (d.v == 0)
    near0 = ~exact0 & (np.abs(d.v) <= NEAR * d.m())
    inside = np.abs(o.v) + o.m() <= H
    inside = np.where(o.e == 0, np.abs(o.v) <= H, inside)
    outside = np.where(o.e == 0, np.abs(o.v) > H, np.abs(o.v) - o.m() > H)
    # the ends' least magnitude when d is not told from 0
    with np.errstate(divide="ignore", invalid="ignore"):
        reach = np.abs(np.abs(o.v) - H) - o.m()
        m_min = np.where(reach > 0, reach / (np.abs(d.v) + d.m()), 0.0)
    far = m_min > 1.001 * range_m
    par = exact0 | near0
    unbounded = par & inside & (exact0 | far)
    empty = par & outside & (exact0 | far)
    # an axis that cannot be told is widened to the whole line: a miss the other axis alone
    # decides is a miss whatever this one is, and a lower end of the other axis bounds d below
    lo = R(np.where(par, -np.inf, lo.v), np.where(par, 0.0, lo.e))
    hi = R(np.where(par, np.inf, hi.v), np.where(par, 0.0, hi.e))
    state = np.where(empty, 1, state)
    state = np.where(par & ~unbounded & ~empty, 2, state)
    return lo, hi, state


def _le(a: R, b: R):
    """(a <= b for certain, a > b for certain)"""
    exact = (a.e == 0) & (b.e == 0)
    with np.errstate(invalid="ignore"):
        yes = np.where(exact, a.v <= b.v, a.v + a.m() <= b.v - b.m())
        no = np.where(exact, a.v > b.v, a.v - a.m() > b.v + b.m())
    return yes, no


class LidarOut:
    """the model's outputs for E envs: values, tolerances (0: exact) and what is undecided"""

    def __init__(self, E, cells, stride):
        self.obs = np.zeros((E, stride), np.float64)
        self.tol = np.zeros((E, stride), np.float64)
        self.skip = np.zeros((E, stride), bool)
        self.hit_vehicle = np.full((E, cells), -1, np.int32)
        self.cell_skip = np.zeros((E, cells), bool)
        self.seen = np.zeros((E, 64), np.float32)
        self.seen_skip = np.zeros((E, 64), bool)
        self.counts = np.zeros((E, 4), np.int32)
        self.counts_skip = np.zeros((E, 4), bool)
        self.dropped = np.zeros((E, cells), bool)
        self.cells = 0        # cells in all
        self.returning = 0    # decided cells with a return (before dropout)
        self.undecided = 0    # undecided cells


def words(state, cells, channel, salt, by=None):
    """[E, cells, 4] Philox words of `channel`: counter (cell, step, channel, SALT + salt), key
    (seed low, seed high); `by`: the first counter word instead of the cell index"""
    ew = np.asarray(state).view(np.uint32)[_abi.F_ENV]
    E = ew.shape[0]
    ctr = np.empty((E, cells, 4), np.uint64)
    ctr[..., 0] = np.arange(cells, dtype=np.uint64)[None, :] if by is None else by
    ctr[..., 1] = ew[:, _abi.E_STEP].astype(np.uint64)[:, None]
    ctr[..., 2] = channel
    ctr[..., 3] = (SALT + int(salt)) & 0xFFFFFFFF
    key = np.stack([ew[:, _abi.E_SEED_LO], ew[:, _abi.E_SEED_HI]], -1).astype(np.uint64)[:, None, :]
    return rm.philox4x32_10(ctr, key)


def u01(w):
    """hm_u01: the word's top 24 bits times 2^-24, exact in float32"""
    return (np.asarray(w, np.uint64) >> np.uint64(8)).astype(F32) * F32(2.0 ** -24)


def z_of(w):
    """hwy_sense's unit-variance draw of four words [..., 4], float32 operation by operation"""
    u = u01(w)
    return (((u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])) - F32(2.0)) * F32(1.7320508)


def _tail(cfg, ego):
    """the ego tail as (values float32, tolerances): hwy_grid's, through grid_model"""
    import grid_model as gm

    vals, tols = [], []
    for f in range(cfg.n_features):
        name = next(n for n, fid in _abi.FEATURES.items() if fid == int(cfg.feature_ids[f]))
        rng = ((cfg.features_range[f][0], cfg.features_range[f][1])
               if cfg.normalize and cfg.has_range[f] else None)
        v, t = gm._value(name, ego, ego, rng, bool(cfg.clip), False, True)
        vals.append(float(v))
        tols.append(float(t))
    return vals, tols


def lidar_model(cfg, state, spec, mistake=None) -> LidarOut:
    assert mistake is None or mistake in MISTAKES, mistake
    spec = LidarSpec.from_dict(spec)
    state = np.asarray(state).view(np.uint32)
    E, V, F = state.shape[1], cfg.vehicles_count + 1, cfg.n_features
    cells, sub, n = spec.cells, spec.sub, spec.cells * spec.sub
    stride = spec.stride(F)
    rng32 = F32(spec.range_m)
    range_m = float(rng32)
    X, Y, H, S = (state[k].view(np.float32) for k in (_abi.F_X, _abi.F_Y, _abi.F_HEADING,
                                                       _abi.F_SPEED))
    present = (state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    present[:, V:] = False
    out = LidarOut(E, cells, stride)
    out.cells = E * cells

    # ---- the draws: exact
    by = None
    if mistake == "drop_by_ray":
        by = (np.arange(cells, dtype=np.uint64) * np.uint64(sub))[None, :]
    dropped = np.zeros((E, cells), bool)
    if spec.p_drop > 0.0:
        dropped = u01(words(state, cells, 0, spec.salt, by)[..., 0]) < F32(spec.p_drop)
    noise = np.zeros((E, cells), F32)
    if spec.sigma_r != 0.0:
        noise = F32(spec.sigma_r) * z_of(words(state, cells, 1, spec.salt))  # float32, as the rule
    out.dropped = dropped

    # ---- the rays' angles: float32, bit for bit
    dth = F32(6.283185307179586 / float(n))
    r = np.arange(n, dtype=np.int64)
    off = F32(0.5) - F32(0.5) * F32(sub)
    if mistake == "half_cell":
        off = off + F32(0.5) * F32(sub)
    theta0 = (r.astype(F32) + off) * dth
    hu, hw = (HALF_W, HALF_U) if mistake == "extents_swapped" else (HALF_U, HALF_W)

    for e in range(E):
        ego = (X[e, 0], Y[e, 0], H[e, 0], S[e, 0])
        with np.errstate(all="ignore"):
            theta = theta0 + ego[2] if (spec.align and mistake != "align_ignored") else theta0
            ox32, oy32 = ego[0] - X[e], ego[1] - Y[e]
        finite = np.isfinite(ox32) & np.isfinite(oy32) & np.isfinite(H[e])
        ks = np.flatnonzero(present[e] & (np.arange(64) >= 1))
        nbodies = len(ks)
        ks = ks[finite[ks]]  # a non-finite body returns nothing (include/hwy.h)
        if spec.ego_tail:
            vals, tols = _tail(cfg, ego)
            out.obs[e, 2 * cells:2 * cells + F] = vals
            out.tol[e, 2 * cells:2 * cells + F] = tols
        vehicle = np.full(cells, -1, np.int64)
        dist = R(np.full(cells, range_m))
        vel = R(np.zeros(cells))
        und = np.zeros(cells, bool)
        rivals = [set() for _ in range(cells)]
        if len(ks) and np.all(np.isfinite([float(v) for v in ego[:3]])):
            sy, cx = _sincos(theta)                       # [n]
            sk, ck = _sincos(H[e, ks])                    # [K]
            dx, dy = R(cx.v[:, None], cx.e[:, None]), R(sy.v[:, None], sy.e[:, None])
            ck, sk = R(ck.v[None, :], ck.e[None, :]), R(sk.v[None, :], sk.e[None, :])
            ox, oy = R(ox32[ks][None, :]), R(oy32[ks][None, :])
            ou, ow = ox * ck + oy * sk, oy * ck - ox * sk
            du, dw = dx * ck + dy * sk, dy * ck - dx * sk
            shape = du.v.shape
            ou = R(np.broadcast_to(ou.v, shape), np.broadcast_to(ou.e, shape))
            ow = R(np.broadcast_to(ow.v, shape), np.broadcast_to(ow.e, shape))
            lo_u, hi_u, st_u = _axis(ou, du, hu, range_m)
            lo_w, hi_w, st_w = _axis(ow, dw, hw, range_m)
            t_in = _pick(lo_u, lo_w, lo_u.v >= lo_w.v)
            t_out = _pick(hi_u, hi_w, hi_u.v <= hi_w.v)
            in_le_out, in_gt_out = _le(t_in, t_out)
            out_ge0, out_lt0 = _le(R(np.zeros(shape)), t_out)
            if mistake == "no_tout_test":
                out_ge0, out_lt0 = np.ones(shape, bool), np.zeros(shape, bool)
            pos, nonpos = _le(R(np.zeros(shape)), t_in)  # 0 <= t_in for certain / t_in < 0
            if mistake == "inside_negative":
                d = R(t_in.v, t_in.e)
            else:
                # d = t_in > 0 ? t_in : +0: exactly 0 where t_in is below 0 by the margin
                d = R(np.where(t_in.v > 0, t_in.v, 0.0), np.where(nonpos, 0.0, t_in.e))
            d_test = d
            if mistake == "range_after_noise":
                cell_of_ray = r // sub
                d_test = d + R(noise[e][cell_of_ray].astype(np.float64)[:, None])
            in_range, beyond = _le(d_test, R(np.full(shape, range_m)))
            some_empty = (st_u == 1) | (st_w == 1)
            some_open = (st_u == 2) | (st_w == 2)
            miss = some_empty | in_gt_out | out_lt0 | beyond
            hit = ~some_empty & ~some_open & in_le_out & out_ge0 & in_range
            status = np.where(miss, MISS, np.where(hit, HIT, MAYBE))
            with np.errstate(invalid="ignore"):
                d_lo = np.where(status == HIT, d.v - d.m(), np.maximum(
                    np.where(np.isfinite(t_in.v), t_in.v - t_in.m(), 0.0), 0.0))
            d_lo = np.where(np.isnan(d_lo), 0.0, d_lo)

            cand = (status != MISS).reshape(cells, -1).any(1)
            for c in np.flatnonzero(cand):
                rows = slice(c * sub, (c + 1) * sub)
                stc, dc, ec, lc = status[rows], d.v[rows], d.e[rows], d_lo[rows]   # [sub, K]
                hits = np.argwhere(stc == HIT)
                win = None
                if len(hits):
                    def key(jk):
                        j, k = jk
                        dv = dc[j, k]
                        if mistake == "farthest_wins":
                            dv = -dv
                        kk = -ks[k] if mistake == "tie_highest" else ks[k]
                        return (dv, j, kk)
                    win = tuple(min((tuple(h) for h in hits), key=key))
                    limit = dc[win] + TOL * ec[win]
                else:
                    limit = range_m
                for j, k in np.argwhere(stc != MISS):
                    if win is not None and (j, k) == win:
                        continue
                    if stc[j, k] == HIT and win is not None and ec[j, k] == 0 and ec[win] == 0:
                        continue  # two exact distances: the rule's order decides
                    if mistake == "farthest_wins" and stc[j, k] == HIT:
                        continue
                    if lc[j, k] <= limit:
                        und[c] = True
                        rivals[c].add(int(ks[k]))
                if win is not None:
                    j, k = win
                    vehicle[c] = ks[k]
                    rivals[c].add(int(ks[k]))
                    dist.v[c], dist.e[c] = dc[win], ec[win]
                    kk = ks[k]
                    spd_k, spd_e = R(float(S[e, kk])), R(float(ego[3]))
                    se, ce = _sincos(np.asarray(ego[2]))
                    skk, ckk = _sincos(np.asarray(H[e, kk]))
                    dvx, dvy = spd_k * ckk - spd_e * ce, spd_k * skk - spd_e * se
                    rdx, rdy = R(cx.v[c * sub + j], cx.e[c * sub + j]), R(sy.v[c * sub + j],
                                                                        sy.e[c * sub + j])
                    if mistake == "vel_along_heading":
                        rdx, rdy = ckk, skk
                    vq = dvx * rdx + dvy * rdy
                    vel.v[c], vel.e[c] = float(vq.v), float(vq.e)

        # ---- after pooling: dropout, noise, normalisation
        out.returning += int(((vehicle >= 0) & ~und).sum())
        out.undecided += int(und.sum())
        ret = (vehicle >= 0) & ~dropped[e]
        dist = R(np.where(ret, dist.v, range_m), np.where(ret, dist.e, 0.0))
        vel = R(np.where(ret, vel.v, 0.0), np.where(ret, vel.e, 0.0))
        if spec.sigma_r != 0.0:
            moved = dist + R(noise[e].astype(np.float64))
            moved = R(np.clip(moved.v, 0.0, range_m), moved.e)
            dist = R(np.where(ret, moved.v, dist.v), np.where(ret, moved.e, dist.e))
        if spec.normalize:
            dist, vel = dist / R(range_m), vel / R(float(F32(spec.speed_scale)))
        out.obs[e, 0:2 * cells:2], out.tol[e, 0:2 * cells:2] = dist.v, TOL * dist.e
        out.obs[e, 1:2 * cells:2], out.tol[e, 1:2 * cells:2] = vel.v, TOL * vel.e
        # an undecided cell that is dropped is decided: it is written as no return
        und_out = und & ~dropped[e]
        out.skip[e, 0:2 * cells:2] = und_out
        out.skip[e, 1:2 * cells:2] = und_out
        out.cell_skip[e] = und_out
        out.hit_vehicle[e] = np.where(ret, vehicle, -1)
        for c in np.flatnonzero(ret & ~und_out):
            out.seen[e, vehicle[c]] = 1.0
        for c in np.flatnonzero(und_out):
            for k in rivals[c]:
                out.seen_skip[e, k] = True
        out.seen_skip[e] &= out.seen[e] == 0  # seen through a decided cell is seen
        out.counts[e] = (nbodies, int(out.seen[e].sum()), int((ret & ~und_out).sum()),
                         int(dropped[e].sum()))
        out.counts_skip[e, 1:3] = bool(und_out.any())  # bodies and dropped cells are exact
    return out


def compare(model: LidarOut, got, what=""):
    """every output of `got` (a dict of numpy arrays by hwy_lidar_args' names; a missing one is
    not compared) against the model: equal where the bound is 0, within it elsewhere, undecided
    entries left out"""
    E = model.obs.shape[0]
    if got.get("obs") is not None:
        g = np.asarray(got["obs"], np.float32).reshape(E, -1)
        assert g.shape == model.obs.shape, (g.shape, model.obs.shape)
        exact = (model.tol == 0) & ~model.skip
        want = model.obs.astype(np.float32)
        bad = exact & (g != want)
        assert not bad.any(), (f"{what}obs differs where the model is exact, first at (env, entry) "
                               f"{tuple(np.argwhere(bad)[0])}: got {g[bad][0]!r}, model "
                               f"{want[bad][0]!r}")
        near = ~exact & ~model.skip
        with np.errstate(invalid="ignore"):
            off = near & ~(np.abs(g.astype(np.float64) - model.obs) <= model.tol)
        assert not off.any(), (f"{what}obs outside the model's bound, first at (env, entry) "
                               f"{tuple(np.argwhere(off)[0])}: got {g[off][0]!r}, model "
                               f"{model.obs[off][0]!r} +- {model.tol[off][0]!r}")
    for name, want, skip in (("hit_vehicle", model.hit_vehicle, model.cell_skip),
                             ("seen", model.seen, model.seen_skip),
                             ("counts", model.counts, model.counts_skip)):
        if got.get(name) is None:
            continue
        a = np.asarray(got[name]).reshape(E, -1)
        bad = (a != want) & ~skip
        assert not bad.any(), (f"{what}{name} differs, first at (env, entry) "
                               f"{tuple(np.argwhere(bad)[0])}: got {a[bad][0]}, model "
                               f"{np.broadcast_to(want, a.shape)[bad][0]}")
