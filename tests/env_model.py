"""A float64 restatement of the observation, the fused wrapper, the reward and `terminated`.

Independent of csrc/hwy_math.h and of oracle/hwy_oracle.c: plain numpy on the packed state
[NFIELDS, E, 64] that hwy_export_state (or the oracle) hands out.  The source is upstream's
semantics as SURVEY.md §8 (a1.7, a1.8, a3-a5) and the DESIGN.md §4 constant table record them,
not the C code, so a misreading shared by the kernel and the oracle shows here.

Every result is a `Q`: the float64 value `v` and a bound `e` on how far a float32 evaluation of
the same expression can be from it.  The bound is derived, not measured:

  * a stored float32 word, a config float and an integer are exact (e = 0);
  * each float32 operation adds 2^-24 * |its result| (round to nearest) to the errors its
    operands carry, scaled by what the operation does to them (|b| e_a + |a| e_b for a product,
    e_a / |b| + |a / b| e_b / |b| for a quotient, e_a + e_b for a sum; clip and a sign change add
    nothing; the Euclidean norm is 1-Lipschitz in each component, plus its own four roundings);
  * each device sin / cos adds 1e-7 absolute (so 1e-7 * |speed| once multiplied by a speed),
    the bound tests/test_kernels_gpu.py::test_device_math_accuracy_against_libm pins, on top of
    the error of its argument (|sin'|, |cos'| <= 1);
  * a float32 constant that stands for a real number (2 pi) counts as one more rounding.

The comparison allows TOL_FACTOR = 2 times that sum: the first-order propagation above drops
the products of two errors and the device bound is 2e-7 relative where |cos| is near 1.  A value
whose bound is 0 (presence, a raw stored word, a zero row) must be equal exactly.

Decisions (who is admitted, on_road) are taken in float64; `uncertain` names the envs where such
a decision sits on a float32 rounding edge, which the comparison then leaves out for that step.
The one exception is the sort key of `sorted`: |x_k - x_ego| as ONE float32 subtraction of the
stored positions, which is correctly rounded and is what defines the order.
"""

from __future__ import annotations

import numpy as np

from hwy import _abi

U = 2.0 ** -24        # relative error of one float32 operation, round to nearest
SINCOS_ABS = 1e-7     # device sin / cos, absolute (test_device_math_accuracy_against_libm)
TOL_FACTOR = 2.0      # see the module docstring
ASIN_REL, ATAN_REL, TAN_REL = 3e-7, 2e-7, 6e-7  # device asin / atan / tan, relative (same test)
POW_REL = 1e-5        # device pow, relative (test_device_pow_and_idm_pow_against_numpy)

LANE_WIDTH = 4.0      # AbstractLane.DEFAULT_WIDTH
ROAD_LENGTH = 10000.0  # straight_road_network
VEHICLE_LENGTH = 5.0  # Vehicle.LENGTH and AbstractLane.VEHICLE_LENGTH
PERCEPTION = 200.0    # 5 * Vehicle.MAX_SPEED
EDGE = 1e-3           # metres: float32 ulp at 1.5 km is 1.2e-4, so 1e-3 covers the subtraction
#                       and the square root of a threshold test


class Q:
    """value and float32 error bound, elementwise numpy float64"""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape).copy()

    @staticmethod
    def of(x):
        return x if isinstance(x, Q) else Q(x)

    def _op(self, v, e):
        return Q(v, e + U * np.abs(v))

    def __add__(self, o):
        o = Q.of(o)
        return self._op(self.v + o.v, self.e + o.e)

    def __sub__(self, o):
        o = Q.of(o)
        return self._op(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        o = Q.of(o)
        return self._op(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e)

    def __truediv__(self, o):
        o = Q.of(o)
        r = self.v / o.v
        return self._op(r, self.e / np.abs(o.v) + np.abs(r) * o.e / np.abs(o.v))

    def clip(self, lo, hi):
        return Q(np.clip(self.v, lo, hi), self.e)

    def abs(self):
        return Q(np.abs(self.v), self.e)

    def cos(self):
        return Q(np.cos(self.v), self.e + SINCOS_ABS)

    def sin(self):
        return Q(np.sin(self.v), self.e + SINCOS_ABS)

    def where(self, mask, other):
        other = Q.of(other)
        return Q(np.where(mask, self.v, other.v), np.where(mask, self.e, other.e))

    # ---- the operations of the dynamics (tests/dyn_model.py).  The library bounds are the ones
    # test_device_math_accuracy_against_libm (asin 3e-7, atan 2e-7, tan 6e-7 relative) and
    # test_device_pow_and_idm_pow_against_numpy (pow 1e-5 relative) pin; sqrt is correctly
    # rounded (test_math_library_correctly_rounded_ops).
    def sqrt(self):
        r = np.sqrt(np.maximum(self.v, 0.0))
        with np.errstate(divide="ignore", invalid="ignore"):
            # the root over [v - e, v + e]; at v <= e the whole of sqrt(v + e)
            e = np.where(self.v > self.e, self.e / (2.0 * np.sqrt(np.maximum(self.v - self.e, 1e-300))),
                         np.sqrt(np.maximum(self.v, 0.0) + self.e))
        return Q(r, e + U * r)

    def _through(self, fn, rel, lo=-np.inf, hi=np.inf):
        """a monotone library function: the image of [v - e, v + e] (within the domain) plus the
        library's relative error"""
        r = fn(self.v)
        a, b = fn(np.clip(self.v - self.e, lo, hi)), fn(np.clip(self.v + self.e, lo, hi))
        return Q(r, np.maximum(np.abs(a - r), np.abs(b - r)) + rel * np.abs(r))

    def asin(self):
        return Q(np.clip(self.v, -1.0, 1.0), self.e)._through(np.arcsin, ASIN_REL, -1.0, 1.0)

    def atan(self):
        return self._through(np.arctan, ATAN_REL)

    def tan(self):
        """for |v| + e < pi / 2"""
        return self._through(np.tan, TAN_REL)

    def pow(self, p):
        """v ** p for v >= 0 and an exact exponent p"""
        r = np.power(self.v, p)
        with np.errstate(divide="ignore", invalid="ignore"):
            d = np.where(self.v > 0, np.abs(p) * r / np.where(self.v > 0, self.v, 1.0), 0.0)
        return Q(r, d * self.e + POW_REL * np.abs(r))

    def minimum(self, o):
        """min and max are 1-Lipschitz in the sup norm"""
        o = Q.of(o)
        return Q(np.minimum(self.v, o.v), np.maximum(self.e, o.e))

    def maximum(self, o):
        o = Q.of(o)
        return Q(np.maximum(self.v, o.v), np.maximum(self.e, o.e))

    def clip_sat(self, lo, hi, const_err=0.0):
        """clip that knows when it saturates: where the value is beyond a limit by more than
        TOL_FACTOR times its bound, a float32 evaluation returns the limit itself, whose error
        is `const_err` (0 for a limit float32 holds exactly, one rounding for pi / 4)."""
        sat = (self.v - TOL_FACTOR * self.e > hi) | (self.v + TOL_FACTOR * self.e < lo)
        return Q(np.clip(self.v, lo, hi), np.where(sat, const_err, self.e + const_err))

    def __getitem__(self, idx):
        return Q(self.v[idx], self.e[idx])


def qstack(qs, axis=-1):
    return Q(np.stack([q.v for q in qs], axis), np.stack([q.e for q in qs], axis))


def norm2(a: Q, b: Q) -> Q:
    """sqrt(a*a + b*b) as float32 computes it: two products, a sum, a root"""
    d = np.sqrt(a.v * a.v + b.v * b.v)
    return Q(d, a.e + b.e + 2.0 * U * d)


def lmap(v: Q, x0, x1, y0, y1) -> Q:
    """utils.lmap: y0 + (v - x0) * (y1 - y0) / (x1 - x0)"""
    return Q.of(y0) + (v - Q.of(x0)) * (Q.of(y1) - Q.of(y0)) / (Q.of(x1) - Q.of(x0))


# ------------------------------------------------------------------------------- state
def _f(state, field):
    return state[field].view(np.float32).astype(np.float64)


def _present(cfg, state):
    V = cfg.vehicles_count + 1
    p = (state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    p[:, V:] = False
    return p


def _admitted(cfg, state):
    """Road.close_objects_to(ego, 200 m, see_behind): [E, 64] bool (the ego itself is not)."""
    x, y = _f(state, _abi.F_X), _f(state, _abi.F_Y)
    dx, dy = x - x[:, :1], y - y[:, :1]
    ok = _present(cfg, state) & (np.sqrt(dx * dx + dy * dy) < PERCEPTION)
    if not cfg.see_behind:
        ok &= dx > -2.0 * VEHICLE_LENGTH
    ok[:, 0] = False
    return ok


def observed_vehicles(cfg, state):
    """[E, N-1] vehicle indices of the observation's rows 1.., -1 for a missing row.  `sorted`:
    by |dx| (one float32 subtraction of the stored positions), ties by vehicle index;
    `shuffled`: the first N-1 admitted by index (before the permutation)."""
    E = state.shape[1]
    N = cfg.obs_vehicles
    ok = _admitted(cfg, state)
    x32 = state[_abi.F_X].view(np.float32)
    key = np.abs(x32 - x32[:, :1])
    assert key.dtype == np.float32
    out = np.full((E, max(N - 1, 0)), -1, np.int64)
    for e in range(E):
        idx = np.nonzero(ok[e])[0]
        if cfg.order == _abi.ORDER_SORTED:
            idx = idx[np.argsort(key[e, idx], kind="stable")]
        idx = idx[:N - 1]
        out[e, :len(idx)] = idx
    return out


def _features(cfg, state):
    """Vehicle.to_dict per feature of the config's list: Q [E, 64, F]"""
    x, y, h, spd = (Q(_f(state, k)) for k in (_abi.F_X, _abi.F_Y, _abi.F_HEADING, _abi.F_SPEED))
    c, s = h.cos(), h.sin()
    by_id = {0: Q(np.ones_like(x.v)), 1: x, 2: y, 3: spd * c, 4: spd * s, 5: c, 6: s, 7: h}
    return qstack([by_id[int(cfg.feature_ids[f])] for f in range(cfg.n_features)])


RELATIVE = (1, 2, 3, 4)  # x, y, vx, vy


def observe_model(cfg, state) -> Q:
    """KinematicObservation.observe before the shuffle and before the wrapper: Q [E, N, F].

    Row 0 is the ego, absolute.  Rows 1.. are `observed_vehicles`; x, y, vx, vy relative to the
    ego unless `absolute`; a feature is mapped from its range to [-1, 1] only under `normalize`
    and only if it has a range, and clipped only then and only under `clip`; missing rows are 0."""
    E, N, F = state.shape[1], cfg.obs_vehicles, cfg.n_features
    feat = _features(cfg, state)
    rows = observed_vehicles(cfg, state)
    ar = np.arange(E)[:, None]
    src = np.concatenate([np.zeros((E, 1), np.int64), np.maximum(rows, 0)], 1)
    val = feat[ar, src]                                   # [E, N, F]
    other = np.concatenate([np.zeros((E, 1), bool), np.ones((E, N - 1), bool)], 1)
    cols = []
    for f in range(F):
        q = val[:, :, f]
        if not cfg.absolute and int(cfg.feature_ids[f]) in RELATIVE:
            q = (q - feat[:, 0, f][:, None]).where(other, q)
        if cfg.normalize and cfg.has_range[f]:
            q = lmap(q, float(cfg.features_range[f][0]), float(cfg.features_range[f][1]), -1.0, 1.0)
            if cfg.clip:
                q = q.clip(-1.0, 1.0)
        cols.append(q)
    obs = qstack(cols)
    missing = np.concatenate([np.zeros((E, 1), bool), rows < 0], 1)
    return Q(np.zeros_like(obs.v)).where(missing[:, :, None], obs)


def wrap_rows(cfg, rows: Q, ref: Q, table, positions=None) -> Q:
    """The fused wrapper on rows Q [..., F] against the reference row `ref` Q [..., F] (the row
    at ego_idx): Q [..., F_out].  RankPE appends table[position]; `positions` [...] then names
    each row's index in the observation."""
    kind, d, F = int(cfg.pe_kind), int(cfg.d_embed), int(cfg.n_features)
    if kind == _abi.PE_NONE:
        return rows
    if kind == _abi.PE_RANK:
        t = np.asarray(table, np.float64).reshape(cfg.obs_vehicles, d)[positions]
        return Q(np.concatenate([rows.v, t], -1), np.concatenate([rows.e, np.zeros_like(t)], -1))
    rx = rows[..., 0] - ref[..., 0]
    if kind == _abi.PE_DIST1:    # DistanceEmbedWrapper(use_euclidean=False): |x_i - x_ego|
        dist = rx.abs()
    else:                        # ||obs[i, :2] - obs[ego, :2]||
        dist = norm2(rx, rows[..., 1] - ref[..., 1])
    nd = (dist / float(cfg.pe_max_dist)).clip(0.0, 1.0)
    tab = np.asarray(table if table is not None else [], np.float64)
    two_pi = Q(2.0 * np.pi, U * 2.0 * np.pi)  # the float32 constant
    if kind in (_abi.PE_DIST, _abi.PE_DIST1):
        ang = [(two_pi * nd) * float(tab[k]) for k in range(d // 2)]
        return Q(np.concatenate([rows.v] + [a.sin().v[..., None] for a in ang] +
                                [a.cos().v[..., None] for a in ang], -1),
                 np.concatenate([rows.e] + [a.sin().e[..., None] for a in ang] +
                                [a.cos().e[..., None] for a in ang], -1))
    assert kind == _abi.PE_ROPE
    cols = [rows[..., f] for f in range(F)]
    for p in range(d // 2):
        th = (two_pi * nd) * float(tab[p])
        c, s = th.cos(), th.sin()
        xx, yy = rows[..., 2 * p], rows[..., 2 * p + 1]
        cols[2 * p] = xx * c - yy * s
        cols[2 * p + 1] = xx * s + yy * c
    return qstack(cols)


def wrap_model(cfg, obs: Q, table) -> Q:
    """The fused wrapper on an observation Q [E, N, F] in its final row order."""
    E, N = obs.v.shape[:2]
    eg = int(cfg.ego_idx)
    ref = Q(obs.v[:, eg:eg + 1, :], obs.e[:, eg:eg + 1, :])
    pos = np.broadcast_to(np.arange(N), (E, N))
    return wrap_rows(cfg, obs, ref, table, pos)


def on_road(cfg, state):
    """The ego lane's AbstractLane.on_lane(position, margin=0) on the straight road, as the oracle
    defines it: |y - 4 * lane| <= 4 / 2 and -5 <= x < 10000 + 5, with `lane` the ego's stored
    lane id.  [E] bool."""
    x, y = _f(state, _abi.F_X)[:, 0], _f(state, _abi.F_Y)[:, 0]
    lane = state[_abi.F_LANE][:, 0].astype(np.int32).astype(np.float64)
    return (np.abs(y - LANE_WIDTH * lane) <= LANE_WIDTH / 2.0) & \
        (-VEHICLE_LENGTH <= x) & (x < ROAD_LENGTH + VEHICLE_LENGTH)


def reward_model(cfg, state):
    """HighwayEnv._rewards / _reward / _is_terminated on the ego of the post-step state.
    Returns (terms Q [E, 4] in REWARD_KEYS order, reward Q [E], terminated bool [E])."""
    lane = state[_abi.F_LANE][:, 0].astype(np.int32).astype(np.float64)
    crashed = (state[_abi.F_FLAGS][:, 0] & _abi.FLAG_CRASHED) != 0
    spd, h = Q(_f(state, _abi.F_SPEED)[:, 0]), Q(_f(state, _abi.F_HEADING)[:, 0])
    lo, hi = float(cfg.reward_speed_range[0]), float(cfg.reward_speed_range[1])
    cr, rl = float(cfg.collision_reward), float(cfg.right_lane_reward)
    hs, onr = float(cfg.high_speed_reward), float(cfg.on_road_reward)
    collision = Q(crashed.astype(np.float64))
    right_lane = Q(lane) / float(max(cfg.lanes_count - 1, 1))
    high_speed = lmap(spd * h.cos(), lo, hi, 0.0, 1.0).clip(0.0, 1.0)
    road = on_road(cfg, state)
    road_f = Q(road.astype(np.float64))
    rew = Q(np.zeros_like(lane))
    for w, term in ((cr, collision), (rl, right_lane), (hs, high_speed), (onr, road_f)):
        rew = rew + Q(w) * term
    if cfg.normalize_reward:
        rew = lmap(rew, cr, Q(hs) + Q(rl), 0.0, 1.0)
    rew = rew * road_f
    terminated = crashed | (bool(cfg.offroad_terminal) & ~road)
    return qstack([collision, right_lane, high_speed, road_f]), rew, terminated


def uncertain(cfg, state):
    """[E] bool: a decision of this env sits on a float32 rounding edge -- a present vehicle
    within 1e-3 m of the 200 m or (without see_behind) the -10 m admission threshold, or the ego
    within 1e-3 m of an edge of its lane."""
    x, y = _f(state, _abi.F_X), _f(state, _abi.F_Y)
    dx, dy = x - x[:, :1], y - y[:, :1]
    p = _present(cfg, state)
    p[:, 0] = False
    edge = np.abs(np.sqrt(dx * dx + dy * dy) - PERCEPTION) < EDGE
    if not cfg.see_behind:
        edge |= np.abs(dx + 2.0 * VEHICLE_LENGTH) < EDGE
    lane = state[_abi.F_LANE][:, 0].astype(np.int32).astype(np.float64)
    lat = np.abs(y[:, 0] - LANE_WIDTH * lane)
    return (edge & p).any(axis=1) | (np.abs(lat - LANE_WIDTH / 2.0) < EDGE)
