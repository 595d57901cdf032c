"""hwy_traffic restated in numpy: the neighbour rule, gaps, time-to-collision, time headway, the
ego row and the per-episode fold.  It shares no code with the kernel; the source is the rule as
include/hwy.h states it (Road.neighbour_vehicles as tests/dyn_model.py:neighbours restates it).

What is exact and what carries a bound
--------------------------------------
Every decision and value that the kernel forms from stored words with float32 operations whose
result IEEE-754 fixes is restated here in numpy float32 and must match bit for bit:

  * the candidates: |y_k - 4c| <= 3 as ONE float32 subtraction of the stored y and the exact
    float32 4c, and -5 <= x_k < 10005 on the stored x; front / rear and the ego's side-lane
    neighbours are then comparisons of stored words: exact, no tolerance, nothing left out;
  * gap = (x_f - x_i) - 5, the rear gap (x_e - x_r) - 5, the side gaps, slot 13 = y_e - 4 ln:
    two float32 operations each, correctly rounded, so numpy float32 gives the same bits;
  * slot 11: dx = x_k - x_e, dy = y_k - y_e, dx*dx + dy*dy (two products and a sum, no fused
    multiply-add), the least over the other present vehicles, one correctly rounded square root;
  * slot 12: the count of 0 <= x_k - x_e <= near_range on the float32 difference.

Everything downstream of vx = speed * cos(heading) carries a bound, derived with env_model.Q:

  * cos: the device's cosine is within SINCOS_ABS = 1e-7 absolute of the real one, so
    e(vx) = |speed| * 1e-7 + U |vx| (the product's rounding, U = 2^-24);
  * closing = vx_i - vx_f: e = e(vx_i) + e(vx_f) + U |closing|.  Two vehicles whose heading and
    speed words are equal bit for bit have the same vx bit for bit (one deterministic function of
    the same inputs), so their closing is exactly 0 and carries no bound;
  * ttc = gap / closing and thw = gap / vx_i: the float32 gap is exact (above), so by Q's quotient
    rule e = |q| e(den) / |den| + U |q|;
  * risk = 1 - ttc / H: e(ttc) / H + U |ttc / H| for the quotient, plus U |risk| for the
    difference.

A value is accepted within TOL_FACTOR = 2 times its bound, as in the other models (first-order
propagation drops products of two errors; the cosine's bound is 2e-7 relative near |cos| = 1).  A
value whose bound is 0 (0, +inf, 1, a value of equal words) must be equal exactly.

Three decisions take a bounded value: closing > 0, vx > 0 (each only where 0 < gap < inf: at
gap <= 0 the result is 0 and at gap = +inf it is +inf either way) and ttc < risk_horizon.  Where
the float64 value is within TOL_FACTOR times its bound of the threshold, the entry is marked
undecided and that output (and what follows from it: risk from ttc) is not compared there.

`CONSTS` holds what tests change to show the comparison notices a mistake.
"""

from __future__ import annotations

import numpy as np

import dyn_model as dm
from env_model import Q, TOL_FACTOR
from hwy import _abi

CONSTS = dict(
    LENGTH=5.0,          # Vehicle.LENGTH: the gap is bumper to bumper
    MARGIN=1.0,          # on_lane margin of Road.neighbour_vehicles
    FRONT_TIE_LAST=True,   # among equal x the front is the last in vehicle order
    REAR_TIE_FIRST=True,   # ... and the rear the first
    REAR_STRICT=True,    # rear: x_k < x_i (front: x_i <= x_k)
    CLOSING_SIGN=1.0,    # closing = vx_i - vx_f
    COSINE=True,         # vx = speed * cos(heading)
)
DEFAULTS = dict(ttc_thresh=2.0, thw_thresh=1.0, risk_horizon=4.0, near_range=50.0)
NEGO, NACC = 16, 8
F32 = np.float32
INF32 = F32(np.inf)
EXACT_EGO = (4, 7, 8, 9, 10, 11, 12, 13)    # float32 restatements: bit for bit
BOUND_EGO = (0, 1, 2, 3, 5, 6, 14, 15)      # downstream of vx (slot 0 is the exact gap again)


def neighbours(x, onl, front_last=True, rear_first=True, rear_strict=True):
    """dyn_model.neighbours with the three readings a mistake could take as switches; with the
    defaults it is that function (tests/test_traffic_model.py holds the two together)."""
    E, V, L = onl.shape
    k = np.arange(V)
    other = k[:, None] != k[None, :]
    xk = np.broadcast_to(x[:, None, :], (E, V, V))
    xi = x[:, :, None]
    ahead = (xk >= xi) & other
    behind = ((xk < xi) if rear_strict else (xk <= xi)) & other
    front = np.full((E, V, L), -1, np.int64)
    rear = np.full((E, V, L), -1, np.int64)
    for c in range(L):
        for out, cand, nearest, want_last in ((front, ahead, np.min, front_last),
                                              (rear, behind, np.max, not rear_first)):
            M = cand & onl[:, None, :, c]
            fill = np.inf if nearest is np.min else -np.inf
            ext = nearest(np.where(M, xk, fill), axis=-1)
            best = M & (xk == ext[..., None])
            first = np.argmax(best, -1)
            last = V - 1 - np.argmax(best[..., ::-1], -1)
            out[:, :, c] = np.where(M.any(-1), last if want_last else first, -1)
    return front, rear


def _take(a, idx):
    """a [E, V] at vehicle indices idx [E, ...]; a negative index reads vehicle 0 (masked by the
    caller)"""
    ar = np.arange(a.shape[0]).reshape((a.shape[0],) + (1,) * (idx.ndim - 1))
    return a[ar, np.maximum(idx, 0)]


def _qtake(q, idx):
    return Q(_take(q.v, idx), _take(q.e, idx))


def _lane_pick(arr, lane, L):
    """arr [E, V, L] at each vehicle's lane [E, V]; -1 where the lane does not exist"""
    ok = (lane >= 0) & (lane < L)
    got = np.take_along_axis(arr, np.clip(lane, 0, L - 1)[..., None], -1)[..., 0]
    return np.where(ok, got, -1)


def _near(q, thresh):
    """|q - thresh| within TOL_FACTOR times q's bound (and the bound not 0): undecidable"""
    with np.errstate(invalid="ignore"):
        return (np.abs(q.v - thresh) <= TOL_FACTOR * q.e) & (q.e > 0)


def _ratio(gap32, den):
    """the ttc / thw rule on an exact float32 gap and a bounded denominator:
    0 where gap <= 0, gap / den where den > 0, else +inf -> (Q, undecided)"""
    gap = np.asarray(gap32, np.float64)
    live = (gap > 0) & np.isfinite(gap)
    und = live & _near(den, 0.0)
    pos = den.v > 0
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        q = Q(np.where(live & pos, gap, 1.0)) / Q(np.where(live & pos, den.v, 1.0),
                                                  np.where(live & pos, den.e, 0.0))
    v = np.where(gap <= 0, 0.0, np.where(live & pos, q.v, np.inf))
    e = np.where(live & pos, q.e, 0.0)
    return Q(v, e), und


def _risk(ttc, und_ttc, horizon):
    und = und_ttc | _near(ttc, horizon)
    inside = ttc.v < horizon
    t = Q(np.where(inside, ttc.v, 0.0), np.where(inside, ttc.e, 0.0))
    r = Q(1.0) - t / Q(float(horizon))
    return Q(np.where(inside, r.v, 0.0), np.where(inside, r.e, 0.0)), und


def _pad(a, fill, dtype):
    out = np.full((a.shape[0], 64), fill, dtype)
    out[:, :a.shape[1]] = a
    return out


def _qpad(q, fill):
    return Q(_pad(q.v, fill, np.float64), _pad(q.e, 0.0, np.float64))


def traffic_model(cfg, st, consts=None, **thresholds):
    """hwy_traffic's outputs for the packed state st [NFIELDS, E, 64] uint32.

    Returns a dict: `front`, `rear` [E, 64] int; `gap` [E, 64] float32 (exact); `closing`, `ttc`,
    `thw`, `risk` Q [E, 64]; `und` a dict name -> [E, 64] bool for the four; `present` [E, 64];
    `ego_exact` {slot: [E] float32}; `ego` {slot: Q [E]}; `ego_und` {slot: [E] bool};
    `side` (front, rear) [E, 2] the ego's neighbours on lanes ln - 1 and ln + 1."""
    K = dict(CONSTS, **(consts or {}))
    T = dict(DEFAULTS, **thresholds)
    s = dm.unpack(cfg, st)
    E, V = s["x"].shape
    L = int(cfg.lanes_count)
    x32 = st[_abi.F_X].view(F32)[:, :V]
    y32 = st[_abi.F_Y].view(F32)[:, :V]
    hbits, sbits = st[_abi.F_HEADING][:, :V], st[_abi.F_SPEED][:, :V]
    x, lane, present = s["x"], s["lane"], s["present"]
    length = F32(K["LENGTH"])

    # ---- the candidates of every lane, in float32, and the neighbours
    lat = y32[:, :, None] - (F32(4.0) * np.arange(L, dtype=F32))[None, None, :]
    assert lat.dtype == F32
    in_s = (F32(-5.0) <= x32) & (x32 < F32(10005.0))
    onl = (np.abs(lat) <= F32(2.0 + K["MARGIN"])) & (present & in_s)[:, :, None]
    fr_all, re_all = neighbours(x, onl, K["FRONT_TIE_LAST"], K["REAR_TIE_FIRST"], K["REAR_STRICT"])
    front = np.where(present, _lane_pick(fr_all, lane, L), -1)
    rear = np.where(present, _lane_pick(re_all, lane, L), -1)

    def gap_to(idx, ahead):
        """(x_other - x_i) - LENGTH ahead, (x_i - x_other) - LENGTH behind, float32; +inf for -1"""
        xo = _take(x32, idx)
        xi = x32 if idx.ndim == 2 and idx.shape[1] == V else x32[:, :1]
        d = (xo - xi) if ahead else (xi - xo)
        g = d - length
        assert g.dtype == F32
        return np.where(idx >= 0, g, INF32)

    gap = gap_to(front, True)

    # ---- vx and what follows from it
    spd, h = Q(s["speed"]), Q(s["heading"])
    vx = spd * h.cos() if K["COSINE"] else spd

    def closing_of(a_idx, a_vx, b_idx, b_vx, has):
        """vx_a - vx_b where `has`, exactly 0 between equal (heading, speed) words"""
        c = (a_vx - b_vx) if K["CLOSING_SIGN"] > 0 else (b_vx - a_vx)
        same = (_take(hbits, a_idx) == _take(hbits, b_idx)) & \
               (_take(sbits, a_idx) == _take(sbits, b_idx))
        exact0 = same | ~has
        return Q(np.where(exact0, 0.0, c.v), np.where(exact0, 0.0, c.e))

    me = np.broadcast_to(np.arange(V), (E, V))
    has_f = front >= 0
    closing = closing_of(me, vx, front, _qtake(vx, front), has_f)
    ttc, und_ttc = _ratio(gap, closing)
    thw, und_thw = _ratio(gap, vx)
    risk, und_risk = _risk(ttc, und_ttc, T["risk_horizon"])

    # absent slots: the "none" values
    for q, none in ((closing, 0.0), (ttc, np.inf), (thw, np.inf), (risk, 0.0)):
        q.v = np.where(present, q.v, none)
        q.e = np.where(present, q.e, 0.0)
    gap = np.where(present, gap, INF32)
    out = {
        "front": _pad(front, -1, np.int64), "rear": _pad(rear, -1, np.int64),
        "gap": _pad(gap, INF32, F32), "closing": _qpad(closing, 0.0), "ttc": _qpad(ttc, np.inf),
        "thw": _qpad(thw, np.inf), "risk": _qpad(risk, 0.0), "present": _pad(present, False, bool),
        "und": {"closing": _pad(np.zeros_like(present), False, bool),
                "ttc": _pad(und_ttc & present, False, bool),
                "thw": _pad(und_thw & present, False, bool),
                "risk": _pad(und_risk & present, False, bool)},
    }

    # ---- the ego row
    z = np.zeros((E, 1), np.int64)
    e_rear = rear[:, :1]
    rgap = gap_to(e_rear, False)[:, 0]
    rclos = closing_of(e_rear, _qtake(vx, e_rear), z, vx[:, :1], e_rear >= 0)
    rttc, und_rttc = _ratio(rgap[:, None], rclos)
    eln = lane[:, 0]
    side_f = np.stack([_lane_pick(fr_all[:, :1], (eln + d)[:, None], L)[:, 0] for d in (-1, 1)], 1)
    side_r = np.stack([_lane_pick(re_all[:, :1], (eln + d)[:, None], L)[:, 0] for d in (-1, 1)], 1)
    others = present.copy()
    others[:, 0] = False
    dx, dy = x32 - x32[:, :1], y32 - y32[:, :1]
    d2 = dx * dx + dy * dy
    assert d2.dtype == F32
    dist = np.sqrt(np.where(others, d2, INF32).min(1, initial=INF32)).astype(F32)
    near = (others & (F32(0.0) <= dx) & (dx <= F32(T["near_range"]))).sum(1).astype(F32)
    off = y32[:, 0] - st[_abi.F_LANE][:, 0].astype(np.int32).astype(F32) * F32(4.0)
    assert off.dtype == F32
    out["ego_exact"] = {
        4: rgap, 7: gap_to(side_f[:, :1], True)[:, 0], 8: gap_to(side_r[:, :1], False)[:, 0],
        9: gap_to(side_f[:, 1:], True)[:, 0], 10: gap_to(side_r[:, 1:], False)[:, 0],
        11: dist, 12: near, 13: off,
    }
    out["ego"] = {0: Q(gap[:, 0].astype(np.float64)), 1: closing[:, 0], 2: ttc[:, 0],
                  3: thw[:, 0], 5: rclos[:, 0], 6: rttc[:, 0], 14: vx[:, 0], 15: risk[:, 0]}
    no = np.zeros(E, bool)
    out["ego_und"] = {0: no, 1: no, 2: und_ttc[:, 0], 3: und_thw[:, 0], 5: no,
                      6: und_rttc[:, 0], 14: no, 15: und_risk[:, 0]}
    out["side"] = (side_f, side_r)
    return out


def undecided_share(m):
    """the share of present (env, vehicle) entries with an undecided output"""
    u = m["und"]["ttc"] | m["und"]["thw"] | m["und"]["risk"]
    n = int(m["present"].sum())
    return float((u & m["present"]).sum()) / max(n, 1)


def within(got, q):
    """got (float32 array) against Q: equal where the bound is 0 (inf included), else within
    TOL_FACTOR times the bound -> bool array"""
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        close = np.abs(got - q.v) <= TOL_FACTOR * q.e
    return np.where(q.e > 0, close, got == q.v)


def compare(m, got, what=""):
    """a kernel's (or the model's own) outputs `got` -- a dict of numpy arrays by hwy_traffic's
    names, `ego` [E, 16] included -- against the model m; returns a list of failures"""
    bad = []

    def note(name, ok, keep=None):
        ok = np.asarray(ok)
        if keep is not None:
            ok = ok | ~keep
        if not ok.all():
            at = np.argwhere(~ok)[0].tolist()
            bad.append(f"{what}{name}: {int((~ok).sum())} wrong, first at {at}")

    if "front" in got:
        note("front", got["front"] == m["front"])
    if "rear" in got:
        note("rear", got["rear"] == m["rear"])
    if "gap" in got:
        note("gap", np.asarray(got["gap"], F32).view(np.uint32) == m["gap"].view(np.uint32))
    for k in ("closing", "ttc", "thw", "risk"):
        if k in got:
            note(k, within(got[k], m[k]), ~m["und"][k])
    if "ego" in got:
        ego = np.asarray(got["ego"], F32)
        for slot, want in m["ego_exact"].items():
            note(f"ego[{slot}]", ego[:, slot].view(np.uint32) == want.view(np.uint32))
        for slot, q in m["ego"].items():
            note(f"ego[{slot}]", within(ego[:, slot], q), ~m["ego_und"][slot])
    return bad


def state_row(ego, has_front, ttc_thresh=DEFAULTS["ttc_thresh"], thw_thresh=DEFAULTS["thw_thresh"]):
    """what one state contributes to acc, [E, 8] float32, from the kernel's own ego row [E, 16]
    and the ego's `front` >= 0"""
    ego = np.asarray(ego, F32)
    one, zero = F32(1.0), F32(0.0)
    return np.stack([np.full(len(ego), one), ego[:, 2], ego[:, 3], ego[:, 0], ego[:, 11],
                     np.where(ego[:, 2] < F32(ttc_thresh), one, zero),
                     np.where(ego[:, 3] < F32(thw_thresh), one, zero),
                     np.where(has_front, one, zero)], 1).astype(F32)


def fold(acc, row, restart):
    """(acc', ep_stats): the running reduction of include/hwy.h on float32 [E, 8] arrays.  A
    marked env flushes its old row to ep_stats and restarts from `row`; a row with n = 0 starts
    from `row` without a flush; otherwise minima for slots 1-4 and sums for 0, 5, 6, 7."""
    acc, row = np.asarray(acc, F32), np.asarray(row, F32)
    restart = np.asarray(restart, bool)
    ep = np.where(restart[:, None], acc, F32(0.0)).astype(F32)
    fresh = restart | (acc[:, 0] == 0)
    merged = acc + row
    merged[:, 1:5] = np.minimum(acc[:, 1:5], row[:, 1:5])
    assert merged.dtype == F32
    return np.where(fresh[:, None], row, merged).astype(F32), ep
