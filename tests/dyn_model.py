"""One simulation frame of the env's dynamics in float64 numpy: the second restatement.

`frame_model(cfg, state_before, actions)` restates what one frame of the step does to the packed
state [NFIELDS, E, 64]: the ego's action, the neighbour search and IDM
(a1.2), MOBIL with the abort rule (a1.3), the lateral control (a1.4), `Vehicle.step` with
`clip_actions` (a1.5) and `handle_collisions` (a1.6), with the constants of DESIGN.md §4's table.
It takes nothing from csrc/hwy_math.h and does not load the oracle; where the documents leave a
point open the reading is the one DESIGN.md §4 lists under "readings taken from the oracle's
comments".  With sim_freq == policy_freq a step is exactly this frame, so the test compares the
after-state with the model of the step's own before-state: no drift enters.

It is vectorised over the envs and over the vehicles.  Upstream's Road.act is sequential, but the
only word one vehicle's act writes that a later vehicle's act reads is the target lane (in the
abort scan), so MOBIL, IDM and the steering are evaluated for all vehicles at once and only the
target lanes are resolved in a loop over the vehicles in list order.

Values follow upstream's own forms: the asin / atan(2 tan .) steering chain, beta = atan(tan
delta / 2), cos / sin of heading + beta, the corner polygons of are_polygons_intersecting.  The
bounds (env_model.Q) follow the operations the build performs, i.e. the closed forms DESIGN.md
lists as deliberate deviations -- so a closed form that left upstream's form would fail here.

Decisions are taken in float64.  One whose margin is within TOL_FACTOR times its own bound marks
the env `uncertain` for the frame; comparisons of two stored float32 words are exact and never
uncertain.
"""

from __future__ import annotations

import numpy as np

import env_model as em
from env_model import Q, TOL_FACTOR, U
from hwy import _abi

# The dynamics constants of DESIGN.md §4's table.  tests/test_dyn_model.py changes each by 1 %
# and requires a case to notice.
CONSTS = dict(
    A_MAX=3.0,            # IDMVehicle.COMFORT_ACC_MAX
    B=5.0,                # -COMFORT_ACC_MIN
    D0=10.0,              # DISTANCE_WANTED = 5 + LENGTH
    T=1.5,                # TIME_WANTED
    ACC_CLIP=6.0,         # IDMVehicle.ACC_MAX
    GAIN=0.2,             # LANE_CHANGE_MIN_ACC_GAIN
    BRAKE=2.0,            # LANE_CHANGE_MAX_BRAKING_IMPOSED
    DELAY=1.0,            # LANE_CHANGE_DELAY
    MARGIN=1.0,           # on_lane margin of Road.neighbour_vehicles
    K_LAT=1.0 / 0.6,      # ControlledVehicle.KP_LATERAL
    K_HEADING=1.0 / 0.2,  # KP_HEADING
    STEER_MAX=np.pi / 3,  # MAX_STEERING_ANGLE
    HALF_L=2.5,           # the bicycle model's L / 2
    SPEED_CLIP=40.0,      # Vehicle.MAX_SPEED = -MIN_SPEED
    LENGTH=5.0,           # the rectangle
    WIDTH=2.0,
    DIAGONAL=float(np.sqrt(29.0)),  # the pre-check's sqrt(LENGTH^2 + WIDTH^2)
    EGO_ACC=5.0,          # ContinuousAction acceleration range
    EGO_STEER=np.pi / 4,  # ContinuousAction steering range
)
LANE_WIDTH, ROAD_LENGTH, LANE_VEH_LEN = em.LANE_WIDTH, em.ROAD_LENGTH, em.VEHICLE_LENGTH
EPS = 1e-2                # utils.not_zero
FLOAT_FIELDS = {"x": _abi.F_X, "y": _abi.F_Y, "heading": _abi.F_HEADING, "speed": _abi.F_SPEED,
                "target_speed": _abi.F_TSPEED, "delta": _abi.F_DELTA, "timer": _abi.F_TIMER,
                "impact_x": _abi.F_IMPX, "impact_y": _abi.F_IMPY}
INT_FIELDS = {"lane": _abi.F_LANE, "target_lane": _abi.F_TLANE}
FLAG_MASK = _abi.FLAG_CRASHED | _abi.FLAG_IMPACT | _abi.FLAG_PRESENT


class _Ctx:
    """collects the envs with a decision on a rounding edge"""

    def __init__(self, E):
        self.E = E
        self.unc = np.zeros(E, bool)
        self.why = {}   # decision -> (env, frame) pairs it left out

    def mark(self, m, why):
        m = np.asarray(m).reshape(self.E, -1).any(1)
        self.unc |= m
        self.why[why] = self.why.get(why, 0) + int(m.sum())

    def lt(self, a, b, rel=True, why="?"):
        """a < b in float64; where it matters (`rel`) and the margin is within the bound of the
        two sides, the env is uncertain.  Two exact operands are never uncertain."""
        a, b = Q.of(a), Q.of(b)
        tol = TOL_FACTOR * (a.e + b.e)
        self.mark((np.abs(a.v - b.v) <= tol) & (tol > 0) & rel, why)
        return a.v < b.v


def _g(a, idx):
    """a [E, V] at the vehicle indices idx [E, ...] (a negative index reads vehicle 0: the
    caller masks it)"""
    ar = np.arange(a.shape[0]).reshape((a.shape[0],) + (1,) * (idx.ndim - 1))
    return a[ar, np.maximum(idx, 0)]


def _qg(q, idx):
    return Q(_g(q.v, idx), _g(q.e, idx))


def _not_zero(x):
    """utils.not_zero on exact values: x if |x| > eps, else eps with x's sign (+ for 0)"""
    return np.where(np.abs(x) > EPS, x, np.where(x >= 0, EPS, -EPS))


def _const(v):
    """a real constant as the float32 the build holds: one rounding"""
    return Q(v, U * abs(v))


def unpack(cfg, st):
    V = cfg.vehicles_count + 1
    f = {k: st[i].view(np.float32)[:, :V].astype(np.float64) for k, i in FLOAT_FIELDS.items()}
    f["lane"] = st[_abi.F_LANE][:, :V].astype(np.int32).astype(np.int64)
    f["target_lane"] = st[_abi.F_TLANE][:, :V].astype(np.int32).astype(np.int64)
    fl = st[_abi.F_FLAGS][:, :V]
    f["crashed"] = (fl & _abi.FLAG_CRASHED) != 0
    f["impact"] = (fl & _abi.FLAG_IMPACT) != 0
    f["present"] = (fl & _abi.FLAG_PRESENT) != 0
    return f


def neighbours(x, onl):
    """Road.neighbour_vehicles for every vehicle i and lane c: (front, rear) [E, V, L] vehicle
    indices, -1 for none.  Candidates are the other vehicles on lane c (`onl` [E, V, L]); front is
    the nearest with s_i <= s_k, the last in list order among equals; rear the nearest with
    s_k < s_i, the first in list order among equals.  The s are stored words: exact."""
    E, V, L = onl.shape
    k = np.arange(V)
    other = k[:, None] != k[None, :]
    xk = np.broadcast_to(x[:, None, :], (E, V, V))
    ahead = (xk >= x[:, :, None]) & other
    behind = (xk < x[:, :, None]) & other
    front = np.full((E, V, L), -1, np.int64)
    rear = np.full((E, V, L), -1, np.int64)
    for c in range(L):
        M = ahead & onl[:, None, :, c]
        mn = np.where(M, xk, np.inf).min(-1)
        best = M & (xk == mn[..., None])
        front[:, :, c] = np.where(M.any(-1), V - 1 - np.argmax(best[..., ::-1], -1), -1)
        M = behind & onl[:, None, :, c]
        mx = np.where(M, xk, -np.inf).max(-1)
        best = M & (xk == mx[..., None])
        rear[:, :, c] = np.where(M.any(-1), np.argmax(best, -1), -1)
    return front, rear


def road_order(cfg, st):
    """[E, V] the position of each vehicle in the road order of the state's own positions:
    present vehicles by x ascending (-0 == +0), the higher index first among equals; every
    absent slot of the 64 after them, the higher index first."""
    V = cfg.vehicles_count + 1
    E = st.shape[1]
    x = st[_abi.F_X].view(np.float32).astype(np.float64)
    pres = (st[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    pres[:, V:] = False
    pos = np.zeros((E, 64), np.int64)
    for e in range(E):
        idx = np.nonzero(pres[e])[0]
        order = sorted(idx, key=lambda i: (x[e, i], -i))
        absent = sorted(set(range(64)) - set(idx.tolist()), reverse=True)
        for p, i in enumerate(list(order) + absent):
            pos[e, i] = p
    return pos[:, :V]


def frame_model(cfg, st, actions, consts=None):
    """(state_after, uncertain): state_after maps a field name to Q [E, V] (float fields), to an
    int array [E, V] (`lane`, `target_lane`, `flags` without the order bits), and `ego_acc`,
    `ego_steer` to Q [E] (the stored action words), and `why` to a dict decision -> the number
    of envs it left out; uncertain is [E] bool.  `consts` overrides entries of CONSTS."""
    K = dict(CONSTS, **(consts or {}))
    s = unpack(cfg, st)
    E, V = s["x"].shape
    L = int(cfg.lanes_count)
    ctx = _Ctx(E)
    x, y, h, v = s["x"], s["y"], s["heading"], s["speed"]
    lane, tl0, present, crashed = s["lane"], s["target_lane"], s["present"], s["crashed"]
    idx = np.broadcast_to(np.arange(V), (E, V))
    traffic = present & (idx > 0)
    dt = Q(1.0) / Q(float(cfg.sim_freq))
    lane_c = LANE_WIDTH * np.arange(L)

    # ---- a1.1 the ego's action: clip, two lmaps
    a = np.clip(np.asarray(actions, np.float32).astype(np.float64), -1.0, 1.0)
    ego_acc = em.lmap(Q(a[:, 0]), -1.0, 1.0, -K["EGO_ACC"], K["EGO_ACC"])
    ego_steer = em.lmap(Q(a[:, 1]), -1.0, 1.0, _const(-K["EGO_STEER"]), _const(K["EGO_STEER"]))

    # ---- AbstractLane.on_lane(position, margin) for every vehicle and lane, and the neighbours
    lat = Q(y[:, :, None]) - Q(lane_c)                                    # [E, V, L]
    in_s = ((-LANE_VEH_LEN <= x) & (x < ROAD_LENGTH + LANE_VEH_LEN))[:, :, None]
    rel = np.broadcast_to((present[:, :, None] & in_s), lat.v.shape)
    onl = ~ctx.lt(Q(LANE_WIDTH / 2 + K["MARGIN"]), lat.abs(), rel, "on_lane margin") & rel
    front, rear = neighbours(x, onl)

    ch, sh = Q(h).cos(), Q(h).sin()
    inv2sab = _const(1.0 / (2.0 * np.sqrt(K["A_MAX"] * K["B"])))

    def desired_gap(ev, fv):
        """IDMVehicle.desired_gap(ego, front, projected=True)"""
        va, vb = Q(_g(v, ev)), Q(_g(v, fv))
        ca, sa, cb, sb = _qg(ch, ev), _qg(sh, ev), _qg(ch, fv), _qg(sh, fv)
        dv = (va * ca - vb * cb) * ca + (va * sa - vb * sb) * sa
        return Q(K["D0"]) + va * K["T"] + (va * dv) * inv2sab

    def idm(ev, fv, dl):
        """IDMVehicle.acceleration(ego_vehicle=ev, front_vehicle=fv) under the exponent dl"""
        v0 = np.where(ev == 0, 0.0, np.clip(_g(s["target_speed"], ev), 0.0, float(cfg.speed_limit)))
        base = Q(np.maximum(_g(v, ev), 0.0)) / Q(np.abs(_not_zero(v0)))
        acc = Q(K["A_MAX"]) - Q(K["A_MAX"]) * base.pow(dl)
        if (fv >= 0).any():
            d = Q(_g(x, fv)) - Q(_g(x, ev))
            relv = (ev >= 0) & (fv >= 0)
            small = ~ctx.lt(Q(EPS), d.abs(), relv, "not_zero(d)")
            dz = Q(np.where(small, np.where(d.v >= 0, EPS, -EPS), d.v), np.where(small, 0.0, d.e))
            gq = desired_gap(ev, fv) / dz
            acc = (acc - Q(K["A_MAX"]) * (gq * gq)).where(fv >= 0, acc)
        return Q(np.zeros(ev.shape)).where(ev < 0, acc)

    # ---- a1.3 change_lane_policy: the timer branch (MOBIL), for every traffic vehicle at once
    active = traffic & ~crashed
    changing = active & (lane != tl0)
    fired = active & (lane == tl0) & (K["DELAY"] < s["timer"])
    slow = np.abs(v) < 1.0
    own_front = np.take_along_axis(front, lane[:, :, None], 2)[:, :, 0]
    wish = lane.copy()
    if fired.any():
        self_a = idm(idx, own_front, s["delta"])
        for side in (-1, 1):                      # RoadNetwork.side_lanes: lane - 1, then lane + 1
            c = lane + side
            cc = np.clip(c, 0, L - 1)
            cand = fired & (c >= 0) & (c < L) & ~slow
            if not cand.any():
                continue
            latc = np.take_along_axis(lat.v, cc[:, :, None], 2)[:, :, 0]
            late = np.take_along_axis(lat.e, cc[:, :, None], 2)[:, :, 0]
            reach = ~ctx.lt(Q(2.0 * LANE_WIDTH), Q(np.abs(latc), late), cand, "is_reachable_from")
            reach &= (0.0 <= x) & (x < ROAD_LENGTH + LANE_VEH_LEN)    # is_reachable_from
            cand = cand & reach
            new_front = np.take_along_axis(front, cc[:, :, None], 2)[:, :, 0]
            new_rear = np.take_along_axis(rear, cc[:, :, None], 2)[:, :, 0]
            rear_pred = idm(np.where(cand, new_rear, -1), idx, s["delta"])
            veto = ctx.lt(rear_pred, Q(-K["BRAKE"]), cand, "braking veto")
            cand = cand & ~veto
            self_pred = idm(idx, new_front, s["delta"])
            gain = self_pred - self_a            # politeness 0: the followers' terms drop out
            ok = cand & ~ctx.lt(gain, Q(K["GAIN"]), cand, "MOBIL gain")
            wish = np.where(ok, c, wish)

    # ---- the abort rule and Road.act's order: vehicle i sees the target lanes vehicles before it
    # in the list have already set in this frame
    tl = tl0.copy()
    if changing.any():
        ii, kk = idx[:, :, None], idx[:, None, :]
        d = Q(x[:, None, :]) - Q(x[:, :, None])                          # [E, i, k] lane_distance_to
        dstar = desired_gap(np.broadcast_to(ii, (E, V, V)), np.broadcast_to(kk, (E, V, V)))
    for i in range(1, V):
        ch_i = changing[:, i]
        if ch_i.any():
            who = present & (idx != i) & (idx != 0) & (lane != tl[:, i:i + 1]) & \
                (tl == tl[:, i:i + 1]) & ch_i[:, None]
            if who.any():
                di, dsi = d[:, i, :], dstar[:, i, :]
                inside = (0.0 < di.v) & ctx.lt(di, dsi, who & (0.0 < di.v), "abort d < d*") & who
                tl[:, i] = np.where(inside.any(1), lane[:, i], tl[:, i])
        tl[:, i] = np.where(fired[:, i], wish[:, i], tl[:, i])
    timer = Q(s["timer"]).where(~fired, Q(np.zeros((E, V))))

    # ---- a1.4 steering_control towards the target lane (traffic)
    spd_nz = _not_zero(v)
    inv = Q(1.0) / Q(spd_nz)
    lat_t = Q(y) - Q(LANE_WIDTH * tl)
    q1 = (lat_t * _const(-K["K_LAT"]) * inv).clip_sat(-1.0, 1.0)
    href = q1.asin().clip_sat(-np.pi / 4, np.pi / 4, U * np.pi / 4)
    dh = href - Q(h)
    r = np.mod(dh.v + np.pi, 2.0 * np.pi)                                # utils.wrap_to_pi
    we = dh.e + 4.0 * U * 2.0 * np.pi
    ctx.mark((np.minimum(r, 2.0 * np.pi - r) <= TOL_FACTOR * we) & active, "wrap_to_pi")
    rate = Q(r - np.pi, we) * _const(K["K_HEADING"])
    z = ((Q(K["HALF_L"]) * inv) * rate).clip_sat(-1.0, 1.0)
    steer = np.clip(np.arctan(2.0 * np.tan(np.arcsin(z.v))), -K["STEER_MAX"], K["STEER_MAX"])
    # the bound: the build's 2 z / sqrt((1 - z)(1 + z)) clipped at tan(STEER_MAX).  The clip
    # saturates from |z| = sin(atan(tan(STEER_MAX) / 2)) = 0.655 on; beyond it by more than z's
    # bound (and 1e-5 for the closed form's own roundings) the result is the constant itself,
    # below it the closed form's operations on |z| <= 0.7 give the bound.
    tan_max = np.tan(K["STEER_MAX"])
    z_sat = np.sin(np.arctan(tan_max / 2.0))
    sat = np.abs(z.v) - TOL_FACTOR * z.e > z_sat + 1e-5
    zc = Q(np.clip(z.v, -0.7, 0.7), z.e)
    t_closed = Q(2.0) * (zc / ((Q(1.0) - zc) * (Q(1.0) + zc)).sqrt())
    tan_tr = Q(np.tan(steer), np.where(sat, U * tan_max, t_closed.e + U * tan_max))

    # ---- a1.2 IDMVehicle.act's acceleration
    acc = idm(idx, own_front, s["delta"])
    moving = active & (lane != tl)
    if moving.any():
        tgt_front = np.take_along_axis(front, np.clip(tl, 0, L - 1)[:, :, None], 2)[:, :, 0]
        acc = acc.minimum(idm(idx, np.where(moving, tgt_front, -1), s["delta"])).where(moving, acc)
    acc = acc.clip_sat(-K["ACC_CLIP"], K["ACC_CLIP"])

    # ---- a1.5 Vehicle.step.  clip_actions first
    ego_col = idx == 0
    acc = Q(np.where(ego_col, ego_acc.v[:, None], acc.v), np.where(ego_col, ego_acc.e[:, None], acc.e))
    acc = Q(-v).where(crashed, acc)
    acc = acc.minimum(Q(K["SPEED_CLIP"]) - Q(v)).where(v > K["SPEED_CLIP"], acc)
    acc = acc.maximum(Q(-K["SPEED_CLIP"]) - Q(v)).where(v < -K["SPEED_CLIP"], acc)
    tan_ego = ego_steer.tan()
    tan_d = Q(np.where(ego_col, tan_ego.v[:, None], tan_tr.v), np.where(ego_col, tan_ego.e[:, None], tan_tr.e))
    tan_d = Q(np.zeros((E, V))).where(crashed, tan_d)
    delta_f = np.where(crashed, 0.0, np.where(ego_col, ego_steer.v[:, None], steer))
    # the bound: cos / sin of beta from 1 / sqrt(1 + u^2), of heading + beta by angle addition
    u = tan_d * 0.5
    cb = Q(1.0) / (u * u + 1.0).sqrt()
    sb = u * cb
    vx_b, vy_b = Q(v) * (ch * cb - sh * sb), Q(v) * (sh * cb + ch * sb)
    hr_b = (Q(v) * sb) * (dt * (Q(1.0) / Q(K["HALF_L"])))
    # the values: upstream's beta = atan(tan(delta) / 2)
    beta = np.arctan(0.5 * np.tan(delta_f))
    vx = Q(v * np.cos(h + beta), vx_b.e)
    vy = Q(v * np.sin(h + beta), vy_b.e)
    x1, y1 = Q(x) + vx * dt, Q(y) + vy * dt
    imp = s["impact"] & present
    x1 = (x1 + Q(s["impact_x"])).where(imp, x1)
    y1 = (y1 + Q(s["impact_y"])).where(imp, y1)
    crashed1 = crashed | imp
    h1 = Q(h) + Q(v * np.sin(beta) / K["HALF_L"] * dt.v, hr_b.e)
    v1 = Q(v) + acc * dt
    timer1 = (timer + dt).where(~fired, Q(np.broadcast_to(dt.v, (E, V)), dt.e))
    timer1 = timer1.where(traffic, Q(s["timer"]))
    # on_state_update: the closest lane, the first among equals
    dist = (Q(y1.v[:, :, None], y1.e[:, :, None]) - Q(lane_c)).abs()
    lane1 = np.argmin(dist.v, -1)
    if L > 1:
        two = np.sort(dist.v, -1)[:, :, :2]
        ctx.mark((two[:, :, 1] - two[:, :, 0] <= TOL_FACTOR * 2.0 * dist.e.max(-1)) & present &
                 (y1.e > 0), "closest lane")

    def keep(q, old):
        return q.where(present, Q(old))

    x1, y1, h1, v1 = keep(x1, x), keep(y1, y), keep(h1, h), keep(v1, v)
    lane1 = np.where(present, lane1, lane)
    tl = np.where(present, tl, tl0)

    # ---- a1.6 handle_collisions on the stepped state, pairs i < j in list order
    impx, impy = Q(np.zeros((E, V))), Q(np.zeros((E, V)))
    has_imp = np.zeros((E, V), bool)
    dxm, dym = x1.v[:, None, :] - x1.v[:, :, None], y1.v[:, None, :] - y1.v[:, :, None]
    near = np.sqrt(dxm * dxm + dym * dym) <= K["DIAGONAL"] + np.abs(v1.v[:, :, None]) * dt.v + 0.01
    near &= present[:, :, None] & present[:, None, :] & (idx[:, :, None] < idx[:, None, :])
    pe, pi, pj = np.nonzero(near)                       # lexicographic: upstream's pair order
    if len(pe):
        A = [Q(q.v[pe, pi], q.e[pe, pi]) for q in (x1, y1, h1, v1)]
        B = [Q(q.v[pe, pj], q.e[pe, pj]) for q in (x1, y1, h1, v1)]
        dd = em.norm2(B[0] - A[0], B[1] - A[1])
        thr = _const(K["DIAGONAL"]) + A[3] * dt
        tol = TOL_FACTOR * (dd.e + thr.e)
        close = ~(dd.v > thr.v)
        inter, will, tx, ty, unc_s = _sat(K, A, B, dt)
        unc_s["pre-check radius"] = (np.abs(dd.v - thr.v) <= tol) & (inter | will)  # it decides something
        # `intersecting` only sets `crashed`: between two vehicles that are crashed already it
        # decides nothing.  (An applied impact leaves its pair exactly touching, so that case is
        # the rule after every crash, not the exception.)
        unc_s["SAT intersecting"] &= ~(crashed1[pe, pi] & crashed1[pe, pj])
        for why, m in unc_s.items():
            m = m & (close | (why == "pre-check radius"))
            np.logical_or.at(ctx.unc, pe, m)
            ctx.why[why] = len(set(pe[m].tolist()))
        for p in np.nonzero(close & will)[0]:           # a later pair's impact replaces an earlier
            e_, i_, j_ = pe[p], pi[p], pj[p]
            for q, t in ((impx, tx), (impy, ty)):       # self.impact = t / 2, other.impact = -t / 2
                q.v[e_, i_], q.v[e_, j_] = 0.5 * t.v[p], -0.5 * t.v[p]
                q.e[e_, i_] = q.e[e_, j_] = 0.5 * t.e[p]
            has_imp[e_, i_] = has_imp[e_, j_] = True
        hit = close & inter
        crashed1 = crashed1.copy()
        crashed1[pe[hit], pi[hit]] = True
        crashed1[pe[hit], pj[hit]] = True

    flags = (crashed1 * _abi.FLAG_CRASHED + has_imp * _abi.FLAG_IMPACT +
             present * _abi.FLAG_PRESENT).astype(np.int64)
    flags = np.where(present, flags, st[_abi.F_FLAGS][:, :V].astype(np.int64) & FLAG_MASK)
    out = {"x": x1, "y": y1, "heading": h1, "speed": v1, "target_speed": Q(s["target_speed"]),
           "delta": Q(s["delta"]), "timer": timer1,
           "impact_x": impx.where(present, Q(s["impact_x"])),
           "impact_y": impy.where(present, Q(s["impact_y"])),
           "lane": lane1, "target_lane": tl, "flags": flags,
           # Vehicle.action after clip_actions, which rewrites it
           "ego_acc": acc[:, 0], "ego_steer": Q(np.zeros(E)).where(crashed[:, 0], ego_steer)}
    out["why"] = ctx.why
    return out, ctx.unc


def _sat(K, A, B, dt):
    """utils.are_polygons_intersecting(a.polygon(), b.polygon(), a.velocity * dt, b.velocity * dt)
    on P pairs: (intersecting [P], will_intersect [P], translation x, y Q [P], uncertain [P]).
    The values come from the corner polygons, the bounds from the build's closed form: the
    interval of a rectangle on axis n is centre . n -/+ (L/2 |u . n| + W/2 |v . n|)."""
    hl, hw = K["LENGTH"] / 2.0, K["WIDTH"] / 2.0
    P = len(A[0].v)
    local = np.array([[-hl, -hw], [-hl, hw], [hl, hw], [hl, -hw]])

    def corners(x, y, hd):
        c, s_ = np.cos(hd.v), np.sin(hd.v)
        return np.stack([c[:, None] * local[:, 0] - s_[:, None] * local[:, 1] + x.v[:, None],
                         s_[:, None] * local[:, 0] + c[:, None] * local[:, 1] + y.v[:, None]], -1)

    pa, pb = corners(*A[:3]), corners(*B[:3])                          # [P, 4, 2]
    normals = []
    for poly in (pa, pb):
        nxt = np.roll(poly, -1, 1)
        n = np.stack([-nxt[:, :, 1] + poly[:, :, 1], nxt[:, :, 0] - poly[:, :, 0]], -1)
        normals.append(n / np.linalg.norm(n, axis=-1, keepdims=True))
    n = np.concatenate(normals, 1)                                       # [P, 8, 2]
    proj_a = np.einsum("pkd,pcd->pkc", n, pa)
    proj_b = np.einsum("pkd,pcd->pkc", n, pb)
    min_a, max_a, min_b, max_b = proj_a.min(-1), proj_a.max(-1), proj_b.min(-1), proj_b.max(-1)
    ca, sa, cb, sb = A[2].cos(), A[2].sin(), B[2].cos(), B[2].sin()
    ddx = (A[3] * ca) * dt - (B[3] * cb) * dt
    ddy = (A[3] * sa) * dt - (B[3] * sb) * dt
    vp = n[:, :, 0] * ddx.v[:, None] + n[:, :, 1] * ddy.v[:, None]

    def gap(mn_a, mx_a, mn_b, mx_b):                                     # utils.interval_distance
        return np.where(mn_a < mn_b, mn_b - mx_a, mn_a - mx_b)

    d0 = gap(min_a, max_a, min_b, max_b)
    min_a2 = np.where(vp < 0, min_a + vp, min_a)
    max_a2 = np.where(vp < 0, max_a, max_a + vp)
    d1 = gap(min_a2, max_a2, min_b, max_b)
    # the bound of an interval end, of the swept end and of the centre difference on an axis
    e_n = np.maximum(ca.e, sa.e)[:, None] * np.ones(8)
    e_n[:, 4:] = np.maximum(cb.e, sb.e)[:, None]

    def end_err(x, y, c, s_):
        """an interval end = centre . n -/+ (L/2 |u . n| + W/2 |v . n|) as the build evaluates it
        on ITS axis: the centre's error weighted by the axis, three roundings at the size of
        the products; the two headings' errors and four roundings on the half extent; the sum's
        rounding.  (What the axis' own error does is common to both rectangles: see e_axis.)"""
        px, py = np.abs(x.v)[:, None] * np.abs(n[:, :, 0]), np.abs(y.v)[:, None] * np.abs(n[:, :, 1])
        centre = x.e[:, None] * np.abs(n[:, :, 0]) + y.e[:, None] * np.abs(n[:, :, 1]) + 3.0 * U * (px + py)
        extent = (hl + hw) * (2.0 * (np.maximum(c.e, s_.e)[:, None] + e_n) + 4.0 * U)
        return centre + extent + U * (px + py + hl + hw)

    # the build's axis differs from the model's by e_n a component: on a distance between the
    # two intervals that acts on the centre difference only
    e_axis = (np.abs(A[0].v - B[0].v) + np.abs(A[1].v - B[1].v))[:, None] * e_n
    ea, eb = end_err(A[0], A[1], ca, sa), end_err(B[0], B[1], cb, sb)
    e_vp = (ddx.e + ddy.e)[:, None] + (np.abs(ddx.v) + np.abs(ddy.v))[:, None] * e_n + 3.0 * U * np.abs(vp)
    e0 = ea + eb + e_axis + U * np.abs(d0)
    e1 = e0 + e_vp + U * (np.abs(max_a2) + np.abs(d1))
    t0, t1 = TOL_FACTOR * e0, TOL_FACTOR * e1
    inter = (d0 <= 0).all(1)
    will = (d1 <= 0).all(1)
    unc = {"SAT intersecting": (d0 <= t0).all(1) != (d0 <= -t0).all(1),
           "SAT will intersect": (d1 <= t1).all(1) != (d1 <= -t1).all(1)}
    # the translation: the first axis of the least |distance|, towards a
    k = np.argmin(np.abs(d1), 1)
    ar = np.arange(P)
    cd = n[:, :, 0] * (A[0].v - B[0].v)[:, None] + n[:, :, 1] * (A[1].v - B[1].v)[:, None]
    sign = np.where(cd > 0, 1.0, -1.0)
    tvec = (np.abs(d1) * sign)[:, :, None] * n                           # [P, 8, 2]
    t = tvec[ar, k]
    e_cd = (A[0].e + B[0].e + A[1].e + B[1].e)[:, None] + (np.abs(A[0].v - B[0].v) + np.abs(
        A[1].v - B[1].v))[:, None] * (e_n + 4.0 * U)
    e_t = e1[ar, k] + np.abs(d1[ar, k]) * e_n[ar, k] + U * np.abs(d1[ar, k])
    # another axis as near, whose translation is another vector; or the side test on its edge
    rival = np.abs(d1) - np.abs(d1[ar, k])[:, None] <= t1 + t1[ar, k][:, None]
    # (another vector: one that would use up a quarter of what the comparison allows)
    other_vec = np.abs(tvec - t[:, None, :]).max(-1) > 0.25 * TOL_FACTOR * e_t[:, None]
    near_mins = np.abs(min_a2 - min_b) <= TOL_FACTOR * (ea + eb + e_vp)   # interval_distance's own branch
    unc["SAT axis of least distance"] = (rival & other_vec).any(1) & will
    unc["SAT side of the axis"] = (np.abs(cd[ar, k]) <= TOL_FACTOR * e_cd[ar, k]) & will
    unc["interval_distance branch"] = will & near_mins[ar, k] & \
        (np.abs((max_a2 - min_a2) - (max_b - min_b))[ar, k] > t1[ar, k])
    tx = Q(np.where(will, t[:, 0], 0.0), np.where(will, e_t, 0.0))
    ty = Q(np.where(will, t[:, 1], 0.0), np.where(will, e_t, 0.0))
    return inter, will, tx, ty, unc
