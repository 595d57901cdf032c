"""A numpy restatement of hwy_grid's rule (include/hwy.h), independent of the kernel.

Plain numpy on the packed state [NFIELDS, E, 64] that hwy_export_state (or the oracle) hands out,
one env and one vehicle at a time.  It shares no code with csrc/.

Without ``align`` every quantity that decides a cell is a correctly rounded float32 operation on
stored words and exact constants -- the subtraction of the ego's position, the subtraction of the
origin, the division by the step, floor -- and numpy's float32 gives the very same bits.  So the
cell of every vehicle, the winner, cell_vehicle, veh_cell, counts and the presence, x, y, heading
and on_road values are exact (bound 0: compared bit for bit).

With ``align`` the rotation goes through hm_sincosf, which differs from libm in the last bits.
The model rotates in float64 with libm and carries a derived bound: for u = dx c + dy s

    |u_device - u| <= (|dx| + |dy|) SINCOS_ABS            the device's sin / cos (env_model.py)
                    + U (|dx c| + |dy s|) + U |u|         two products and a sum, each rounded

and then the subtraction of the origin and the division add U |u - x0| / step and U |q|.  The
comparison allows env_model's TOL_FACTOR times that.  A vehicle whose qx or qy lies within that
of an integer 0..n (and which the other axis does not already put outside) is *undecided*, with
every cell it may be in; the on_road entry of a cell whose rotated centre lies within the bound
of one of the road's four limits likewise.  Undecided entries are left out of a comparison.

vx, vy, cos_h and sin_h go through env_model's Q with the bounds it derives for those features
(a layer value of the ego itself is the exact +0.0 of v - v and is held exact).

``mistake`` turns one deliberate misreading of the rule on (tests/test_grid_model.py).
"""

from __future__ import annotations

import numpy as np

import env_model as em
from hwy import _abi
from hwy._abi import GridSpec

F32 = np.float32
MISTAKES = ("highest_wins", "edge_lower", "layout_chw", "absolute", "rot_sign", "no_ego",
            "absent_drawn", "no_clip", "corner_centre")
EXACT_LAYERS = ("presence", "x", "y", "heading", "on_road")
RELATIVE = ("x", "y", "vx", "vy")


def _lmap32(v, lo, hi):
    """hm_lmap(v, lo, hi, -1, 1) in float32, operation by operation"""
    v, lo, hi = F32(v), F32(lo), F32(hi)
    return F32(-1.0) + ((v - lo) * (F32(1.0) - F32(-1.0))) / (hi - lo)


def _clip32(v):
    return F32(-1.0) if v < F32(-1.0) else (F32(1.0) if v > F32(1.0) else v)


def _feature_q(name, x, y, h, spd):
    """Vehicle.to_dict's entry as an env_model.Q (scalars)"""
    xq, yq, hq, sq = (em.Q(float(v)) for v in (x, y, h, spd))
    return {"presence": em.Q(1.0), "x": xq, "y": yq, "vx": sq * hq.cos(), "vy": sq * hq.sin(),
            "cos_h": hq.cos(), "sin_h": hq.sin(), "heading": hq}[name]


def _value(name, veh, ego, rng, clip, relative, is_ego):
    """(value, tolerance) of a layer / tail entry.  veh, ego: (x, y, h, spd) float32; rng: (lo,
    hi) or None; relative: subtract the ego's value.  Tolerance 0 means bit for bit."""
    exact = name in EXACT_LAYERS or (relative and is_ego)
    if exact:
        if name == "presence":
            v = F32(1.0)
        elif relative and is_ego:
            v = F32(0.0)  # v - v of identical bits (a non-finite ego aside: no such case is asked)
        else:
            v = {"x": veh[0], "y": veh[1], "heading": veh[2]}[name]
            if relative:
                v = v - {"x": ego[0], "y": ego[1]}[name]
        if rng is not None:
            v = _lmap32(v, *rng)
            if clip:
                v = _clip32(v)
        return F32(v), 0.0
    q = _feature_q(name, *veh)
    if relative:
        q = q - _feature_q(name, *ego)
    if rng is not None:
        q = em.lmap(q, float(F32(rng[0])), float(F32(rng[1])), -1.0, 1.0)
        if clip:
            q = q.clip(-1.0, 1.0)
    return float(q.v), em.TOL_FACTOR * float(q.e)


class GridOut:
    """the model's outputs for E envs: values, tolerances (0: exact) and what is undecided"""

    def __init__(self, E, ncells, stride):
        self.grid = np.zeros((E, stride), np.float64)
        self.tol = np.zeros((E, stride), np.float64)
        self.skip = np.zeros((E, stride), bool)
        self.cell_vehicle = np.full((E, ncells), -1, np.int32)
        self.cell_skip = np.zeros((E, ncells), bool)
        self.veh_cell = np.full((E, 64), -1, np.int32)
        self.veh_skip = np.zeros((E, 64), bool)
        self.counts = np.zeros((E, 4), np.int32)
        self.counts_skip = np.zeros(E, bool)
        self.pairs = 0       # present (env, vehicle) pairs
        self.undecided = 0   # of them undecided


def _axis(d_along, d_across, c, s, sign, origin, step, n, align, edge_lower):
    """one axis of one vehicle: (q, tolerance, inside, index, undecided, candidate indices)"""
    with np.errstate(all="ignore"):
        if align:
            a, b = float(d_along), float(d_across)
            u = a * c + sign * b * s
            eu = ((abs(a) + abs(b)) * em.SINCOS_ABS + em.U * (abs(a * c) + abs(b * s))
                  + em.U * abs(u))
            q = (u - float(origin)) / float(step)
            tol = em.TOL_FACTOR * ((eu + em.U * abs(u - float(origin))) / float(step)
                                   + em.U * abs(q))
        else:
            q, tol = (F32(d_along) - origin) / step, 0.0
    if not np.isfinite(q):
        return q, tol, False, 0, False, []
    if edge_lower:
        inside = bool(q > 0 and q <= n)
        i = int(np.ceil(q)) - 1
    else:
        inside = bool(q >= 0 and q < n)
        i = int(np.floor(q))
    r = float(np.rint(q))
    und = bool(align and 0 <= r <= n and abs(float(q) - r) <= tol)
    cand = {i} if inside else set()
    if und:
        cand |= {int(r) - 1, int(r)}
    return q, tol, inside, i, und, sorted(k for k in cand if 0 <= k < n)


def grid_model(cfg, state, spec, mistake=None) -> GridOut:
    assert mistake is None or mistake in MISTAKES, mistake
    spec = GridSpec.from_dict(spec)
    state = np.asarray(state).view(np.uint32)
    E, V, F = state.shape[1], cfg.vehicles_count + 1, cfg.n_features
    nx, ny, ncells = spec.nx, spec.ny, spec.nx * spec.ny
    width, stride = spec.width(F), spec.stride(F)
    x0, y0, sx, sy = F32(spec.x0), F32(spec.y0), F32(spec.step_x), F32(spec.step_y)
    X, Y, H, S = (state[k].view(np.float32) for k in (_abi.F_X, _abi.F_Y, _abi.F_HEADING,
                                                       _abi.F_SPEED))
    present = (state[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0
    if mistake == "absent_drawn":
        present[:, :V] = True
    present[:, V:] = False
    ranges = dict(spec.ranges)
    clip = spec.clip and mistake != "no_clip"
    sign = -1.0 if mistake == "rot_sign" else 1.0
    out = GridOut(E, ncells, stride)

    def at(layer, i, j):
        if mistake == "layout_chw":
            return layer * ncells + j * nx + i
        return layer * ncells + i * ny + j

    for e in range(E):
        ego = (X[e, 0], Y[e, 0], H[e, 0], S[e, 0])
        c, s = float(np.cos(np.float64(ego[2]))), float(np.sin(np.float64(ego[2])))
        with np.errstate(all="ignore"):
            dx, dy = X[e] - ego[0], Y[e] - ego[1]  # float32, correctly rounded
        cell_of, und_cells = {}, set()
        for k in range(V):
            if not present[e, k] or (k == 0 and mistake == "no_ego"):
                continue
            out.pairs += 1
            _, _, in_x, i, und_x, cand_x = _axis(dx[k], dy[k], c, s, sign, x0, sx, nx, spec.align,
                                                 mistake == "edge_lower")
            _, _, in_y, j, und_y, cand_y = _axis(dy[k], dx[k], c, s, -sign, y0, sy, ny, spec.align,
                                                 mistake == "edge_lower")
            und = (und_x and (in_y or und_y)) or (und_y and (in_x or und_x))
            if und:
                out.undecided += 1
                out.veh_skip[e, k] = True
                und_cells |= {a * ny + b for a in cand_x for b in cand_y}
            elif in_x and in_y:
                cell_of[k] = i * ny + j
                out.veh_cell[e, k] = i * ny + j
        for k in sorted(cell_of, reverse=(mistake != "highest_wins")):
            out.cell_vehicle[e, cell_of[k]] = k  # the last writer is the least index
        for cc in und_cells:
            out.cell_skip[e, cc] = True
        others = [k for k in range(1, V) if present[e, k]]
        ins = [k for k in others if k in cell_of]
        out.counts[e] = (len(others), len(ins),
                         sum(out.cell_vehicle[e, cell_of[k]] != k for k in ins),
                         len(others) - len(ins))
        out.counts_skip[e] = bool(out.veh_skip[e, 1:].any())

        for layer, name in enumerate(spec.layers):
            if name == "on_road":
                _on_road(out, e, layer, at, cfg, spec, ego, c, s, sign, mistake)
                continue
            for cc in range(ncells):
                i, j = divmod(cc, ny)
                k = out.cell_vehicle[e, cc]
                if out.cell_skip[e, cc]:
                    out.skip[e, at(layer, i, j)] = True
                elif k >= 0:
                    v, tol = _value(name, (X[e, k], Y[e, k], H[e, k], S[e, k]), ego,
                                    ranges.get(name), clip,
                                    name in RELATIVE and mistake != "absolute", k == 0)
                    out.grid[e, at(layer, i, j)], out.tol[e, at(layer, i, j)] = v, tol
        if spec.ego_tail:
            base = len(spec.layers) * ncells
            for f in range(F):
                name = next(n for n, fid in _abi.FEATURES.items() if fid == int(cfg.feature_ids[f]))
                rng = ((cfg.features_range[f][0], cfg.features_range[f][1])
                       if cfg.normalize and cfg.has_range[f] else None)
                v, tol = _value(name, ego, ego, rng, bool(cfg.clip), False, True)
                out.grid[e, base + f], out.tol[e, base + f] = v, tol
        assert not out.grid[e, width:].any()
    return out


def _on_road(out, e, layer, at, cfg, spec, ego, c, s, sign, mistake):
    half = F32(0.0 if mistake == "corner_centre" else 0.5)
    x0, y0, sx, sy = F32(spec.x0), F32(spec.y0), F32(spec.step_x), F32(spec.step_y)
    y_hi = 4.0 * cfg.lanes_count - 2.0
    for i in range(spec.nx):
        for j in range(spec.ny):
            gx = x0 + (F32(i) + half) * sx   # float32, correctly rounded
            gy = y0 + (F32(j) + half) * sy
            if spec.align:
                a, b = float(gx), float(gy)
                rx, ry = a * c - sign * b * s, sign * a * s + b * c
                er = (abs(a) + abs(b)) * em.SINCOS_ABS
                ex_ = er + em.U * (abs(a * c) + abs(b * s)) + em.U * abs(rx)
                ey_ = er + em.U * (abs(a * s) + abs(b * c)) + em.U * abs(ry)
                Xc, Yc = float(ego[0]) + rx, float(ego[1]) + ry
                tx = em.TOL_FACTOR * (ex_ + em.U * abs(Xc))
                ty = em.TOL_FACTOR * (ey_ + em.U * abs(Yc))
                if (min(abs(Xc), abs(Xc - em.ROAD_LENGTH)) <= tx
                        or min(abs(Yc + 2.0), abs(Yc - y_hi)) <= ty):
                    out.skip[e, at(layer, i, j)] = True
                    continue
            else:
                Xc, Yc = ego[0] + gx, ego[1] + gy  # float32
            on = 0.0 <= Xc <= em.ROAD_LENGTH and -2.0 <= Yc < y_hi
            out.grid[e, at(layer, i, j)] = 1.0 if on else 0.0


def compare(model: GridOut, got, what=""):
    """every output of `got` (a dict of numpy arrays by hwy_grid_args' names; a missing one is
    not compared) against the model: bit for bit where the bound is 0, within it elsewhere,
    undecided entries left out"""
    E = model.grid.shape[0]
    if got.get("grid") is not None:
        g = np.asarray(got["grid"], np.float32).reshape(E, -1)
        assert g.shape == model.grid.shape, (g.shape, model.grid.shape)
        exact = (model.tol == 0) & ~model.skip
        want = model.grid.astype(np.float32)
        bad = exact & (g.view(np.uint32) != want.view(np.uint32))
        assert not bad.any(), (f"{what}grid differs where the model is exact, first at (env, entry) "
                               f"{tuple(np.argwhere(bad)[0])}: got {g[bad][0]!r}, model {want[bad][0]!r}")
        near = ~exact & ~model.skip
        with np.errstate(invalid="ignore"):
            off = near & ~(np.abs(g.astype(np.float64) - model.grid) <= model.tol)
        assert not off.any(), (f"{what}grid outside the model's bound, first at (env, entry) "
                               f"{tuple(np.argwhere(off)[0])}: got {g[off][0]!r}, model "
                               f"{model.grid[off][0]!r} +- {model.tol[off][0]!r}")
    for name, want, skip in (("cell_vehicle", model.cell_vehicle, model.cell_skip),
                             ("veh_cell", model.veh_cell, model.veh_skip),
                             ("counts", model.counts, model.counts_skip[:, None])):
        if got.get(name) is None:
            continue
        a = np.asarray(got[name]).reshape(E, -1)
        bad = (a != want) & ~skip
        assert not bad.any(), (f"{what}{name} differs, first at (env, entry) "
                               f"{tuple(np.argwhere(bad)[0])}: got {a[bad][0]}, model "
                               f"{np.broadcast_to(want, a.shape)[bad][0]}")
