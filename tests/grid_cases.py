"""Hand-stated states for hwy_grid with their expected outputs written out, not computed: shared
by the model's test (CPU) and the kernel's (GPU).

Every case is one env of one state (CASE_NAMES gives the env order) on the shipped config with 12
traffic slots (V = 13) and 4 lanes.  Unless a case says otherwise the ego drives at (100, 4),
heading 0, 20 m/s, and the grid is G: 4 x 3 cells of 10 m x 4 m from (-10, -6), so the cells'
lower edges are dx = -10, 0, 10, 20 and dy = -6, -2, 2, and the ego sits in cell (1, 1) = flat 4.
G's layers are presence, x in [-64, 64], y (no range) and vx in [-32, 32], clipped: with those
ranges lmap is exact on the values used, x -> dx / 64, vx -> dvx / 32.

A case states: the winners {(i, j): vehicle} (every other cell is -1), veh_cell {vehicle: flat}
(every other vehicle is -1), counts, and per won cell the value of every vehicle layer (every
other cell of a vehicle layer is +0.0); `on_road`: the cells of the on_road layer that are 1.0;
`tail`: the ego tail.
"""

from __future__ import annotations

import math

import numpy as np

from env_util import _put
from hwy import _abi
from hwy._abi import GridSpec
from parity_util import make_cfg

P, CRASHED = _abi.FLAG_PRESENT, _abi.FLAG_CRASHED
NAN, INF = math.nan, math.inf
PI32 = float(np.float32(math.pi))                       # 3.14159274, just above pi
BELOW_PI = float(np.nextafter(np.float32(PI32), np.float32(0)))  # 3.14159250, just below pi


def _down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


_GEO = dict(nx=4, ny=3, x0=-10.0, y0=-6.0, step_x=10.0, step_y=4.0, ego_tail=False, pad_to=1)
_R = {"x": (-64.0, 64.0), "vx": (-32.0, 32.0)}
G = GridSpec(layers=("presence", "x", "y", "vx"), ranges=_R, **_GEO)
G_NOCLIP = GridSpec(layers=("presence", "x", "y", "vx"), ranges=_R, clip=False, **_GEO)
G_X0 = GridSpec(layers=("presence", "x", "y", "vx"), ranges=_R, **{**_GEO, "x0": 0.0})
G_AHEAD = GridSpec(layers=("presence", "x", "y", "vx"), ranges=_R, **{**_GEO, "x0": 10.0})
# the aligned cases' grid starts at dx = -15, so that the ego (u = 0) is in the middle of cell 1
G_ALIGN = GridSpec(layers=("presence", "x", "y"), ranges={"x": (-64.0, 64.0)}, align=True,
                   **{**_GEO, "x0": -15.0})
# cell centres at dx = -15, -5, 5, 15 and dy = -4, 0, 4; the ego in cell (2, 1) = flat 7
G_ROAD = GridSpec(layers=("presence", "on_road"), **{**_GEO, "x0": -20.0})
G_ONE = GridSpec(layers=("presence",), nx=1, ny=1, x0=-5.0, y0=-2.0, step_x=10.0, step_y=4.0,
                 ego_tail=False, pad_to=1)
# the shipped config's row is x, y, vx, vy in [-100, 100]^2 x [-30, 30]^2: 48 + 4 floats, padded to 56
G_TAIL = GridSpec(layers=("presence", "x", "y", "vx"), ranges=_R, **{**_GEO, "ego_tail": True,
                                                                      "pad_to": 8})

EGO = (100.0, 4.0, 0.0, 20.0)
EGO_ROW = (1.0, 0.0, 0.0, 0.0)   # the ego's own entries: presence and three +0.0
ALL_ROAD = {(i, j) for i in range(4) for j in range(3)}

# name -> dict(spec, ego (x, y, heading, speed), cars {k: (x, y[, heading[, speed[, flags]]])},
#              cells, veh_cell, counts, values {(i, j): per vehicle layer}, on_road, tail)
CASES = {
    # 1 and 2 share cell (2, 1): the lower index wins wherever it stands
    "shared-low-nearer": dict(
        spec=G, cars={1: (112.0, 4.0), 2: (116.0, 5.0)},
        cells={(1, 1): 0, (2, 1): 1}, veh_cell={0: 4, 1: 7, 2: 7}, counts=(2, 2, 1, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.1875, 0.0, 0.0)}),
    "shared-low-farther": dict(
        spec=G, cars={2: (116.0, 5.0, 0.0, 28.0), 5: (112.0, 4.0)},
        cells={(1, 1): 0, (2, 1): 2}, veh_cell={0: 4, 2: 7, 5: 7}, counts=(2, 2, 1, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.25, 1.0, 0.25)}),
    # dx = 10 and dy = 2 lie on edges: each belongs to the upper cell
    "shared-edge": dict(
        spec=G, cars={1: (110.0, 4.0), 2: (100.0, 6.0)},
        cells={(1, 1): 0, (2, 1): 1, (1, 2): 2}, veh_cell={0: 4, 1: 7, 2: 5}, counts=(2, 2, 0, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.15625, 0.0, 0.0), (1, 2): (1.0, 0.0, 2.0, 0.0)}),
    # x0 = 0, the ego at x = +0.0 and vehicle 1 at x = -0.0: dx = -0.0, u - x0 = -0.0, inside cell
    # 0; vehicle 2 a hair below it is outside
    "minus-zero": dict(
        spec=G_X0, ego=(0.0, 4.0, 0.0, 20.0), cars={1: (-0.0, 8.0), 2: (-2.0 ** -100, 4.0)},
        cells={(0, 1): 0, (0, 2): 1}, veh_cell={0: 1, 1: 2}, counts=(2, 1, 0, 1),
        values={(0, 1): EGO_ROW, (0, 2): (1.0, 0.0, 4.0, 0.0)}),
    # dx = 30 = x0 + nx step is outside; one float below it (dx = 30 - 2^-16) is in the last cell
    "upper-edge": dict(
        spec=G, cars={1: (130.0, 4.0), 2: (_down(130.0), 4.0)},
        cells={(1, 1): 0, (3, 1): 2}, veh_cell={0: 4, 2: 10}, counts=(2, 1, 0, 1),
        values={(1, 1): EGO_ROW, (3, 1): (1.0, 0.46875 - 2.0 ** -22, 0.0, 0.0)}),
    # the grid starts 10 m ahead: the ego is outside its own grid and wins nothing
    "ego-outside": dict(
        spec=G_AHEAD, cars={1: (125.0, 4.0)},
        cells={(1, 1): 1}, veh_cell={1: 4}, counts=(1, 1, 0, 0),
        values={(1, 1): (1.0, 0.390625, 0.0, 0.0)}),
    # non-finite positions are outside; 5 shares the ego's cell and loses it
    "non-finite": dict(
        spec=G, cars={1: (NAN, 4.0), 2: (INF, 4.0), 3: (-INF, 4.0), 4: (110.0, NAN),
                      5: (105.0, 4.0), 6: (105.0, INF)},
        cells={(1, 1): 0}, veh_cell={0: 4, 5: 4}, counts=(6, 1, 1, 5),
        values={(1, 1): EGO_ROW}),
    # a cleared present flag: 1 is not there; 2 is
    "absent": dict(
        spec=G, cars={1: (112.0, 4.0, 0.0, 20.0, 0), 2: (125.0, 4.0)},
        cells={(1, 1): 0, (3, 1): 2}, veh_cell={0: 4, 2: 10}, counts=(1, 1, 0, 0),
        values={(1, 1): EGO_ROW, (3, 1): (1.0, 0.390625, 0.0, 0.0)}),
    # a set flag in lane 20 >= V means nothing
    "lane-past-V": dict(
        spec=G, cars={20: (112.0, 4.0)},
        cells={(1, 1): 0}, veh_cell={0: 4}, counts=(0, 0, 0, 0), values={(1, 1): EGO_ROW}),
    # a crashed vehicle is still drawn
    "crashed": dict(
        spec=G, cars={1: (112.0, 4.0, 0.0, 20.0, P | CRASHED)},
        cells={(1, 1): 0, (2, 1): 1}, veh_cell={0: 4, 1: 7}, counts=(1, 1, 0, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.1875, 0.0, 0.0)}),
    # the ego heads along +y: u = dy, w = -dx.  1, 20 m to the ego's front (the road's +y), is in
    # (3, 1) -- unaligned it would be outside; 2, 8 m ahead and 3 m to the ego's left (the road's
    # -x), is in (2, 2) -- with the rotation's sign flipped it would be in (0, 0)
    "align-half-pi": dict(
        spec=G_ALIGN, ego=(100.0, 4.0, math.pi / 2, 20.0), cars={1: (100.0, 24.0), 2: (97.0, 12.0)},
        cells={(1, 1): 0, (3, 1): 1, (2, 2): 2}, veh_cell={0: 4, 1: 10, 2: 8}, counts=(2, 2, 0, 0),
        values={(1, 1): EGO_ROW[:3], (3, 1): (1.0, 0.0, 20.0), (2, 2): (1.0, -0.046875, 8.0)}),
    # the ego heads along -x, its heading next to +pi and next to -pi: u = -dx, w = -dy
    "align-below-pi": dict(
        spec=G_ALIGN, ego=(100.0, 4.0, BELOW_PI, 20.0), cars={1: (80.0, 4.0), 2: (92.0, 1.0)},
        cells={(1, 1): 0, (3, 1): 1, (2, 2): 2}, veh_cell={0: 4, 1: 10, 2: 8}, counts=(2, 2, 0, 0),
        values={(1, 1): EGO_ROW[:3], (3, 1): (1.0, -0.3125, 0.0), (2, 2): (1.0, -0.125, -3.0)}),
    "align-above-minus-pi": dict(
        spec=G_ALIGN, ego=(100.0, 4.0, -BELOW_PI, 20.0), cars={1: (80.0, 4.0), 2: (92.0, 1.0)},
        cells={(1, 1): 0, (3, 1): 1, (2, 2): 2}, veh_cell={0: 4, 1: 10, 2: 8}, counts=(2, 2, 0, 0),
        values={(1, 1): EGO_ROW[:3], (3, 1): (1.0, -0.3125, 0.0), (2, 2): (1.0, -0.125, -3.0)}),
    # the road's start: the centres are at X = -10, 0, 10, 20; X = 0 is on the road
    "road-start": dict(
        spec=G_ROAD, ego=(5.0, 4.0, 0.0, 20.0), cars={},
        cells={(2, 1): 0}, veh_cell={0: 7}, counts=(0, 0, 0, 0), values={(2, 1): (1.0,)},
        on_road={(i, j) for i in (1, 2, 3) for j in range(3)}),
    # the road's end: X = 9980, 9990, 10000, 10010; X = 10000 is on the road
    "road-end": dict(
        spec=G_ROAD, ego=(9995.0, 4.0, 0.0, 20.0), cars={},
        cells={(2, 1): 0}, veh_cell={0: 7}, counts=(0, 0, 0, 0), values={(2, 1): (1.0,)},
        on_road={(i, j) for i in (0, 1, 2) for j in range(3)}),
    # the outer lane lines: Y = -2 is on the road (centres at Y = -2, 2, 6) ...
    "road-first-line": dict(
        spec=G_ROAD, ego=(100.0, 2.0, 0.0, 20.0), cars={},
        cells={(2, 1): 0}, veh_cell={0: 7}, counts=(0, 0, 0, 0), values={(2, 1): (1.0,)},
        on_road=ALL_ROAD),
    # ... and Y = 4 lanes - 2 = 14 is not (centres at Y = 6, 10, 14); a vehicle in an off-road cell
    # does not touch the layer
    "road-last-line": dict(
        spec=G_ROAD, ego=(100.0, 10.0, 0.0, 20.0), cars={1: (105.0, 14.0)},
        cells={(2, 1): 0, (2, 2): 1}, veh_cell={0: 7, 1: 8}, counts=(1, 1, 0, 0),
        values={(2, 1): (1.0,), (2, 2): (1.0,)},
        on_road={(i, j) for i in range(4) for j in (0, 1)}),
    # dvx = 48 maps to 1.5: clipped to 1, or kept
    "clip-on": dict(
        spec=G, cars={1: (112.0, 4.0, 0.0, 68.0)},
        cells={(1, 1): 0, (2, 1): 1}, veh_cell={0: 4, 1: 7}, counts=(1, 1, 0, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.1875, 0.0, 1.0)}),
    "clip-off": dict(
        spec=G_NOCLIP, cars={1: (112.0, 4.0, 0.0, 68.0)},
        cells={(1, 1): 0, (2, 1): 1}, veh_cell={0: 4, 1: 7}, counts=(1, 1, 0, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.1875, 0.0, 1.5)}),
    # one cell from (-5, -2) to (5, 2): 1 is in it and loses it, 2 is past it
    "one-cell": dict(
        spec=G_ONE, cars={1: (103.0, 5.0), 2: (106.0, 4.0)},
        cells={(0, 0): 0}, veh_cell={0: 0, 1: 0}, counts=(2, 1, 1, 1), values={(0, 0): (1.0,)}),
    # the ego tail: the shipped row x, y, vx, vy of the ego, absolute and normalised: x = 100 and
    # vx = 30 map to 1, y = 0 and vy = 0 to 0; then four floats of padding
    "ego-tail": dict(
        spec=G_TAIL, ego=(100.0, 0.0, 0.0, 30.0), cars={1: (112.0, 0.0, 0.0, 30.0)},
        cells={(1, 1): 0, (2, 1): 1}, veh_cell={0: 4, 1: 7}, counts=(1, 1, 0, 0),
        values={(1, 1): EGO_ROW, (2, 1): (1.0, 0.1875, 0.0, 0.0)}, tail=(1.0, 0.0, 1.0, 0.0)),
}
CASE_NAMES = list(CASES)
SPECS = list(dict.fromkeys(c["spec"] for c in CASES.values()))


def hand_cfg(**kw):
    return make_cfg(E=len(CASES), vehicles_count=12, **kw)


def _lane(y):
    """a lane word inside the road for any y (the grid does not read it)"""
    return min(3, max(0, int(round(y / 4.0)))) if math.isfinite(y) else 0


def hand_state(cfg):
    """[NFIELDS, len(CASES), 64] uint32: env i holds the i-th case"""
    st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
    for e, name in enumerate(CASE_NAMES):
        case = CASES[name]
        x, y, h, spd = case.get("ego", EGO)
        _put(st, e, 0, x, y, heading=h, speed=spd, lane=_lane(y))
        for k, car in case["cars"].items():
            car = tuple(car) + (0.0, 20.0, P)[len(car) - 2:]
            _put(st, e, k, car[0], car[1], heading=car[2], speed=car[3], lane=_lane(car[1]),
                 flags=car[4])
        st[_abi.F_ENV][e, _abi.E_SEED_LO] = 1000 + e
    return st


def ego_into_traffic(cfg, state, rng, heading=0.3):
    """A copy of a natural `state` with every env's ego moved into its traffic: 6 m behind and
    1 m beside a present other vehicle drawn by `rng`, at a heading drawn from +-`heading`.  On
    natural states the ego drives alone most of the time (it starts a hundred metres behind the
    traffic and crashes soon after it gets there), which leaves a grid nearly empty; this fills
    it with natural traffic.  An env without traffic keeps its ego."""
    st = np.array(state, np.uint32)
    V = cfg.vehicles_count + 1
    X, Y, H = (st[k].view(np.float32) for k in (_abi.F_X, _abi.F_Y, _abi.F_HEADING))
    for e in range(st.shape[1]):
        others = 1 + np.flatnonzero((st[_abi.F_FLAGS][e, 1:V] & P) != 0)
        if len(others):
            k = int(rng.choice(others))
            X[e, 0], Y[e, 0] = X[e, k] - np.float32(6.0), Y[e, k] + np.float32(1.0)
            H[e, 0] = np.float32(rng.uniform(-heading, heading)) if heading else np.float32(0.0)
    return st


def check_case(name, e, F, grid=None, cell_vehicle=None, veh_cell=None, counts=None, what=""):
    """env `e` of the outputs of CASES[name]'s spec (full [E, ...] arrays, any of them None) is
    what the case states; F: the handle's n_features"""
    case = CASES[name]
    spec = case["spec"]
    nx, ny, ncells = spec.nx, spec.ny, spec.nx * spec.ny
    tag = f"{what}hand case {name!r} (env {e}): "
    if cell_vehicle is not None:
        want = np.full((nx, ny), -1, np.int32)
        for (i, j), k in case["cells"].items():
            want[i, j] = k
        got = np.asarray(cell_vehicle).reshape(-1, nx, ny)[e]
        assert np.array_equal(got, want), f"{tag}cell_vehicle\n{got}\nstated\n{want}"
    if veh_cell is not None:
        want = np.full(64, -1, np.int32)
        for k, c in case["veh_cell"].items():
            want[k] = c
        got = np.asarray(veh_cell).reshape(-1, 64)[e]
        assert np.array_equal(got, want), f"{tag}veh_cell {got.tolist()}, stated {want.tolist()}"
    if counts is not None:
        got = tuple(int(v) for v in np.asarray(counts).reshape(-1, 4)[e])
        assert got == case["counts"], f"{tag}counts {got}, stated {case['counts']}"
    if grid is not None:
        stride = spec.stride(F)
        want = np.zeros(stride, np.float32)
        vehicle_layers = [l for l, n in enumerate(spec.layers) if n != "on_road"]
        for (i, j), vals in case["values"].items():
            assert len(vals) == len(vehicle_layers), name
            for l, v in zip(vehicle_layers, vals):
                want[l * ncells + i * ny + j] = v
        if "on_road" in spec.layers:
            l = spec.layers.index("on_road")
            for (i, j) in case["on_road"]:
                want[l * ncells + i * ny + j] = 1.0
        if spec.ego_tail:
            base = len(spec.layers) * ncells
            want[base:base + F] = case["tail"]
        got = np.asarray(grid, np.float32).reshape(-1, stride)[e]
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert not len(bad), (f"{tag}grid entry {bad[0]} is {got[bad[0]]!r}, stated "
                              f"{want[bad[0]]!r} ({len(bad)} entries differ)")
