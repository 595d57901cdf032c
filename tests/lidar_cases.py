"""Hand-stated states for hwy_lidar with their expected outputs written out, not computed by the
model: shared by the model's test (CPU) and the kernel's (GPU).

Every case is one env of one state (CASE_NAMES gives the env order) on the shipped config with 12
traffic slots (V = 13) and 4 lanes; the V = 1 case has a config of its own (V1_*).  Unless a case
says otherwise the ego drives at (100, 4), heading 0, 20 m/s, every car has heading 0 and 20 m/s,
and the lidar is L: 4 cells of one ray each, 50 m, not normalised, no ego tail -- cell 0 looks
along +x, cell 1 along +y, cell 2 along -x, cell 3 along -y.  A car is 5 m long and 2 m wide.

A case states `cells` {cell: (vehicle, distance, relative radial speed)}; every other cell has no
return: (-1, range_m, +0.0).  `bodies`: the present others; `dropped`: the dropped cells; `seen`
and the other counts follow from `cells`.  `tol`: 0 (the default) where every stated value is
what float32 gives exactly -- the unaligned ray 0 has the direction (1, 0) exactly and a
heading-0 body the axes (1, 0), (0, 1) exactly, so cell 0 of such cases is exact arithmetic on
the stated numbers -- else 1e-4 (metres, m/s): the other rays' directions carry the device
sin / cos error of 2e-7, which at 50 m and 40 m/s is 1e-5, an order below.  The dropout and noise
cases quote their Philox draws (tests/rng_model.py gives them; tests/test_lidar_model.py checks
the quotes against it), for the seed 1000 + env and step 0 that hand_state writes.
"""

from __future__ import annotations

import math

import numpy as np

from env_util import _put
from hwy import _abi
from hwy._abi import LidarSpec
from parity_util import make_cfg

P, CRASHED = _abi.FLAG_PRESENT, _abi.FLAG_CRASHED
NAN, INF = math.nan, math.inf
UP1 = float(np.nextafter(np.float32(1.0), np.float32(2.0)))        # 1 + 2^-23
UP152 = float(np.nextafter(np.float32(152.5), np.float32(200.0)))  # 152.5 + 2^-16

_BASE = dict(cells=4, sub=1, range_m=50.0, normalize=False, ego_tail=False, pad_to=1)
L = LidarSpec(**_BASE)
L_ALIGN = LidarSpec(**{**_BASE, "align": True})
L_SUB = LidarSpec(**{**_BASE, "sub": 4})
L_NORM = LidarSpec(**{**_BASE, "normalize": True, "speed_scale": 25.0})
L_TAIL = LidarSpec(**{**_BASE, "ego_tail": True, "pad_to": 8})
L_DROP = LidarSpec(**{**_BASE, "sub": 2, "p_drop": 0.5, "salt": 3})
L_NOISE = LidarSpec(**{**_BASE, "sigma_r": 0.5, "salt": 4})

EGO = (100.0, 4.0, 0.0, 20.0)
S33 = math.sin(math.radians(33.75))

# the quoted draws: env index, spec -> per cell the dropout uniform hm_u01(w(0)[0]) and the noise
# sigma_r * z of w(1), as float32 (filled in from rng_model once; test_lidar_model re-derives them)
DROP_U = {}    # case name -> 4 uniforms
NOISE = {}     # case name -> 4 float32 additions

# name -> dict(spec, ego (x, y, heading, speed), cars {k: (x, y[, heading[, speed[, flags]]])},
#              cells {cell: (vehicle, dist, vel)}, bodies, dropped, tol, tail)
CASES = {
    # a car dead ahead, its centre 20 m on: the rear bumper is 17.5 m away; it pulls away at 5 m/s
    "ahead": dict(spec=L, cars={1: (120.0, 4.0, 0.0, 25.0)}, cells={0: (1, 17.5, 5.0)}, bodies=1),
    # a slower car behind: it falls back, so the range grows at 5 m/s along the ray (-1, 0)
    "behind": dict(spec=L, cars={1: (80.0, 4.0, 0.0, 15.0)}, cells={2: (1, 17.5, 5.0)}, bodies=1,
                   tol=1e-4),
    # a faster car alongside, one lane to the left: its flank is 3 m away; it gains along x, not
    # along the ray (0, 1)
    "alongside": dict(spec=L, cars={1: (100.0, 8.0, 0.0, 22.0)}, cells={1: (1, 3.0, 0.0)},
                      bodies=1, tol=1e-4),
    # two cars in line: the far one (the lower index) returns nothing
    "in-line": dict(spec=L, cars={1: (140.0, 4.0), 2: (120.0, 4.0, 0.0, 23.0)},
                    cells={0: (2, 17.5, 3.0)}, bodies=2),
    # ray 0 runs along the body's flank, dw == 0: ow = ye - y_k = 1.0 exactly is inside ...
    "graze-inside": dict(spec=L, ego=(100.0, 1.0, 0.0, 20.0), cars={1: (120.0, 0.0)},
                         cells={0: (1, 17.5, 0.0)}, bodies=1),
    # ... and ow = 1 + 2^-23, one float above it, is not
    "graze-outside": dict(spec=L, ego=(100.0, UP1, 0.0, 20.0), cars={1: (120.0, 0.0)},
                          cells={}, bodies=1),
    # the rear bumper exactly at range_m counts: the distance equals a cell without a return's,
    # the vehicle and the speed tell them apart ...
    "range-exact": dict(spec=L, cars={1: (152.5, 4.0, 0.0, 25.0)}, cells={0: (1, 50.0, 5.0)},
                        bodies=1),
    # ... and one float beyond it (d = 50 + 2^-16) does not
    "range-beyond": dict(spec=L, cars={1: (UP152, 4.0, 0.0, 25.0)}, cells={}, bodies=1),
    # the ego's centre inside a body (2 m behind its centre, half a metre beside): every ray
    # starts inside it, distance 0
    "overlap": dict(spec=L, cars={1: (102.0, 4.5)},
                    cells={c: (1, 0.0, 0.0) for c in range(4)}, bodies=1),
    # a cleared present flag: 1 is not there and does not occlude 2
    "absent": dict(spec=L, cars={1: (120.0, 4.0, 0.0, 20.0, 0), 2: (140.0, 4.0)},
                   cells={0: (2, 37.5, 0.0)}, bodies=1),
    # a set flag in lane 20 >= V means nothing
    "lane-past-V": dict(spec=L, cars={20: (120.0, 4.0)}, cells={}, bodies=0),
    # non-finite positions return nothing and occlude nothing
    "non-finite": dict(spec=L, cars={1: (NAN, 4.0), 2: (INF, 4.0), 3: (110.0, NAN),
                                     4: (120.0, 4.0), 5: (-INF, 4.0)},
                       cells={0: (4, 17.5, 0.0)}, bodies=5),
    # a crashed car is a body like any other
    "crashed": dict(spec=L, cars={1: (120.0, 4.0, 0.0, 0.0, P | CRASHED)},
                    cells={0: (1, 17.5, -20.0)}, bodies=1),
    # the ego heads along +y and the lidar is aligned: cell 0 looks along +y, where a car 20 m on
    # shows its flank at 19 m; the ego moves at (0, 20), the car at (20, 0): along (0, 1) the range
    # closes at 20 m/s.  Unaligned, the return would be in cell 1
    "align-turned": dict(spec=L_ALIGN, ego=(100.0, 4.0, math.pi / 2, 20.0),
                         cars={1: (100.0, 24.0)}, cells={0: (1, 19.0, -20.0)}, bodies=1, tol=1e-4),
    # four sub-rays per cell at -33.75, -11.25, 11.25 and 33.75 degrees about the cell's centre:
    # only the last of cell 0 meets the car at (110, 10.5), on its right flank y = 9.5, 5.5 m to
    # the ego's left: 5.5 / sin(33.75 deg) along the ray; the cell's centre direction meets nothing
    "sub-off-centre": dict(spec=L_SUB, cars={1: (110.0, 10.5)}, cells={0: (1, 5.5 / S33, 0.0)},
                           bodies=1, tol=1e-4),
    # two cars in the same place: equal distances, the lower index wins (its speed shows which)
    "tie": dict(spec=L, cars={3: (120.0, 4.0, 0.0, 30.0), 2: (120.0, 4.0, 0.0, 25.0)},
                cells={0: (2, 17.5, 5.0)}, bodies=2),
    # normalised: 17.5 / 50 and 5 / 25; a cell without a return is (1, 0)
    "normalised": dict(spec=L_NORM, cars={1: (120.0, 4.0, 0.0, 25.0)},
                       cells={0: (1, float(np.float32(17.5) / np.float32(50.0)),
                                  float(np.float32(5.0) / np.float32(25.0)))}, bodies=1),
    # the ego tail: the shipped row x, y, vx, vy of the ego, absolute and normalised: x = 100 and
    # vx = 30 map to 1, y = 0 and vy = 0 to 0; 8 + 4 floats, then four of padding
    "ego-tail": dict(spec=L_TAIL, ego=(100.0, 0.0, 0.0, 30.0), cars={1: (120.0, 0.0, 0.0, 30.0)},
                     cells={0: (1, 17.5, 0.0)}, bodies=1, tail=(1.0, 0.0, 1.0, 0.0)),
    # dropout with p = 0.5 on two sub-rays per cell, the ego inside a body so that every cell
    # would return 0 m: the cells whose quoted uniform is below 0.5 are written as no return
    "dropout": dict(spec=L_DROP, cars={1: (102.0, 4.5)}, cells="from DROP_U", bodies=1),
    # range noise of 0.5 m: cell 0's distance moves by its quoted addition
    "noise": dict(spec=L_NOISE, cars={1: (120.0, 4.0, 0.0, 25.0)}, cells="from NOISE", bodies=1),
    # the range test is on the true distance: a return exactly at range_m stays one whatever the
    # noise, and its noisy distance is clipped to range_m
    "noise-at-range": dict(spec=L_NOISE, cars={1: (152.5, 4.0, 0.0, 25.0)}, cells="from NOISE",
                           bodies=1),
}
CASE_NAMES = list(CASES)

# ---- the quoted draws (hm_u01 of word 0 of channel 0; sigma_r * z of channel 1), per cell
# (a None: a cell without a return, whose draw no stated value depends on)
DROP_U["dropout"] = (0.42310911417007446, 0.1220504641532898, 0.8252717852592468,
                     0.3395809531211853)
NOISE["noise"] = (0.03939530998468399, None, None, None)
NOISE["noise-at-range"] = (0.5377745628356934, None, None, None)


def _resolve():
    u = DROP_U["dropout"]
    CASES["dropout"]["dropped"] = tuple(c for c in range(4) if u[c] < 0.5)
    CASES["dropout"]["cells"] = {c: (1, 0.0, 0.0) for c in range(4) if not u[c] < 0.5}
    add = np.float32(NOISE["noise"][0])
    CASES["noise"]["cells"] = {0: (1, float(np.float32(17.5) + add), 5.0)}
    add = np.float32(NOISE["noise-at-range"][0])
    far = min(max(np.float32(50.0) + add, np.float32(0.0)), np.float32(50.0))
    CASES["noise-at-range"]["cells"] = {0: (1, float(far), 5.0)}


_resolve()
SPECS = list(dict.fromkeys(c["spec"] for c in CASES.values()))

# the V = 1 case: no traffic slot at all; a flagged word in lane 1 means nothing
V1_SPEC = L
V1_CASE = dict(spec=L, cars={1: (120.0, 4.0)}, cells={}, bodies=0)


def hand_cfg(**kw):
    return make_cfg(E=len(CASES), vehicles_count=12, **kw)


def v1_cfg(**kw):
    return make_cfg(E=1, vehicles_count=0, **kw)


def _lane(y):
    """a lane word inside the road for any y (the lidar does not read it)"""
    return min(3, max(0, int(round(y / 4.0)))) if math.isfinite(y) else 0


def _write(st, e, case):
    x, y, h, spd = case.get("ego", EGO)
    _put(st, e, 0, x, y, heading=h, speed=spd, lane=_lane(y))
    for k, car in case["cars"].items():
        car = tuple(car) + (0.0, 20.0, P)[len(car) - 2:]
        _put(st, e, k, car[0], car[1], heading=car[2], speed=car[3], lane=_lane(car[1]),
             flags=car[4])
    st[_abi.F_ENV][e, _abi.E_SEED_LO] = 1000 + e


def hand_state(cfg):
    """[NFIELDS, len(CASES), 64] uint32: env i holds the i-th case"""
    st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
    for e, name in enumerate(CASE_NAMES):
        _write(st, e, CASES[name])
    return st


def v1_state(cfg):
    st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
    _write(st, 0, V1_CASE)
    return st


def check_case(case, e, F, obs=None, hit_vehicle=None, seen=None, counts=None, what=""):
    """env `e` of the outputs of `case`'s spec (a name of CASES or a case dict; full [E, ...]
    arrays, any of them None) is what the case states; F: the handle's n_features"""
    name = case if isinstance(case, str) else "V=1"
    case = CASES[case] if isinstance(case, str) else case
    spec = case["spec"]
    n, tol = spec.cells, case.get("tol", 0.0)
    tag = f"{what}hand case {name!r} (env {e}): "
    stated = case["cells"]
    if hit_vehicle is not None:
        want = np.full(n, -1, np.int32)
        for c, (k, _, _) in stated.items():
            want[c] = k
        got = np.asarray(hit_vehicle).reshape(-1, n)[e]
        assert np.array_equal(got, want), f"{tag}hit_vehicle {got.tolist()}, stated {want.tolist()}"
    if seen is not None:
        want = np.zeros(64, np.float32)
        for k, _, _ in stated.values():
            want[k] = 1.0
        got = np.asarray(seen, np.float32).reshape(-1, 64)[e]
        assert np.array_equal(got, want), (f"{tag}seen {np.flatnonzero(got).tolist()}, stated "
                                           f"{np.flatnonzero(want).tolist()}")
    if counts is not None:
        want = (case["bodies"], len({k for k, _, _ in stated.values()}), len(stated),
                len(case.get("dropped", ())))
        got = tuple(int(v) for v in np.asarray(counts).reshape(-1, 4)[e])
        assert got == want, f"{tag}counts {got}, stated {want}"
    if obs is not None:
        stride = spec.stride(F)
        got = np.asarray(obs, np.float32).reshape(-1, stride)[e]
        none = (np.float32(1.0), np.float32(0.0)) if spec.normalize else (
            np.float32(spec.range_m), np.float32(0.0))
        for c in range(n):
            d, v = got[2 * c], got[2 * c + 1]
            if c in stated:
                _, wd, wv = stated[c]
                ok = (abs(float(d) - wd) <= tol and abs(float(v) - wv) <= tol) if tol else (
                    d == np.float32(wd) and v == np.float32(wv))
                assert ok, f"{tag}cell {c} is ({d!r}, {v!r}), stated ({wd!r}, {wv!r}) +- {tol}"
            else:
                assert (d, v) == none and not np.signbit(v), (
                    f"{tag}cell {c} is ({d!r}, {v!r}), stated no return {none}")
        rest = np.zeros(stride - 2 * n, np.float32)
        if spec.ego_tail:
            rest[:F] = case["tail"]
        tail = got[2 * n:]
        assert np.array_equal(tail.view(np.uint32), rest.view(np.uint32)), (
            f"{tag}the entries after the cells are {tail.tolist()}, stated {rest.tolist()}")


def ego_into_traffic(cfg, state, rng, heading=0.3, lateral=3.0):
    """A copy of a natural `state` with every env's ego moved into its traffic: 6 m behind a
    present other vehicle drawn by `rng`, at a lateral offset drawn from +-`lateral` metres and a
    heading drawn from +-`heading`, both continuous -- grid_cases.ego_into_traffic puts the ego
    exactly one metre off a lane centre, where the axis-parallel rays of an unaligned lidar graze
    every car of that lane exactly.  On natural states the ego drives alone most of the time,
    which leaves a lidar nearly without returns.  An env without traffic keeps its ego."""
    st = np.array(state, np.uint32)
    V = cfg.vehicles_count + 1
    X, Y, H = (st[k].view(np.float32) for k in (_abi.F_X, _abi.F_Y, _abi.F_HEADING))
    for e in range(st.shape[1]):
        others = 1 + np.flatnonzero((st[_abi.F_FLAGS][e, 1:V] & P) != 0)
        if len(others):
            k = int(rng.choice(others))
            X[e, 0] = X[e, k] - np.float32(6.0)
            Y[e, 0] = Y[e, k] + np.float32(rng.uniform(-lateral, lateral))
            H[e, 0] = np.float32(rng.uniform(-heading, heading))
    return st
