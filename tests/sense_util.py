"""Inputs shared by the CPU and the GPU tests of hwy_sense: the hand-stated states with what the
sensor must see in them, the sensors of the trial and the natural states from the oracle."""

from __future__ import annotations

import math

import numpy as np

from env_util import _put
from hwy import _abi
from hwy._abi import SensorModel
from oracle.oracle import OracleEnv
from parity_util import make_cfg, policy_actions

NULL = SensorModel()
LOS = SensorModel(los=True)
RANGE40 = SensorModel(range=40.0)
LOS40 = SensorModel(los=True, range=40.0)
FULL = SensorModel(los=True, range=120.0, dropout=0.2, noise=(0.5, 0.2, 0.4), salt=7)

# natural states: name -> (make_cfg keywords, steps of random actions)
NATURAL = {
    "E1-N2-3cars": (dict(E=1, N=2, vehicles_count=3), 4),
    "E6-N15-50cars": (dict(E=6, N=15), 12),
    "E16-N64-63cars": (dict(E=16, N=64, vehicles_count=63), 8),
    "E6-N15-50cars-shuffled": (dict(E=6, N=15, order="shuffled"), 9),
}


def natural_state(name, **kw):
    """(cfg, state): the oracle's state after the entry's steps of seeded random actions; `kw`
    (a fused wrapper, say) goes into the returned config only: the states do not depend on it,
    and the oracle needs no table"""
    ckw, steps = NATURAL[name]
    cfg = make_cfg(**ckw)
    ora = OracleEnv(cfg)
    ora.reset()
    rng = np.random.default_rng(11)
    for t in range(steps):
        ora.step(policy_actions(rng, cfg.num_envs, t))
    return make_cfg(**{**ckw, **kw}), ora.state.copy()


# ------------------------------------------------------------------------------ hand-stated
def _up(v):
    return float(np.nextafter(np.float32(v), np.float32(np.inf)))


def _down(v):
    return float(np.nextafter(np.float32(v), np.float32(-np.inf)))


# name -> (sensor, ego (x, y), {vehicle: (x, y[, heading[, flags]])}, the visible others).
# Every heading but one is 0 and every coordinate a short binary fraction, so each quantity of the
# rule is exact in binary32 (the model confirms it: no entry is undecided).  Rectangles are 5 x 2,
# so a blocker at (bx, by) covers bx +- 2.5, by +- 1.
HAND = {
    # the leader (1) hides the car ahead of it (2); a car ahead in the next lane (3: the sight
    # line is 2.7 m to the side where it passes 1) and one alongside (4) stay; the absent slot 5
    # between the ego and the leader blocks nothing; 1 is not its own blocker
    "leader": (LOS, (64.0, 8.0), {1: (84.0, 8.0), 2: (110.0, 8.0), 3: (90.0, 12.0), 4: (64.0, 4.0),
                                  5: (74.0, 8.0, 0.0, 0)}, {1, 3, 4}),
    # a blocker across two lanes (x 83..85, y 7.5..12.5) hides 2 and 3 behind it, not 4
    "across": (LOS, (64.0, 8.0), {1: (84.0, 10.0, math.pi / 2), 2: (104.0, 8.0), 3: (104.0, 12.0),
                                  4: (104.0, 0.0)}, {1, 4}),
    # 1 hides 2 (the line passes 0.875 m off 1's centre at its rear), 2 alone hides 3 (the line
    # is 1.2 m off 1, 2.6..2.9 m beside the ego's lane at 2, which covers 1..3): a hidden
    # vehicle still blocks
    "chain": (LOS, (64.0, 8.0), {1: (84.0, 8.0), 2: (104.0, 10.0), 3: (144.0, 13.5)}, {1}),
    # the five inequalities, each one coordinate ulp inside equality (blocked), at equality
    # (blocked) and one ulp past it (not)
    "u-min-at": (LOS, (64.0, 8.0), {1: (61.5, 8.0), 2: (84.0, 8.0)}, {1}),
    "u-min-inside": (LOS, (64.0, 8.0), {1: (_up(61.5), 8.0), 2: (84.0, 8.0)}, {1}),
    "u-min-past": (LOS, (64.0, 8.0), {1: (_down(61.5), 8.0), 2: (84.0, 8.0)}, {1, 2}),
    "u-max-at": (LOS, (64.0, 8.0), {1: (86.5, 8.0), 2: (84.0, 8.0)}, set()),   # 2 hides 1 too
    "u-max-inside": (LOS, (64.0, 8.0), {1: (_down(86.5), 8.0), 2: (84.0, 8.0)}, set()),
    "u-max-past": (LOS, (64.0, 8.0), {1: (_up(86.5), 8.0), 2: (84.0, 8.0)}, {2}),
    "w-min-at": (LOS, (64.0, 8.0), {1: (84.0, 7.0), 2: (104.0, 8.0)}, {1}),
    "w-min-inside": (LOS, (64.0, 8.0), {1: (84.0, _up(7.0)), 2: (104.0, 8.0)}, {1}),
    "w-min-past": (LOS, (64.0, 8.0), {1: (84.0, _down(7.0)), 2: (104.0, 8.0)}, {1, 2}),
    "w-max-at": (LOS, (64.0, 8.0), {1: (84.0, 9.0), 2: (104.0, 8.0)}, {1}),
    "w-max-inside": (LOS, (64.0, 8.0), {1: (84.0, _down(9.0)), 2: (104.0, 8.0)}, {1}),
    "w-max-past": (LOS, (64.0, 8.0), {1: (84.0, _up(9.0)), 2: (104.0, 8.0)}, {1, 2}),
    # the sight line through the corner (2.5, 1) of 1: from (4.5, 0) to (0.5, 2) in 1's frame
    "corner-at": (LOS, (36.5, 8.0), {1: (32.0, 8.0), 2: (32.5, 10.0)}, {1}),
    "corner-inside": (LOS, (_down(36.5), 8.0), {1: (32.0, 8.0), 2: (32.5, 10.0)}, {1}),
    "corner-past": (LOS, (_up(36.5), 8.0), {1: (32.0, 8.0), 2: (32.5, 10.0)}, {1, 2}),
    # range 40 m, no line of sight: at 40 m exactly (ahead, behind, 24 / 32 to the side) a vehicle
    # is in range, one ulp of the distance further it is not, one ulp nearer (9) it is
    "range": (RANGE40, (64.0, 8.0), {1: (104.0, 8.0), 2: (_up(104.0), 8.0), 3: (24.0, 8.0),
                                     4: (24.0 - 2.0 ** -18, 8.0), 5: (88.0, 40.0), 6: (_up(88.0), 40.0),
                                     7: (64.0, _down(-32.0)), 8: (64.0, -32.0),
                                     9: (_down(104.0), 8.0)}, {1, 3, 5, 8, 9}),
    # a body out of range still blocks: 1 (41.5 m away, covering x 103..108) is not seen itself and
    # hides 2 at 39.5 m, whose centre lies under it; 3 beside them at 39 m is seen
    "range-body": (LOS40, (64.0, 8.0), {1: (105.5, 8.0), 2: (103.5, 8.0), 3: (103.0, 12.0)}, {3}),
}
HAND_NAMES = list(HAND)


def _lane(y):
    """a lane word inside the road for any y (the sensor does not read it)"""
    return min(3, max(0, int(round(y / 4.0))))


def hand_cfg(**kw):
    return make_cfg(E=len(HAND), vehicles_count=12, N=5, **kw)


def hand_state(cfg):
    """[NFIELDS, len(HAND), 64] uint32: env i holds HAND's i-th case; every env has its own seed
    words and step word 3"""
    st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
    for e, name in enumerate(HAND_NAMES):
        _, ego, cars, _ = HAND[name]
        _put(st, e, 0, ego[0], ego[1])
        for i, c in cars.items():
            _put(st, e, i, c[0], c[1], heading=c[2] if len(c) > 2 else 0.0, lane=_lane(c[1]),
                 flags=c[3] if len(c) > 3 else _abi.FLAG_PRESENT)
        st[_abi.F_ENV][e, _abi.E_STEP] = 3
        st[_abi.F_ENV][e, _abi.E_SEED_LO] = 1000 + e
        st[_abi.F_ENV][e, _abi.E_SEED_HI] = 7
    return st


def check_hand(visible_of, what=""):
    """visible_of(sensor) -> visible [E, 64]; every HAND case's visible others as stated"""
    cache = {}
    for e, name in enumerate(HAND_NAMES):
        sensor, _, cars, want = HAND[name]
        if sensor not in cache:
            cache[sensor] = np.asarray(visible_of(sensor))
        got = {int(i) for i in np.flatnonzero(cache[sensor][e][1:]) + 1}
        assert got == want, f"{what}hand case {name!r} (env {e}): visible {sorted(got)}, stated {sorted(want)}"
        assert cache[sensor][e][0], f"{what}hand case {name!r}: the ego is not visible"


# vehicles on the 40 m circle around the ego (exactly: 24-32-40 and the axes), for the mistake of
# testing the range on the perceived positions: all are in range whatever the noise
RING = [(40.0, 0.0), (-40.0, 0.0), (0.0, 40.0), (0.0, -40.0), (24.0, 32.0), (-24.0, 32.0),
        (24.0, -32.0), (-24.0, -32.0), (32.0, 24.0), (-32.0, 24.0), (32.0, -24.0), (-32.0, -24.0)]
RING_SENSOR = SensorModel(range=40.0, noise=(1.0, 1.0, 0.0))


def ring_state(cfg):
    st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
    for e in range(cfg.num_envs):
        _put(st, e, 0, 64.0, 8.0)
        for i, (dx, dy) in enumerate(RING, 1):
            _put(st, e, i, 64.0 + dx, 8.0 + dy, lane=_lane(8.0 + dy))
        st[_abi.F_ENV][e, _abi.E_STEP] = e
        st[_abi.F_ENV][e, _abi.E_SEED_LO] = 77
    return st
