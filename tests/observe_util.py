"""Inputs shared by the CPU and the GPU tests of hwy_observe: the config table, the crafted
states and the oracle's observation of an arbitrary state."""

from __future__ import annotations

import numpy as np

import observe_model as om
from env_util import _clear, _put
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import make_cfg

VIEWS = ("sorted", "shuffled")

# the trial's configs: name -> make_cfg keywords
CONFIGS = {
    "default": {},
    "N30": dict(N=30),
    "2lanes": dict(lanes_count=2),
    "10cars": dict(vehicles_count=10),
    "see_behind": dict(observation={"see_behind": True}),
}


def oracle_observe(cfg, state, table=None):
    """the oracle's observation of `state` under `cfg` (any config of the state's geometry)"""
    ora = OracleEnv(cfg, table)
    ora.state[...] = np.asarray(state).view(np.uint32)
    return ora.observe()


N_CRAFT = 5   # rows of the crafted config: 4 slots
E_CRAFT = 8


def craft_cfg(order="sorted", **kw):
    return make_cfg(E=E_CRAFT, order=order, N=N_CRAFT, **kw)


def craft(cfg):
    """[NFIELDS, 8, 64] uint32: a reset's state words (seeds, episode) with hand-placed vehicles
    around the ego at (5000, 12):
      0  vehicles 3 and 7 at one x (a tie of |dx|: the lower index goes first), 5 nearer
      1  vehicle 2 at a NaN x (never admitted), 4 and 6 behind it in index
      2  absent slots 1, 2, 4 between present 3, 5
      3  two admitted: fewer than N - 1
      4  ten within reach: more than N - 1
      5, 6, 7  env 4's vehicles at step words 1, 7 and 200 (the shuffle depends on the step)
    Every env carries env 4's seed words, so 4..7 differ in the step alone."""
    assert cfg.num_envs == E_CRAFT and cfg.obs_vehicles == N_CRAFT and cfg.vehicles_count >= 12
    ora = OracleEnv(cfg)
    ora.reset()
    st = ora.state.copy()
    _clear(cfg, st)
    for e in range(E_CRAFT):
        _put(st, e, 0, 5000.0, 12.0)
    _put(st, 0, 7, 5030.0, 8.0)
    _put(st, 0, 3, 5030.0, 4.0)
    _put(st, 0, 5, 5012.0, 12.0)
    _put(st, 0, 9, 5090.0, 0.0)
    _put(st, 1, 2, float("nan"), 12.0)
    _put(st, 1, 4, 5040.0, 8.0)
    _put(st, 1, 6, 5020.0, 4.0)
    _put(st, 2, 3, 5060.0, 12.0)
    _put(st, 2, 5, 5015.0, 8.0)
    _put(st, 3, 1, 5100.0, 12.0)
    _put(st, 3, 2, 5050.0, 0.0)
    _put(st, 3, 8, 5300.0, 4.0)     # beyond 200 m
    _put(st, 3, 9, 4980.0, 4.0)     # more than 10 m behind (admitted only with see_behind)
    for e in (4, 5, 6, 7):
        for i in range(1, 11):
            _put(st, e, i, 5000.0 + 17.0 * ((i * 7) % 11) + 0.25 * i, 4.0 * (i % 4))
    ew = st[_abi.F_ENV]
    ew[:, _abi.E_SEED_LO], ew[:, _abi.E_SEED_HI] = ew[4, _abi.E_SEED_LO], ew[4, _abi.E_SEED_HI]
    ew[:, _abi.E_STEP] = 0
    for e, step in ((5, 1), (6, 7), (7, 200)):
        ew[e, _abi.E_STEP] = step
    return st


def check_crafted_map(rows_sorted):
    """what the crafted states' `sorted` map must be, stated by hand (see_behind off)"""
    want = {0: [0, 5, 3, 7, 9], 1: [0, 6, 4, -1, -1], 2: [0, 5, 3, -1, -1], 3: [0, 2, 1, -1, -1]}
    for e, w in want.items():
        assert list(rows_sorted[e]) == w, f"crafted env {e}: {list(rows_sorted[e])} != {w}"


def identify_with_oracle(cfg, state, rows, view, keep=None):
    """om.identify of `rows` against the oracle's observation under the identity config"""
    ic = om.identity_cfg(cfg, view)
    return om.identify(ic, state, rows, oracle_observe(ic, state), keep)
