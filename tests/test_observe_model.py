"""tests/observe_model.py (the row -> vehicle map of hwy_observe) against the CPU oracle, by an
identification that shares nothing with the model: under an absolute, un-normalised copy of the
config a row's x and y are the stored words of the vehicle it shows.

Inputs: five configs, each stored as `sorted` and as `shuffled`, each state viewed in both
orders; 16 envs x 24 steps of parity_util.policy_actions (rng seed 3) with autoreset, plus the
crafted states of observe_util.  env_model.uncertain may leave out at most 1 % of the cases."""

from __future__ import annotations

import numpy as np
import pytest

import env_model as em
import observe_model as om
import observe_util as ou
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import make_cfg, policy_actions

E, STEPS = 16, 24


def trajectories():
    """(name, cfg, state) after every step of every (config, stored order)"""
    for name, kw in ou.CONFIGS.items():
        for stored in ou.VIEWS:
            cfg = make_cfg(E=E, order=stored, **kw)
            ora = OracleEnv(cfg)
            ora.reset()
            rng = np.random.default_rng(3)
            for t in range(STEPS):
                ora.step(policy_actions(rng, E, t))
                yield f"{name}/{stored}/step{t}", cfg, ora.state.copy()


def crafted():
    for stored in ou.VIEWS:
        for kw in ({}, dict(observation={"see_behind": True})):
            cfg = ou.craft_cfg(stored, **kw)
            yield f"crafted/{stored}/{'behind' if kw else 'ahead'}", cfg, ou.craft(cfg)


@pytest.fixture(scope="module")
def trial():
    out = {}
    for source, gen in (("trajectories", trajectories), ("crafted", crafted)):
        s = dict(cases=0, rows=0, empty=0, left_out=0, resets=0, bad=[],
                 refused={m: 0 for m in om.MUTATIONS})
        for name, cfg, state in gen():
            keep = ~em.uncertain(cfg, state)
            s["resets"] += int((state[_abi.F_ENV][:, _abi.E_EPISODE] > 0).sum())
            for view in ou.VIEWS:
                ic = om.identity_cfg(cfg, view)
                obs_abs = ou.oracle_observe(ic, state)
                rows = om.row_vehicles(cfg, state, view)
                seen, empty, bad = om.identify(ic, state, rows, obs_abs, keep)
                s["cases"] += int(keep.sum())
                s["left_out"] += int((~keep).sum())
                s["rows"] += seen
                s["empty"] += empty
                s["bad"] += [(name, view) + b for b in bad]
                for m in om.MUTATIONS:
                    wrong = om.row_vehicles(cfg, state, view, mut=m)
                    s["refused"][m] += len(om.identify(ic, state, wrong, obs_abs, keep)[2]) > 0
        out[source] = s
    return out


def test_the_model_identifies_every_row_of_the_oracles_observation(trial):
    s = trial["trajectories"]
    print(f"cases {s['cases']} left out {s['left_out']} rows {s['rows']} empty {s['empty']} "
          f"mismatches {len(s['bad'])} env-states past an autoreset {s['resets']}")
    assert not s["bad"], s["bad"][:5]
    total = s["cases"] + s["left_out"]
    assert total == 5 * 2 * 2 * E * STEPS == 7680
    assert s["left_out"] <= 0.01 * total
    assert s["left_out"] == 0, "these inputs sit on no rounding edge"
    assert s["rows"] == 138240
    assert 0 < s["empty"] < s["rows"]
    assert s["resets"] > 0, "no autoreset in the trajectories"


def test_the_model_on_the_crafted_states(trial):
    s = trial["crafted"]
    assert not s["bad"], s["bad"][:5]
    assert s["left_out"] == 0 and s["cases"] == 2 * 2 * 2 * ou.E_CRAFT
    cfg = ou.craft_cfg("shuffled")
    st = ou.craft(cfg)
    rows = om.row_vehicles(cfg, st, "sorted")
    ou.check_crafted_map(rows)
    assert list(rows[4]) == [0, 8, 5, 2, 10], "the four nearest of ten, by |dx|"
    behind = om.row_vehicles(ou.craft_cfg("sorted", observation={"see_behind": True}), st)
    assert list(behind[3]) == [0, 9, 2, 1, -1], "see_behind admits the car 20 m back"
    # `shuffled` admits the first N - 1 by index (the same vehicles where no more are in reach)
    # and moves empty slots along with the full ones; among envs 4..7 only the step word differs
    sh = om.row_vehicles(cfg, st)
    for e in range(ou.E_CRAFT):
        want = sorted(rows[e, 1:]) if e < 4 else [1, 2, 3, 4]
        assert sorted(sh[e, 1:]) == want and sh[e, 0] == 0
    assert len({tuple(sh[e]) for e in (4, 5, 6, 7)}) > 1
    moved = False
    for t in range(8):   # env 3: two full slots, two empty ones
        r = om.row_vehicles(cfg, _at_step(st, t))[3, 1:]
        moved |= int((r < 0).argmax()) < int(np.nonzero(r >= 0)[0].max())
    assert moved, "an empty slot never moved ahead of a full one"


def _at_step(st, t):
    st = st.copy()
    st[_abi.F_ENV][:, _abi.E_STEP] = t
    return st


@pytest.mark.parametrize("mut", om.MUTATIONS)
def test_each_deliberate_mistake_is_refused(trial, mut):
    n = trial["trajectories"]["refused"][mut] + trial["crafted"]["refused"][mut]
    print(f"{mut}: refused on {n} (state, view) cases")
    assert n > 0, f"no case tells the model with '{mut}' from the model"


def test_scatter_model():
    rv = np.array([[0, 3, -1, 5], [0, -1, -1, 63]])
    vals = np.array([[1.5, -2.0, 9.0, -0.0], [np.nan, 7.0, 8.0, -1.0]], np.float32)
    out = om.scatter(rv, vals)
    assert out.shape == (2, 64) and out.dtype == np.uint32
    f = out.view(np.float32)
    assert f[0, 0] == 1.5 and f[0, 3] == -2.0 and out[0, 5] == 0x80000000
    assert np.isnan(f[1, 0]) and f[1, 63] == -1.0
    mask = np.ones((2, 64), bool)
    mask[0, [0, 3, 5]] = mask[1, [0, 63]] = False
    assert not out[mask].any(), "an entry no row shows is +0.0"
