"""The numpy model of hwy_grid (tests/grid_model.py) against the hand-stated cases
(tests/grid_cases.py), each deliberate misreading of the rule against them, and how much of a
natural aligned grid the model leaves undecided."""

from __future__ import annotations

import numpy as np
import pytest

import grid_cases as gc
import grid_model as gm
from hwy._abi import GridSpec
from oracle.oracle import OracleEnv
from parity_util import make_cfg

CFG = gc.hand_cfg()
STATE = gc.hand_state(CFG)


def _check_all(mistake=None):
    """every hand case against the model (with `mistake`); the names of the cases that fail"""
    outs = {spec: gm.grid_model(CFG, STATE, spec, mistake) for spec in gc.SPECS}
    failed = []
    for e, name in enumerate(gc.CASE_NAMES):
        m = outs[gc.CASES[name]["spec"]]
        try:
            assert not (m.skip[e].any() or m.cell_skip[e].any() or m.veh_skip[e].any()
                        or m.counts_skip[e]), f"hand case {name!r} has undecided entries"
            gc.check_case(name, e, CFG.n_features, grid=m.grid, cell_vehicle=m.cell_vehicle,
                          veh_cell=m.veh_cell, counts=m.counts)
        except AssertionError as err:
            if mistake is None:
                raise
            failed.append((name, str(err).splitlines()[0]))
    return failed


def test_there_are_enough_hand_cases_and_every_spec_is_used():
    assert len(gc.CASES) >= 16 and len(gc.SPECS) >= 7
    assert any(c["spec"].align for c in gc.CASES.values())
    assert any("on_road" in c["spec"].layers for c in gc.CASES.values())


def test_model_passes_the_hand_cases():
    assert _check_all() == []


@pytest.mark.parametrize("mistake", gm.MISTAKES)
def test_each_deliberate_mistake_fails_a_hand_case(mistake):
    failed = _check_all(mistake)
    print(f"{mistake}: fails {[n for n, _ in failed]}")
    assert failed, f"no hand case notices the mistake {mistake!r}"


def test_exact_without_align_bounded_with_it():
    m = gm.grid_model(CFG, STATE, gc.G)
    # presence, x, y are exact; vx carries env_model's bound, except the ego's own +0.0
    n = gc.G.nx * gc.G.ny
    assert not m.tol[:, :3 * n].any() and m.tol[:, 3 * n:].any()
    assert m.undecided == 0 and m.pairs > len(gc.CASES)
    assert gm.grid_model(CFG, STATE, gc.G_ROAD).tol.max() == 0.0


@pytest.mark.parametrize("lanes", [2, 4])
def test_natural_aligned_states_leave_at_most_one_percent_undecided(lanes):
    """16 envs x 40 steps of random actions, 50 traffic vehicles, the default grid aligned: the
    share of present (env, vehicle) pairs the model cannot decide is at most 1 %.  Each state is
    taken twice: as it is, where the ego mostly drives alone, and with the ego moved into the
    traffic at a random heading (grid_cases.ego_into_traffic), where the grid is full."""
    cfg = make_cfg(E=16, vehicles_count=50, lanes_count=lanes, seed_base=7)
    ora = OracleEnv(cfg)
    ora.reset()
    rng = np.random.default_rng(3)
    spec = GridSpec(align=True, layers=("presence", "vx", "vy", "on_road"))
    pairs = undecided = inside = 0
    for t in range(40):
        a = np.tanh(rng.normal(size=(16, 2)) * np.array([0.6, 0.3])).astype(np.float32)
        ora.step(a)
        if t % 4 == 3:  # every fourth state: ten states, twice 8,160 pairs
            for st in (ora.state, gc.ego_into_traffic(cfg, ora.state, rng)):
                m = gm.grid_model(cfg, st, spec)
                pairs, undecided = pairs + m.pairs, undecided + m.undecided
                inside += int(m.counts[~m.counts_skip, 1].sum())
    share = undecided / pairs
    print(f"lanes {lanes}: {undecided} of {pairs} pairs undecided ({100 * share:.3f} %), "
          f"{inside} others inside a grid")
    assert pairs >= 2 * 16 * 10 * 20 and inside >= 16 * 10 and share <= 0.01
