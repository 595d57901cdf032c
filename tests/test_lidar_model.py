"""The numpy model of hwy_lidar (tests/lidar_model.py) against the hand-stated cases
(tests/lidar_cases.py), each deliberate misreading of the rule against them, and how much of a
natural lidar the model leaves undecided."""

from __future__ import annotations

import numpy as np
import pytest

import lidar_cases as lc
import lidar_model as lm
import rng_model as rm
from hwy._abi import LidarSpec
from oracle.oracle import OracleEnv
from parity_util import make_cfg

CFG = lc.hand_cfg()
STATE = lc.hand_state(CFG)


def _check_all(mistake=None):
    """every hand case against the model (with `mistake`); the names of the cases that fail"""
    outs = {spec: lm.lidar_model(CFG, STATE, spec, mistake) for spec in lc.SPECS}
    failed = []
    for e, name in enumerate(lc.CASE_NAMES):
        m = outs[lc.CASES[name]["spec"]]
        try:
            assert not (m.skip[e].any() or m.cell_skip[e].any() or m.seen_skip[e].any()
                        or m.counts_skip[e].any()), f"hand case {name!r} has undecided entries"
            lc.check_case(name, e, CFG.n_features, obs=m.obs.astype(np.float32),
                          hit_vehicle=m.hit_vehicle, seen=m.seen, counts=m.counts)
        except AssertionError as err:
            if mistake is None:
                raise
            failed.append((name, str(err).splitlines()[0]))
    return failed


def test_there_are_enough_hand_cases_and_mistakes():
    assert len(lc.CASES) + 1 >= 16 and len(lc.SPECS) >= 7 and len(lm.MISTAKES) >= 8
    assert any(c["spec"].align for c in lc.CASES.values())
    assert any(c["spec"].sub > 1 for c in lc.CASES.values())


def test_model_passes_the_hand_cases():
    assert _check_all() == []
    cfg = lc.v1_cfg()
    m = lm.lidar_model(cfg, lc.v1_state(cfg), lc.V1_SPEC)
    assert m.undecided == 0
    lc.check_case(lc.V1_CASE, 0, cfg.n_features, obs=m.obs.astype(np.float32),
                  hit_vehicle=m.hit_vehicle, seen=m.seen, counts=m.counts)


@pytest.mark.parametrize("mistake", lm.MISTAKES)
def test_each_deliberate_mistake_fails_a_hand_case(mistake):
    failed = _check_all(mistake)
    print(f"{mistake}: fails {[n for n, _ in failed]}")
    assert failed, f"no hand case notices the mistake {mistake!r}"


def test_the_quoted_draws_are_philox_s():
    """the uniforms and noise additions lidar_cases quotes, from rng_model alone: counter (cell,
    step 0, channel, 'LIDA' + salt), key (1000 + env, 0)"""
    def word(cell, channel, salt, seed):
        return rm.philox4x32_10(np.array([cell, 0, channel, (0x4C494441 + salt) & 0xFFFFFFFF],
                                         np.uint64), np.array([seed, 0], np.uint64))

    def u01(w):
        return np.float32(int(w) >> 8) * np.float32(2.0 ** -24)

    for name, quoted in lc.DROP_U.items():
        e, salt = lc.CASE_NAMES.index(name), lc.CASES[name]["spec"].salt
        for c, q in enumerate(quoted):
            assert q is None or np.float32(q) == u01(word(c, 0, salt, 1000 + e)[0]), (name, c)
    for name, quoted in lc.NOISE.items():
        e, spec = lc.CASE_NAMES.index(name), lc.CASES[name]["spec"]
        for c, q in enumerate(quoted):
            if q is None:
                continue
            u = [u01(x) for x in word(c, 1, spec.salt, 1000 + e)]
            z = (((u[0] + u[1]) + (u[2] + u[3])) - np.float32(2.0)) * np.float32(1.7320508)
            assert np.float32(q) == np.float32(spec.sigma_r) * z, (name, c)
    u = lc.DROP_U["dropout"]
    assert any(v < 0.5 for v in u) and any(v >= 0.5 for v in u)
    assert lc.NOISE["noise-at-range"][0] > 0  # else the range test after the noise shows nothing


def test_exact_where_the_directions_are_exact():
    """the unaligned ray 0 against heading-0 bodies: bound 0; the other cells carry one"""
    m = lm.lidar_model(CFG, STATE, lc.L)
    e = lc.CASE_NAMES.index("ahead")
    assert m.tol[e, 0] == 0 and m.tol[e, 1] == 0
    e = lc.CASE_NAMES.index("behind")
    assert m.tol[e, 4] > 0 and m.tol[e, 4] < 1e-4


def natural_states(lanes):
    """16 envs x 40 steps of random actions on 50 traffic vehicles, every fourth state, each as it
    is and with the ego moved into its traffic (lidar_cases.ego_into_traffic): 20 states"""
    cfg = make_cfg(E=16, vehicles_count=50, lanes_count=lanes, seed_base=7)
    ora = OracleEnv(cfg)
    ora.reset()
    rng = np.random.default_rng(3)
    states = []
    for t in range(40):
        a = np.tanh(rng.normal(size=(16, 2)) * np.array([0.6, 0.3])).astype(np.float32)
        ora.step(a)
        if t % 4 == 3:
            states += [np.array(ora.state), lc.ego_into_traffic(cfg, ora.state, rng)]
    return cfg, states


# (spec fields, every n-th state).  sub > 1 is asserted aligned: unaligned, a natural ego at
# heading 0 in a lane's centre sees the cars of its lane mirror-symmetrically, a cell's sub-rays
# j and sub - 1 - j return equal distances up to rounding and the model cannot tell which wins --
# 16 x 4 unaligned left 1.3 % (2 lanes) and 1.4 % (4 lanes) of the cells undecided, printed below
NATURAL = [(dict(cells=64), 1), (dict(cells=64, align=True), 1), (dict(cells=360, align=True), 2),
           (dict(cells=32, sub=4, align=True), 1), (dict(cells=24, sub=16, align=True), 1)]


@pytest.mark.parametrize("lanes", [2, 4])
def test_natural_states_leave_at_most_one_percent_undecided(lanes):
    cfg, states = natural_states(lanes)
    for kw, every in NATURAL + [(dict(cells=16, sub=4), 1)]:
        spec = LidarSpec(**kw)
        cells = undecided = returning = 0
        # the states alternate: as it is, moved; `every` keeps both kinds
        for st in states[0::2][::every] + states[1::2][::every]:
            m = lm.lidar_model(cfg, st, spec)
            cells, undecided = cells + m.cells, undecided + m.undecided
            returning += m.returning
        share = undecided / cells
        print(f"lanes {lanes} {kw}: {undecided} of {cells} cells undecided ({100 * share:.3f} %), "
              f"{returning} return ({100 * returning / cells:.1f} %)")
        if (kw, every) in NATURAL:
            assert returning >= 1000 and share <= 0.01, (kw, returning, share)
