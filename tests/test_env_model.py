"""The CPU oracle against tests/env_model.py (a float64 numpy restatement that shares no code
with hwy_math.h or hwy_oracle.c) over the config-space case table of tests/env_util.py.

The kernel is bit-equal to the oracle (tests/test_env_config_gpu.py runs the same cases), so a
misreading the two share shows here first, without a GPU.  Each case also proves its own
conditions on the CPU: the branch it is about really occurs ("must occur"), and `uncertain`
leaves out at most 5 % of its (env, step) pairs.
"""

import numpy as np
import pytest

import env_model as em
from env_util import CASES, Checker, run_case_on_oracle
from hwy import _abi
from parity_util import make_cfg


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_oracle_matches_the_model(case):
    run_case_on_oracle(case).finish()


_SWITCHED = [c for c in CASES if c.ignore]


@pytest.mark.parametrize("case", _SWITCHED, ids=[c.name for c in _SWITCHED])
def test_case_would_catch_a_step_that_dropped_its_switch(case):
    """The case's run tells its switch from the value a step would fall back to if its copy of
    the config lost the field: the oracle's outputs under the case's config are refused by the
    checker reading the config without the switch."""
    cfg, table = case.make()
    from oracle.oracle import OracleEnv

    ora = OracleEnv(cfg, table)
    ora.reset()
    ck = Checker(case, case.dropped_cfg(), table)
    rng = np.random.default_rng(case.seed)
    with pytest.raises(AssertionError):
        for t in range(case.steps):
            out = ora.step(case.actions(rng, cfg.num_envs, t))
            ck.check(out, ora.state)


def test_case_table_stays_small():
    """every case is a few seconds at most on the GPU: 16 to 24 envs, 12 to 20 steps"""
    names = {c.name for c in CASES}
    assert len(names) == len(CASES)
    for c in CASES:
        assert 16 <= c.E <= 24 and 12 <= c.steps <= 20, c.name


# ---------------------------------------------------------------- the model's own known answers
def _state(cfg, xs, ys, speeds=None, headings=None, lanes=None):
    """a packed state of one env holding the given vehicles (index 0 is the ego)"""
    st = np.zeros((_abi.NFIELDS, 1, 64), np.uint32)
    n = len(xs)
    st[_abi.F_X].view(np.float32)[0, :n] = xs
    st[_abi.F_Y].view(np.float32)[0, :n] = ys
    st[_abi.F_SPEED].view(np.float32)[0, :n] = speeds if speeds is not None else 20.0
    st[_abi.F_HEADING].view(np.float32)[0, :n] = headings if headings is not None else 0.0
    st[_abi.F_LANE][0, :n] = lanes if lanes is not None else np.round(np.asarray(ys) / 4).astype(np.uint32)
    st[_abi.F_FLAGS][0, :n] = _abi.FLAG_PRESENT
    return st


def test_model_admission_and_order_by_hand():
    # ego at 300; others at dx = +20, -5, -15, +199.9 (3 m aside: beyond 200 m), +8, -8
    xs = [300.0, 320.0, 295.0, 285.0, 499.9, 308.0, 292.0]
    ys = [0.0, 4.0, 0.0, 4.0, 3.0, 8.0, 4.0]
    cfg = make_cfg(E=1, N=6, vehicles_count=6)
    rows = em.observed_vehicles(cfg, _state(cfg, xs, ys))
    # -15 is behind the -10 m line, 499.9 is 199.92 m away (inside); |dx| 8 ties: index order
    assert rows.tolist() == [[2, 5, 6, 1, 4]]
    cfg = make_cfg(E=1, N=6, vehicles_count=6, observation=dict(see_behind=True))
    assert em.observed_vehicles(cfg, _state(cfg, xs, ys)).tolist() == [[2, 5, 6, 3, 1]]
    cfg = make_cfg(E=1, N=4, vehicles_count=6, order="shuffled")
    assert em.observed_vehicles(cfg, _state(cfg, xs, ys)).tolist() == [[1, 2, 4]]
    ys[4] = 12.0  # sqrt(199.9^2 + 12^2) = 200.26: out
    cfg = make_cfg(E=1, N=8, vehicles_count=6)
    assert em.observed_vehicles(cfg, _state(cfg, xs, ys)).tolist() == [[2, 5, 6, 1, -1, -1, -1]]


def test_model_observation_and_reward_by_hand():
    xs, ys = [300.0, 320.0], [4.0, 8.0]
    cfg = make_cfg(E=1, N=3, vehicles_count=1)
    st = _state(cfg, xs, ys, speeds=[25.0, 20.0])
    obs = em.observe_model(cfg, st)
    want = [[1.0, 0.04, 25 / 30, 0.0], [0.2, 0.04, -5 / 30, 0.0], [0.0] * 4]  # ego x clipped
    np.testing.assert_allclose(obs.v[0], want, atol=1e-12)
    assert (obs.e[0, 2] == 0).all() and obs.e[0, 0, 0] > 0
    cfg = make_cfg(E=1, N=3, vehicles_count=1, observation=dict(absolute=True, normalize=False))
    np.testing.assert_array_equal(em.observe_model(cfg, st).v[0],
                                  [[300.0, 4.0, 25.0, 0.0], [320.0, 8.0, 20.0, 0.0], [0.0] * 4])
    # reward: lane 1 of 4, 25 m/s -> 0.1/3 + 0.4 * 0.5, mapped from [-1, 0.5] to [0, 1]
    cfg = make_cfg(E=1, vehicles_count=1)
    terms, rew, term = em.reward_model(cfg, st)
    np.testing.assert_allclose(terms.v[0], [0.0, 1 / 3, 0.5, 1.0], atol=1e-7)
    np.testing.assert_allclose(rew.v[0], (0.1 / 3 + 0.2 + 1.0) / 1.5, atol=1e-7)
    assert not term[0]
    st[_abi.F_Y].view(np.float32)[0, 0] = 6.5  # 2.5 m off lane 1's centre: off the road
    cfg = make_cfg(E=1, vehicles_count=1, offroad_terminal=True)
    terms, rew, term = em.reward_model(cfg, st)
    assert terms.v[0, 3] == 0.0 and rew.v[0] == 0.0 and term[0]
    assert not em.uncertain(cfg, st)[0]
    st[_abi.F_Y].view(np.float32)[0, 0] = 6.0005
    assert em.uncertain(cfg, st)[0]


def test_model_wrappers_by_hand():
    cfg = make_cfg(E=1, N=3, pe=_abi.PE_DIST, d=2)
    obs = em.Q(np.array([[[0.3, 0.4, 0.0, 0.0], [0.0, 0.0, 0.5, 0.5], [0.0] * 4]]))
    out = em.wrap_model(cfg, obs, [1.0])
    ang = 2 * np.pi * np.array([0.0, 0.5, 0.5]) / 100.0
    np.testing.assert_allclose(out.v[0, :, 4], np.sin(ang), atol=1e-15)
    np.testing.assert_allclose(out.v[0, :, 5], np.cos(ang), atol=1e-15)
    cfg = make_cfg(E=1, N=3, pe=_abi.PE_ROPE, d=2, ego_idx=1)
    out = em.wrap_model(cfg, obs, [1.0])
    th = 2 * np.pi * 0.5 / 100.0  # row 0 is 0.5 from row 1
    np.testing.assert_allclose(out.v[0, 0, :2], [0.3 * np.cos(th) - 0.4 * np.sin(th),
                                                 0.3 * np.sin(th) + 0.4 * np.cos(th)], atol=1e-15)
    np.testing.assert_array_equal(out.v[0, :, 2:], obs.v[0, :, 2:])


def test_checker_rejects_a_wrong_observation():
    """the comparison has teeth: a relative row made absolute, one value off by 1e-5, and two
    shuffled rows merged into one are each refused"""
    case = next(c for c in CASES if c.name == "absolute-shuffled")
    cfg, table = case.make()
    from oracle.oracle import OracleEnv

    ora = OracleEnv(cfg, table)
    ora.reset()
    out = ora.step(np.zeros((cfg.num_envs, 2), np.float32))
    Checker(case, cfg, table).check(out, ora.state)
    for spoil in ("value", "merge"):
        obs = out[0].copy()
        if spoil == "value":
            obs[3, 5, 1] += 1e-5
        else:
            obs[3, 5] = obs[3, 6]
        with pytest.raises(AssertionError):
            Checker(case, cfg, table).check((obs,) + tuple(out[1:]), ora.state)
    rew = out[1].copy()
    rew[2] += 1e-5
    with pytest.raises(AssertionError):
        Checker(case, cfg, table).check((out[0], rew) + tuple(out[2:]), ora.state)
