"""The env's dynamics, one simulation frame at a time, against tests/dyn_model.py.

The oracle alone, on the CPU: the kernel equals it bit for bit (tests/test_env_dyn_gpu.py runs
the same cases on the GPU and compares the kernel with the model directly).  With
sim_freq == policy_freq a step is one frame, and every frame's after-state is compared with the
model of that frame's own before-state, so the chaotic trajectory never enters the comparison.

Each case also proves its own conditions: the branches it is about occur, and `uncertain` leaves
out at most 5 % of its (env, frame) pairs.  test_model_constant_is_exercised shows that the
inputs reach every constant of DESIGN.md §4's table: with the constant 1 % off in the model the
comparison fails.
"""

import numpy as np
import pytest

import dyn_model as dm
import env_model as em
from env_util import DYN_CASES, _clear, _put, run_dyn_case_on_oracle
from hwy import _abi
from parity_util import make_cfg

_BY_NAME = {c.name: c for c in DYN_CASES}


@pytest.mark.parametrize("case", DYN_CASES, ids=[c.name for c in DYN_CASES])
def test_oracle_frames_match_the_model(case):
    run_dyn_case_on_oracle(case).finish()


# constant -> the cases tried, the likeliest first
_WHERE = {
    "A_MAX": ("dyn-crafted-pairs",), "B": ("dyn-default",), "D0": ("dyn-crafted-pairs",),
    "T": ("dyn-crafted-pairs",), "ACC_CLIP": ("dyn-crafted-pairs",),
    "GAIN": ("dyn-crafted-pairs",), "BRAKE": ("dyn-crafted-pairs",), "DELAY": ("dyn-default",),
    "MARGIN": ("dyn-default", "dyn-lanes-8", "dyn-density-3"),
    "K_LAT": ("dyn-crafted-singles",), "K_HEADING": ("dyn-crafted-singles",),
    "STEER_MAX": ("dyn-crafted-singles",), "HALF_L": ("dyn-crafted-singles",),
    "SPEED_CLIP": ("dyn-crafted-singles",), "LENGTH": ("dyn-crafted-pairs",),
    "WIDTH": ("dyn-crafted-pairs", "dyn-default"), "DIAGONAL": ("dyn-crafted-pairs",),
    "EGO_ACC": ("dyn-crafted-singles",), "EGO_STEER": ("dyn-crafted-singles",),
}


def test_every_constant_has_a_case():
    assert set(_WHERE) == set(dm.CONSTS)


@pytest.mark.parametrize("name", sorted(dm.CONSTS))
def test_model_constant_is_exercised(name):
    """One of the constant's cases refuses the model with the constant 1 % larger: the inputs
    tell the constant from its neighbour."""
    for case_name in _WHERE[name]:
        try:
            run_dyn_case_on_oracle(_BY_NAME[case_name], {name: dm.CONSTS[name] * 1.01})
        except AssertionError:
            return
    pytest.fail(f"no case of {_WHERE[name]} tells {name} from 1.01 * {name}")


def test_case_table_stays_small():
    """natural runs are 16 envs for 96 one-frame steps, crafted ones at most 8 envs and 4"""
    assert len(_BY_NAME) == len(DYN_CASES)
    for c in DYN_CASES:
        cfg = c.make()
        assert cfg.sim_freq == cfg.policy_freq and not cfg.autoreset, c.name
        assert (c.E, c.steps) == (16, 96) if c.craft is None else (c.E <= 8 and c.steps <= 4), c.name


# ---------------------------------------------------------------- the model's own known answers
def _one(cfg, put):
    """a packed state of one env: every slot absent, then put(st)"""
    st = np.zeros((_abi.NFIELDS, 1, 64), np.uint32)
    _clear(cfg, st)
    put(st)
    return st


def test_model_free_road_and_follower_by_hand():
    """IDM by hand at dt = 1 / 15: a free road at v = v0 holds its speed; at v0 = 30 the speed
    gains 3 (1 - (20 / 30)^4) / 15; a follower 40 m behind an equal car (d* = 40) loses 3 / 15"""
    cfg = make_cfg(E=1, vehicles_count=3, policy_frequency=15, autoreset=False)

    def put(st):
        _put(st, 0, 1, 100.0, 0.0)
        _put(st, 0, 2, 500.0, 4.0, tspeed=30.0)
        _put(st, 0, 3, 60.0, 0.0)

    out, unc = dm.frame_model(cfg, _one(cfg, put), np.zeros((1, 2), np.float32))
    assert not unc[0]
    np.testing.assert_allclose(out["speed"].v[0, 1:], [20.0, 20.0 + 3 * (1 - (2 / 3) ** 4) / 15,
                                                       20.0 - 3.0 / 15], rtol=1e-12)
    np.testing.assert_allclose(out["x"].v[0, 1:], [100 + 20 / 15, 500 + 20 / 15, 60 + 20 / 15], rtol=1e-12)
    assert out["timer"].v[0, 1] == pytest.approx(1 / 15) and out["timer"].v[0, 0] == 0.0
    assert (out["flags"][0] == _abi.FLAG_PRESENT).all()
    assert out["lane"][0].tolist() == [3, 0, 1, 0]


def test_model_neighbour_ties_and_margin_by_hand():
    """front: the last in list order among the nearest ahead (equal s included); rear: the first
    among the nearest behind; a car 3 m off the lane's centre is on it, one at 3.01 m is not"""
    x = np.array([[100.0, 120.0, 120.0, 100.0, 80.0, 80.0]])
    y = np.array([[0.0, 0.0, 3.0, 3.01, -1.0, 0.5]])
    lat = np.abs(y[:, :, None] - 4.0 * np.arange(2))
    front, rear = dm.neighbours(x, lat <= 3.0)
    assert front[0, 0, 0] == 2 and rear[0, 0, 0] == 4     # vehicle 3 (3.01 m) is not on lane 0
    assert front[0, 4, 0] == 5 and front[0, 5, 0] == 4    # equal s: each is the other's front
    assert front[0, 2, 0] == 1 and rear[0, 1, 0] == 0
    # lane 1 (y = 4): 2 and 3 are on it; 3 is level with 0 (s_0 <= s_3), so it is 0's front
    assert front[0, 0, 1] == 3 and rear[0, 1, 1] == 3 and front[0, 3, 1] == 2


def test_model_collision_by_hand():
    """two parallel cars at rest 4 m apart overlap by 1 m along x and by 2 m across: both crashed,
    and the pending impact pushes each 0.5 m apart along x; 5.2 m apart nothing happens; a car
    at 30 m/s 6.9 m behind one at rest ends the step 4.9 m behind it: it overlaps"""
    cfg = make_cfg(E=3, vehicles_count=2, policy_frequency=15, autoreset=False)
    st = np.zeros((_abi.NFIELDS, 3, 64), np.uint32)
    _clear(cfg, st)
    wreck = _abi.FLAG_PRESENT | _abi.FLAG_CRASHED   # crashed cars take acc = -v and no steering
    for e, (gap, va) in enumerate(((4.0, 0.0), (5.2, 0.0), (6.9, 30.0))):
        _put(st, e, 1, 100.0, 0.0, speed=va, flags=wreck)
        _put(st, e, 2, 100.0 + gap, 0.0, speed=0.0, flags=wreck)
    out, unc = dm.frame_model(cfg, st, np.zeros((3, 2), np.float32))
    assert not unc.any()
    hit = wreck | _abi.FLAG_IMPACT
    assert out["flags"][:, 1:].tolist() == [[hit, hit], [wreck, wreck], [hit, hit]]
    np.testing.assert_allclose(out["impact_x"].v[0, 1:], [-0.5, 0.5], atol=1e-12)
    np.testing.assert_allclose(out["impact_y"].v[0, 1:], [0.0, 0.0], atol=1e-12)
    np.testing.assert_allclose(out["x"].v[2, 1:], [102.0, 106.9], rtol=1e-7)   # 106.9 as float32
    np.testing.assert_allclose(out["speed"].v[2, 1], 28.0, rtol=1e-12)


def test_q_new_operations_bound_a_float32_evaluation():
    """sqrt, asin, atan, tan, pow and the saturating clip on random float32 inputs: a float32
    evaluation by numpy stays within TOL_FACTOR times the bound, and a saturated clip is exact"""
    rng = np.random.default_rng(0)
    a = rng.uniform(0.01, 30.0, 4000).astype(np.float32)
    b = rng.uniform(0.01, 30.0, 4000).astype(np.float32)
    s = em.Q(a.astype(np.float64)) / em.Q(b.astype(np.float64))    # carries one rounding
    s32 = a / b
    for q, got in ((s.sqrt(), np.sqrt(s32)), (s.atan(), np.arctan(s32)),
                   (s.clip(0, 1).asin(), np.arcsin(np.minimum(s32, np.float32(1)))),
                   (s.clip(0, 1.2).tan(), np.tan(np.minimum(s32, np.float32(1.2)))),
                   (s.pow(4.25), np.power(s32, np.float32(4.25)))):
        err = np.abs(got.astype(np.float64) - q.v)
        assert (err <= em.TOL_FACTOR * q.e).all(), float((err / q.e).max())
    c = s.clip_sat(0.0, 1.0)
    assert (c.e[s.v > 1.001] == 0).all() and (c.e[s.v < 0.999] > 0).all()
    assert (em.Q(3.0, 0.1).minimum(em.Q(3.05, 0.2)).e == 0.2)
