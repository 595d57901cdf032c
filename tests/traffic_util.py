"""Inputs shared by the CPU and the GPU tests of hwy_traffic: the natural configurations, the
crafted states, and the deliberate mistakes the comparison has to notice."""

from __future__ import annotations

import numpy as np

from env_util import _clear, _put
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import make_cfg, policy_actions

STEPS = 32
ACTION_SEED = 11

# name -> make_cfg keywords.  Between them: E in {1, 5, 16}, lanes in {1, 4, 8, 64},
# vehicles_count in {0, 1, 50, 63}, dt 1/15 and 1/5.  64 lanes take neighbours_ordered's second
# branch (more than 62 lanes), 5 envs leave a block of four one-quarter full.
NATURAL = {
    "E16-default": dict(E=16),
    "E5-dt5": dict(E=5, simulation_frequency=5),
    "E1": dict(E=1),
    "E16-1lane": dict(E=16, lanes_count=1),
    "E5-8lanes-63cars": dict(E=5, lanes_count=8, vehicles_count=63),
    "E5-64lanes-63cars-dt5": dict(E=5, lanes_count=64, vehicles_count=63, simulation_frequency=5),
    "E16-64lanes": dict(E=16, lanes_count=64),
    "E5-no-traffic": dict(E=5, vehicles_count=0),
    "E16-1car": dict(E=16, vehicles_count=1),
    "E1-8lanes-1car-dt5": dict(E=1, lanes_count=8, vehicles_count=1, simulation_frequency=5),
}


def natural_cfg(name, **kw):
    return make_cfg(**dict(dict(max_episode_steps=12, vehicles_density=2), **NATURAL[name], **kw))


def actions(name):
    """the case's STEPS action arrays"""
    E = NATURAL[name]["E"]
    rng = np.random.default_rng(ACTION_SEED)
    return [policy_actions(rng, E, t) for t in range(STEPS)]


def oracle_states(name):
    """the reset state and the state after each of the STEPS steps, on the CPU oracle"""
    cfg = natural_cfg(name)
    ora = OracleEnv(cfg)
    ora.reset()
    out = [ora.state.copy()]
    for a in actions(name):
        ora.step(a)
        out.append(ora.state.copy())
    return cfg, out


# ------------------------------------------------------------------------------- crafted states
E_CRAFT = 12
PI = float(np.float32(np.pi))


def craft_cfg():
    return make_cfg(E=E_CRAFT, lanes_count=4, vehicles_count=12)


def craft(cfg):
    """[NFIELDS, 12, 64] uint32: the ego at (5000, 4) on lane 1, speed 20, with hand-placed cars.
      0  equal x on one lane: 3 and 7 both at 5030 ahead (front = 7, the last), 2 and 5 both at
         4970 behind (rear = 2, the first); for 3 the front is 7 and for 7 it is 3
      1  gap exactly 0 (front at x + 5) and a rear with gap exactly 0
      2  overlapping cars: front at x + 3 (gap -2), and one at the ego's own x on lane 2 (its
         front there, gap -5)
      3  closing exactly 0: a front with the ego's heading and speed words
      4  negative speed: the ego reverses (thw +inf), the front reverses faster (closing > 0)
      5  cars at |y - 4c| exactly 3 (on the lane) and nearer ones just past it (not), either side
      6  x just below -5 (no candidate) and at 10005 (no candidate), the ego near each end
      7  an absent slot between present ones (slots 1, 2, 4 absent; 3, 5 present)
      8  the leader of a lane: cars behind only
      9  the ego alone
     10  headings near +pi and -pi (vx = -speed cos: negative), a front likewise
     11  side lanes: a car alongside on lane 0 (front gap negative) and cars ahead / behind on 2"""
    assert cfg.num_envs == E_CRAFT and cfg.vehicles_count >= 12 and cfg.lanes_count == 4
    ora = OracleEnv(cfg)
    ora.reset()
    st = ora.state.copy()
    _clear(cfg, st)
    for e in range(E_CRAFT):
        _put(st, e, 0, 5000.0, 4.0)
    up = float(np.nextafter(np.float32(7.0), np.float32(8.0)))
    _put(st, 0, 3, 5030.0, 4.0), _put(st, 0, 7, 5030.0, 4.5, speed=15.0)
    _put(st, 0, 2, 4970.0, 4.0), _put(st, 0, 5, 4970.0, 3.5, speed=25.0)
    _put(st, 1, 1, 5005.0, 4.0, speed=10.0), _put(st, 1, 2, 4995.0, 4.0, speed=30.0)
    _put(st, 2, 1, 5003.0, 4.0, speed=10.0), _put(st, 2, 2, 5000.0, 8.0, speed=12.0)
    _put(st, 3, 4, 5040.0, 4.0, heading=0.0, speed=20.0)
    st[_abi.F_SPEED].view(np.float32)[4, 0] = -5.0
    _put(st, 4, 1, 5020.0, 4.0, speed=-12.0), _put(st, 4, 2, 4980.0, 4.0, speed=-1.0)
    _put(st, 5, 1, 5020.0, 7.0, lane=2), _put(st, 5, 2, 5010.0, up, lane=2)
    _put(st, 5, 3, 4990.0, 1.0, lane=0), _put(st, 5, 4, 4995.0, float(np.float32(1.0 - 2.0 ** -22)), lane=0)
    _put(st, 6, 0, 3.0, 4.0)
    _put(st, 6, 1, float(np.nextafter(np.float32(-5.0), np.float32(-6.0))), 4.0)
    _put(st, 6, 2, -5.0, 4.0, speed=5.0)
    _put(st, 6, 3, 10005.0, 4.0), _put(st, 6, 4, float(np.nextafter(np.float32(10005.0), np.float32(0.0))), 4.0)
    _put(st, 7, 3, 5050.0, 4.0, speed=18.0), _put(st, 7, 5, 5025.0, 4.0, speed=22.0)
    _put(st, 8, 1, 4950.0, 4.0), _put(st, 8, 2, 4900.0, 4.0, speed=30.0), _put(st, 8, 3, 5100.0, 12.0)
    near_pi = float(np.nextafter(np.float32(PI), np.float32(0.0)))
    st[_abi.F_HEADING].view(np.float32)[10, 0] = near_pi
    _put(st, 10, 1, 5030.0, 4.0, heading=-near_pi, speed=10.0)
    _put(st, 10, 2, 4960.0, 4.0, heading=3.0, speed=25.0)
    _put(st, 11, 1, 5002.0, 0.0), _put(st, 11, 2, 5040.0, 8.0, speed=12.0)
    _put(st, 11, 3, 4960.0, 8.0, speed=28.0), _put(st, 11, 4, 5070.0, 8.0)
    return st


def check_crafted(front, rear, gap, ego):
    """what the crafted states must give, stated by hand"""
    inf = np.inf
    f = lambda e: list(front[e, :8])
    r = lambda e: list(rear[e, :8])
    assert (front[0, 0], rear[0, 0], front[0, 3], front[0, 7]) == (7, 2, 7, 3)
    assert (rear[0, 3], rear[0, 7], front[0, 2], front[0, 5], rear[0, 2]) == (0, 0, 5, 2, -1)
    assert (gap[1, 0], ego[1, 2], ego[1, 3], ego[1, 4], ego[1, 6]) == (0.0, 0.0, 0.0, 0.0, 0.0)
    assert (front[2, 0], gap[2, 0], ego[2, 2], ego[2, 3], ego[2, 9]) == (1, -2.0, 0.0, 0.0, -5.0)
    assert (front[3, 0], gap[3, 0], ego[3, 1], ego[3, 2]) == (4, 35.0, 0.0, inf)
    assert ego[4, 3] == inf and ego[4, 1] > 0 and 0 < ego[4, 2] < inf and ego[4, 14] == -5.0
    # y = 7 and y = 1 are within the margin of lane 1 too; 7 + ulp and 1 - 4 ulp are not
    assert f(5)[:5] == [1, -1, 1, 4, -1] and r(5)[:5] == [3, 2, -1, -1, 3]
    assert (rear[6, 0], front[6, 0], rear[6, 2], front[6, 4]) == (2, 4, -1, -1)
    assert (front[6, 1], rear[6, 1], front[6, 3], rear[6, 3]) == (2, -1, -1, 4)
    assert f(7)[:6] == [5, -1, -1, -1, -1, 3] and r(7)[:6] == [-1, -1, -1, 5, -1, 0]
    assert (front[8, 0], gap[8, 0], ego[8, 2], rear[8, 0], rear[8, 1]) == (-1, inf, inf, 1, 2)
    assert (front[9, 0], rear[9, 0], ego[9, 11], ego[9, 12], ego[9, 15]) == (-1, -1, inf, 0.0, 0.0)
    assert all(ego[9, s] == inf for s in (0, 2, 4, 6, 7, 8, 9, 10))
    assert ego[10, 14] < -19.9 and ego[10, 3] == inf and ego[10, 1] < 0 and ego[10, 2] == inf
    assert (ego[11, 7], ego[11, 8], ego[11, 9], ego[11, 10]) == (-3.0, inf, 35.0, 35.0)
    assert ego[11, 11] == np.sqrt(np.float32(20.0)) and ego[11, 12] == 2.0 and ego[11, 13] == 0.0


# name -> the CONSTS override a correct comparison must refuse, and near_range as a threshold
MISTAKES = {
    "length 5 -> 5.05": dict(consts=dict(LENGTH=5.05)),
    "margin 1 -> 1.1": dict(consts=dict(MARGIN=1.1)),
    "front tie rule flipped": dict(consts=dict(FRONT_TIE_LAST=False)),
    "rear tie rule flipped": dict(consts=dict(REAR_TIE_FIRST=False)),
    "sign of closing": dict(consts=dict(CLOSING_SIGN=-1.0)),
    "vx without the cosine": dict(consts=dict(COSINE=False)),
    "rear taken as <=": dict(consts=dict(REAR_STRICT=False)),
    "near_range 50 -> 50.5": dict(near_range=50.5),
}
