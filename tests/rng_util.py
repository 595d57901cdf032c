"""The cases and drivers of the seed / reset / shuffle tests, shared by their CPU run on the
oracle (tests/test_rng_model.py) and their GPU run on the kernel (tests/test_rng_gpu.py).

A driver takes an env that has reset(seeds=None, mask=None) -> obs, step(actions) -> (obs, reward,
terminated, truncated, ...) and the packed state as `state` (OracleEnv: an array) or `state()`
(env_util.HipEnv), and compares it with tests/rng_model.py.  No torch, no libhwy.so here.
"""

from __future__ import annotations

import numpy as np

import env_model as em
import rng_model as rm
from env_util import Case, Checker
from hwy import _abi
from parity_util import make_cfg, policy_actions

E_RESET = 64

# name -> (make_cfg keywords, seed_base)
RESET_CASES = {
    "default": ({}, 42),
    "lanes-1": (dict(lanes_count=1), 42),
    "lanes-2": (dict(lanes_count=2), 42),
    "lanes-7": (dict(lanes_count=7), 42),
    "lanes-16": (dict(lanes_count=16), 42),
    "others-1": (dict(vehicles_count=1), 42),
    "others-10": (dict(vehicles_count=10), 42),
    "others-63": (dict(vehicles_count=63), 42),
    "ego-lane-drawn": (dict(initial_lane_id=-1), 42),
    "ego-lane-3": (dict(initial_lane_id=3), 42),
    "spacing-1-density-3-limit-20": (dict(ego_spacing=1, vehicles_density=3, speed_limit=20), 42),
    "seed_base-0": ({}, 0),
    "seed_base-crosses-2^32": ({}, 2 ** 32 - 2),
    "seed_base-2^33+5": ({}, 2 ** 33 + 5),
}


def reset_cfg(name, E=E_RESET, **more):
    kw, base = RESET_CASES[name]
    return make_cfg(E=E, seed_base=base, **dict(kw, **more))


def explicit_seeds(E=E_RESET):
    """E seeds with 0, 2^32 and 2^63 + 1 among them (the rest spread over 64 bits), and the mask
    that leaves every third env untouched"""
    s = [(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 64) for i in range(E)]
    s[1], s[2], s[4] = 0, 2 ** 32, 2 ** 63 + 1
    mask = (np.arange(E) % 3 != 0).astype(np.uint8)
    assert mask[[1, 2, 4]].all()
    return rm.seeds_u64(s), mask


def state_of(env):
    st = env.state
    return st() if callable(st) else st


def check_reset_obs(cfg, obs, state, envs, model=None):
    """the observation a reset wrote for `envs`, against env_model on the state (a shuffled one
    in rng_model's order)"""
    ck = Checker(Case("reset-obs", {}), cfg, None, rng=model)
    keep = np.zeros(cfg.num_envs, bool)
    keep[envs] = True
    ck._check_obs(obs, em.observe_model(cfg, state), keep & ~em.uncertain(cfg, state), state)


def run_reset_case(env, cfg, model=None, worst=None):
    """hwy_reset on the schedule (k = 0): every env's words against the model"""
    model = model or rm.RngModel()
    obs = env.reset()
    st = state_of(env)
    e = np.arange(cfg.num_envs)
    rm.check_fresh(cfg, st, e, seeds=model.schedule_seed(cfg, e, 0), model=model, episode=0,
                   worst=worst)
    check_reset_obs(cfg, obs, st, e, model)
    return obs, st


def run_explicit_reset(env, cfg, persistent_obs, model=None, worst=None):
    """reset(seeds, mask) after a schedule reset: the masked envs hold the explicit seeds'
    episodes (k = 0), the others every state word and obs row as before.  persistent_obs: the
    env writes into one obs buffer it keeps (HipEnv); else a zeroed one per call (OracleEnv)."""
    model = model or rm.RngModel()
    obs0 = env.reset().copy()
    st0 = state_of(env).copy()
    seeds, mask = explicit_seeds(cfg.num_envs)
    obs = env.reset(seeds=seeds, mask=mask)
    st = state_of(env)
    hit = mask != 0
    rm.check_fresh(cfg, st, hit, seeds=seeds[hit], model=model, episode=0, worst=worst)
    check_reset_obs(cfg, obs, st, np.nonzero(hit)[0], model)
    np.testing.assert_array_equal(st[:, ~hit], st0[:, ~hit], err_msg="state of an unmasked env")
    want = obs0[~hit] if persistent_obs else np.zeros_like(obs0[~hit])
    np.testing.assert_array_equal(obs[~hit].view(np.uint32), want.view(np.uint32),
                                  err_msg="obs rows of an unmasked env")
    return obs, st


# ------------------------------------------------------------------------------- the schedule
def schedule_cfg(E=4, **more):
    """4 envs of 3-step episodes with autoreset, env_offset 5, seed_stride 7"""
    cfg = make_cfg(E=E, seed_base=2 ** 32 - 20, max_episode_steps=3, autoreset=True, **more)
    cfg.env_offset, cfg.seed_stride = 5, 7
    return cfg


class ScheduleTracker:
    """The model's side of a run: per env the episode counter k and the seed the schedule gives
    it.  seed_fn(e, k) -> uint64 [len e] is model.schedule_seed with the handle's settings."""

    def __init__(self, cfg, seed_fn, model=None):
        self.cfg, self.seed_fn, self.model = cfg, seed_fn, model or rm.RngModel()
        self.k = np.zeros(cfg.num_envs, np.int64)
        self.seeds = seed_fn(np.arange(cfg.num_envs), self.k)
        self.fresh_seen = 0

    def after_reset(self, state, seeds=None, mask=None):
        """a reset starts the masked envs at k = 0 with the explicit seed (or the schedule's)"""
        e = np.arange(self.cfg.num_envs)
        hit = np.ones(len(e), bool) if mask is None else np.asarray(mask) != 0
        self.k[hit] = 0
        new = self.seed_fn(e, self.k) if seeds is None else rm.seeds_u64(seeds)
        self.seeds[hit] = new[hit]
        self._check(state, hit)

    def after_step(self, state, done):
        """an autoreset (or a cut) moves a finished env to k + 1 and the schedule's seed of it"""
        done = np.asarray(done).astype(bool)
        self.k[done] += 1
        self.seeds[done] = self.seed_fn(np.arange(self.cfg.num_envs), self.k)[done]
        self._check(state, done)

    def _check(self, state, fresh):
        ew = state[_abi.F_ENV]
        np.testing.assert_array_equal(ew[:, _abi.E_EPISODE], self.k, err_msg="E_EPISODE")
        np.testing.assert_array_equal(rm.state_seeds(state), self.seeds, err_msg="E_SEED words")
        rm.check_fresh(self.cfg, state, fresh, seeds=self.seeds[fresh], model=self.model)
        self.fresh_seen += int(np.sum(fresh))


def run_schedule(env, cfg, seed_fn, model=None, steps=10, step_fn=None, seed=0):
    """reset, `steps` steps of autoreset episodes, then reset(seeds, mask) of all but env 1 and 4
    more steps: after every call the episode and seed words and every fresh env's state are the
    model's.  The explicit reset starts the masked envs' counters at 0 again, so the next
    autoreset takes them to the schedule's k = 1 (not to explicit seed + stride)."""
    tr = ScheduleTracker(cfg, seed_fn, model)
    step_fn = step_fn or (lambda a: env.step(a))
    E = cfg.num_envs
    env.reset()
    tr.after_reset(state_of(env))
    rng = np.random.default_rng(seed)
    for t in range(steps):
        out = step_fn(policy_actions(rng, E, t))
        tr.after_step(state_of(env), np.asarray(out[2]).astype(bool) | np.asarray(out[3]).astype(bool))
    assert (tr.k >= steps // cfg.max_steps).all(), tr.k
    seeds = rm.seeds_u64([2 ** 40 + 3 * e for e in range(E)])
    mask = (np.arange(E) != 1).astype(np.uint8)
    env.reset(seeds=seeds, mask=mask)
    k1 = tr.k[1]
    tr.after_reset(state_of(env), seeds, mask)
    assert tr.k[1] == k1 and (tr.k[mask != 0] == 0).all()
    for t in range(4):
        out = step_fn(policy_actions(rng, E, steps + t))
        tr.after_step(state_of(env), np.asarray(out[2]).astype(bool) | np.asarray(out[3]).astype(bool))
    assert (tr.k[mask != 0] >= 1).all(), tr.k   # autoreset again: on the schedule from k = 1
    np.testing.assert_array_equal(tr.seeds, seed_fn(np.arange(E), tr.k))
    return tr


# ------------------------------------------------------------------------------- the shuffle
TIE_SEED, TIE_STEP, TIE_SLOTS = 27637, 1, (3, 14)   # equal keys at N = 64 (found by search)


def tie_cfg(E=16):
    """N = 64 shuffled with all 63 others admitted; env 0 is reset with TIE_SEED, whose slots 3
    and 14 draw the same key at step 1"""
    return make_cfg(E=E, N=64, order="shuffled", vehicles_count=63, lanes_count=16,
                    observation=dict(see_behind=True), autoreset=False)


def run_tie_case(env, cfg, model=None):
    """one step from a reset with TIE_SEED in env 0: the ordered comparison at the step where two
    keys are equal"""
    model = model or rm.RngModel()
    E = cfg.num_envs
    seeds = rm.seeds_u64([TIE_SEED + 1000 * e for e in range(E)])
    env.reset(seeds=seeds)
    ck = Checker(Case("tie", {}), cfg, None, rng=model)
    out = env.step(np.zeros((E, 2), np.float32))
    st = state_of(env)
    assert st[_abi.F_ENV][0, _abi.E_STEP] == TIE_STEP and rm.state_seeds(st)[0] == TIE_SEED
    assert (em.observed_vehicles(cfg, st)[0] >= 0).all(), "a tied slot holds no vehicle"
    ck.check(out, st)
    return out, st


def shuffled_reset_is_the_sorted_twins_rows_moved(make_env, N, model=None, E=E_RESET):
    """The shuffled reset observation is exactly the sorted twin's rows (a fresh road is in index
    order and the ego is its first car, so both orders list the same vehicles) at the rows the
    model's shuffle_dest names: equal bit for bit."""
    model = model or rm.RngModel()
    kw = dict(E=E, N=N, vehicles_count=max(N - 1, 5), lanes_count=16, observation=dict(see_behind=True))
    cs, cu = make_cfg(order="sorted", **kw), make_cfg(order="shuffled", **kw)
    es, eu = make_env(cs), make_env(cu)
    try:
        obs_s, obs_u = es.reset().copy(), eu.reset().copy()
        st = state_of(eu)
        dest = model.shuffle_dest(N, rm.state_seeds(st), st[_abi.F_ENV][:, _abi.E_STEP])
        want = obs_s.copy()
        want[np.arange(E)[:, None], dest] = obs_s[:, 1:]
        np.testing.assert_array_equal(obs_u.view(np.uint32), want.view(np.uint32))
        assert (dest != 1 + np.arange(N - 1)).any()
    finally:
        for x in (es, eu):
            if hasattr(x, "close"):
                x.close()
