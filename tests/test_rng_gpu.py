"""Seeds, reset draws and the shuffle order of the kernels against tests/rng_model.py, and
against the CPU oracle bit for bit: the cases of tests/test_rng_model.py through hwy_reset (with
and without seeds and a mask), the autoreset inside hwy_step, hwy_step_with_info and
hwy_step_with_final, one hwy_step_group launch over three handles of unlike N with seed groups,
hwy_cut_episodes, and the Python env classes.

The comparison with the model is direct (it does not pass through the oracle); 64 envs and 14
steps at the most.
"""

import ctypes

import numpy as np
import pytest

import rng_model as rm
import rng_util as ru
from env_util import Case, Checker, HipEnv
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import diff_state, make_cfg, policy_actions

pytestmark = pytest.mark.gpu

M = rm.RngModel()
STEP_NAMES = ("obs", "reward", "terminated", "truncated", "ep_return", "ep_length")


class OracleParts:
    """The oracle's side of a handle: one OracleEnv, or with seed groups one per group (a group
    is the solo handle of its envs with seed_base = seed_bases[g], include/hwy.h)."""

    def __init__(self, cfg, bases=None, per=None):
        if bases is None:
            self.parts, self.per = [OracleEnv(cfg)], cfg.num_envs
        else:
            self.per, self.parts = per, []
            for b in bases:
                c = type(cfg).from_buffer_copy(cfg)
                c.num_envs, c.seed_base = per, int(b)
                self.parts.append(OracleEnv(c))

    def _split(self, x):
        return [None if x is None else np.asarray(x)[g * self.per:(g + 1) * self.per]
                for g in range(len(self.parts))]

    def reset(self, seeds=None, mask=None):
        return np.concatenate([p.reset(seeds=s, mask=m) for p, s, m in
                               zip(self.parts, self._split(seeds), self._split(mask))])

    def step(self, a):
        outs = [p.step(x) for p, x in zip(self.parts, self._split(a))]
        return tuple(np.concatenate(x) for x in zip(*outs))

    @property
    def state(self):
        return np.concatenate([p.state for p in self.parts], axis=1)

    def set_state(self, st):
        for g, p in enumerate(self.parts):
            p.state[...] = st[:, g * self.per:(g + 1) * self.per]


class Both:
    """A HipEnv and the oracle in lockstep: every call compares the two bit for bit (state words
    and outputs) and hands out the kernel's side, which the drivers compare with the model."""

    def __init__(self, cfg, bases=None, per=None, step="step"):
        self.cfg, self.hip, self.ora = cfg, HipEnv(cfg), OracleParts(cfg, bases, per)
        if bases is not None:
            self.hip.set_seed_groups(bases, per)
        self.V, self.how = cfg.vehicles_count + 1, step
        self.twin = None
        if step == "step_final":   # an autoreset-off oracle that steps from the same state
            tc = type(cfg).from_buffer_copy(cfg)
            tc.autoreset = 0
            self.twin = OracleEnv(tc)
            self.twin_ck = Checker(Case("final_obs", {}), tc, None)
            self.finals = 0

    def _same(self, what):
        st = self.hip.state()
        d = diff_state(st, self.ora.state, self.V)
        assert d is None, f"{what}: {d}"
        return st

    def state(self):
        return self.hip.state()

    def reset(self, seeds=None, mask=None):
        written = np.ones(self.cfg.num_envs, bool) if mask is None else np.asarray(mask) != 0
        oh, oo = self.hip.reset(seeds=seeds, mask=mask), self.ora.reset(seeds=seeds, mask=mask)
        np.testing.assert_array_equal(oh[written], oo[written], err_msg="reset obs")
        self._same("reset")
        return oh

    def step(self, a):
        if self.twin is not None:
            self.twin.state[...] = self.ora.state
        ro = self.ora.step(a)
        out = getattr(self.hip, self.how)(a)
        rh = out if self.how == "step" else tuple(out[k] for k in HipEnv.STEP_KEYS)
        self._same(self.how)
        for name, h, o in zip(STEP_NAMES, rh, ro):
            np.testing.assert_array_equal(np.asarray(h).astype(o.dtype), o, err_msg=f"{self.how}: {name}")
        if self.twin is not None:
            # final_obs is what the autoreset-off twin observes: the finished episode's vehicles
            # in the order of ITS seed and step count, which the twin's state still holds
            tw = self.twin.step(a)
            done = ro[2] | ro[3]
            np.testing.assert_array_equal(out["final_obs"][done], tw[0][done], err_msg="final_obs")
            self.twin_ck.check(tw, self.twin.state)
            self.finals += int(done.sum())
        return rh

    def close(self):
        self.hip.close()


# ------------------------------------------------------------------------------- hwy_reset
@pytest.mark.parametrize("name", list(ru.RESET_CASES))
def test_reset_state_kernel_equals_model_and_oracle(name):
    cfg = ru.reset_cfg(name)
    env, w = Both(cfg), {}
    try:
        ru.run_reset_case(env, cfg, worst=w)
        print(name, {k: f"{e:.3g} / {b:.3g}" for k, (e, b) in w.items() if b > 0})
    finally:
        env.close()


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_explicit_seeds_with_a_mask(order):
    cfg = make_cfg(E=ru.E_RESET, order=order, initial_lane_id=-1)
    env = Both(cfg)
    try:
        ru.run_explicit_reset(env, cfg, persistent_obs=True)
    finally:
        env.close()


@pytest.mark.parametrize("N", [3, 15, 64])
def test_shuffled_reset_observation_is_the_sorted_twins_rows_moved(N):
    ru.shuffled_reset_is_the_sorted_twins_rows_moved(HipEnv, N)


def test_equal_keys_go_to_the_lower_slot():
    cfg = ru.tie_cfg()
    env = Both(cfg)
    try:
        ru.run_tie_case(env, cfg)
    finally:
        env.close()


# ------------------------------------------------------------------------------- autoreset
@pytest.mark.parametrize("how", ["step", "step_info", "step_final"])
def test_schedule_through_autoreset_and_explicit_reset(how):
    cfg = ru.schedule_cfg(order="shuffled")
    env = Both(cfg, step=how)
    try:
        tr = ru.run_schedule(env, cfg, lambda e, k: M.schedule_seed(cfg, e, k))
        assert tr.fresh_seen >= 4 * (1 + 3 + 1)
        if how == "step_final":
            assert env.finals >= 12
    finally:
        env.close()


def test_schedule_of_seed_groups_through_autoreset():
    bases, per = [2 ** 32 - 3, 900], 2
    cfg = ru.schedule_cfg(E=4)
    env = Both(cfg, bases, per)
    try:
        ru.run_schedule(env, cfg, lambda e, k: M.schedule_seed(cfg, e, k, group_bases=bases,
                                                               group_envs=per))
    finally:
        env.close()


# ------------------------------------------------------------------------------- grouped launch
def test_grouped_step_of_unlike_N_with_seed_groups():
    """Three handles (N = 3 with two seed groups, N = 15 with three, N = 64 with all 63 admitted
    on a schedule with env_offset and stride) in ONE hwy_step_group launch per step: every
    handle's episode and seed words, each fresh env's state and every shuffled observation in
    order against the model, and against the oracle bit for bit."""
    import torch

    from hwy.native import HwyStepGroupPlan, HwyStepIO, check, lib, ptr

    kw = dict(order="shuffled", max_episode_steps=3, autoreset=True)
    specs = [(make_cfg(E=4, N=3, seed_base=1, **kw), [2 ** 32 - 3, 900], 2),
             (make_cfg(E=6, N=15, seed_base=2, **kw), [5, 2 ** 33, -4], 2),
             (make_cfg(E=4, N=64, seed_base=2 ** 32 - 6, vehicles_count=63, lanes_count=16,
                       observation=dict(see_behind=True), **kw), None, None)]
    specs[2][0].env_offset, specs[2][0].seed_stride = 5, 7
    envs = [Both(cfg, b, per) for cfg, b, per in specs]
    n = len(envs)
    try:
        trs, cks = [], []
        for env, (cfg, b, per) in zip(envs, specs):
            env.reset()
            tr = ru.ScheduleTracker(cfg, lambda e, k, cfg=cfg, b=b, per=per: M.schedule_seed(
                cfg, e, k, group_bases=b, group_envs=per))
            tr.after_reset(env.state())
            trs.append(tr)
            cks.append(Checker(Case(f"grouped-N{cfg.obs_vehicles}", {}), cfg, None))
        hips = [e.hip for e in envs]
        dev = hips[0].dev
        acts = [torch.zeros(h.E, 2, device=dev) for h in hips]
        io = (HwyStepIO * n)(*[HwyStepIO(ptr(a), ptr(h.obs), ptr(h.rew), ptr(h.term), ptr(h.trunc),
                                         ptr(h.er), ptr(h.el)) for a, h in zip(acts, hips)])
        hs = (ctypes.c_void_p * n)(*[h.h.value for h in hips])
        table = torch.empty(int(lib().hwy_step_group_table_bytes(n)), dtype=torch.uint8, device=dev)
        plan = HwyStepGroupPlan()
        check(lib().hwy_step_group_prepare(hs, io, n, table.data_ptr(), ctypes.byref(plan), None),
              "hwy_step_group_prepare")
        rng = np.random.default_rng(0)
        for t in range(10):
            a_np = [policy_actions(rng, h.E, t) for h in hips]
            for a, x in zip(acts, a_np):
                a.copy_(torch.as_tensor(x))
            check(lib().hwy_step_group(ctypes.byref(plan), table.data_ptr(), None), "hwy_step_group")
            torch.cuda.synchronize()
            for i, (env, x) in enumerate(zip(envs, a_np)):
                got, want = env.hip._out(), env.ora.step(x)
                st = env._same(f"handle {i} step {t}")
                for name, h, o in zip(STEP_NAMES, got, want):
                    np.testing.assert_array_equal(np.asarray(h).astype(o.dtype), o,
                                                  err_msg=f"handle {i} step {t}: {name}")
                trs[i].after_step(st, want[2] | want[3])
                cks[i].check(got, st)
        assert all((tr.k >= 3).all() for tr in trs)
    finally:
        for e in envs:
            e.close()


# ------------------------------------------------------------------------------- the cut
def test_cut_starts_the_schedules_next_episode():
    """hwy_cut_episodes on a handle with seed groups, two steps into 3-step episodes: every env
    moves to k + 1 and the seed the model's schedule gives it; the oracle reset with the model's
    seeds holds the same words."""
    bases, per = [2 ** 32 - 3, 900, 17], 2
    cfg = ru.schedule_cfg(E=6, order="shuffled")
    env = Both(cfg, bases, per)
    try:
        tr = ru.ScheduleTracker(cfg, lambda e, k: M.schedule_seed(cfg, e, k, group_bases=bases,
                                                                  group_envs=per))
        env.reset()
        tr.after_reset(env.state())
        rng = np.random.default_rng(3)
        for t in range(5):   # through one autoreset, then two steps into the next episode
            out = env.step(policy_actions(rng, 6, t))
            tr.after_step(env.state(), out[2] | out[3])
        steps = env.state()[_abi.F_ENV][:, _abi.E_STEP]
        obs, er, el, cut = env.hip.cut_episodes()
        np.testing.assert_array_equal(cut, (steps >= 1).astype(np.uint8))
        assert cut.sum() >= 4
        st = env.hip.state()
        tr.after_step(st, cut)
        ru.check_reset_obs(cfg, obs, st, np.nonzero(cut)[0])
        ost = env.ora.state.copy()
        for g, p in enumerate(env.ora.parts):   # the oracle's side: reset with the model's seeds
            sl = slice(g * per, (g + 1) * per)
            want = p.reset(seeds=tr.seeds[sl], mask=cut[sl])
            p.state[_abi.F_ENV][:, _abi.E_EPISODE] = tr.k[sl].astype(np.uint32)
            np.testing.assert_array_equal(obs[sl][cut[sl] != 0], want[cut[sl] != 0])
        env._same("after the cut")
        assert not np.array_equal(ost, env.ora.state)
        for t in range(4):   # and the schedule goes on
            out = env.step(policy_actions(rng, 6, 5 + t))
            tr.after_step(env.state(), out[2] | out[3])
    finally:
        env.close()


# ------------------------------------------------------------------------------- Python surface
def test_python_envs_reset_to_the_models_state_of_the_seed():
    """HighwayEnv.reset(seed=s), HighwayVecEnv.reset(seeds=[s]) and a one-env HighwayVecEnv after
    set_seed_schedule(s - 1) export the same state, the model's reset_state(s)."""
    import copy

    import torch

    from config.base_config import HIGHWAY_CONFIG
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv

    s = 2 ** 32 + 12345
    conf = copy.deepcopy(HIGHWAY_CONFIG)
    conf["observation"]["order"] = "shuffled"
    dev = torch.device("cuda", 0)
    one = HighwayEnv(conf, device=dev)
    vec = HighwayVecEnv(conf, num_envs=1, device=dev)
    sched = HighwayVecEnv(conf, num_envs=1, device=dev)
    try:
        o1, _ = one.reset(seed=s)
        o2, _ = vec.reset(seeds=torch.tensor([s]))
        sched.set_seed_schedule(s - 1)
        o3, _ = sched.reset()
        torch.cuda.synchronize()
        states = [e.export_state().cpu().numpy().view(np.uint32)
                  for e in (one.vec_env, vec, sched)]
        for st in states[1:]:
            assert diff_state(st, states[0], 51) is None
        np.testing.assert_array_equal(o2[0].cpu().numpy(), o1)
        np.testing.assert_array_equal(o3[0].cpu().numpy(), o1)
        cfg = vec.hwy_config
        rm.check_fresh(cfg, states[0], [0], seeds=[s], episode=0)
        ru.check_reset_obs(cfg, o1[None], states[0], [0])
    finally:
        one.close()
        vec.close()
        sched.close()
