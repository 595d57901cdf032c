"""The env parity driver shared by the GPU parity tests, the config-space case table with its
checker against tests/env_model.py, and the dynamics case table with its checker against
tests/dyn_model.py (each shared by the CPU and the GPU run of the cases).

torch and libhwy.so are imported only when a HipEnv is built, so the CPU tests can import the
case table and the checker without a GPU.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

import env_model as em
import rng_model as rm
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import diff_state, make_cfg, pe_table_for, policy_actions


class HipEnv:
    """Direct C-ABI driver (no Python env layer) so the test exercises exactly libhwy.so."""

    STEP_KEYS = ("obs", "rew", "term", "trunc", "er", "el")
    INFO_KEYS = ("speed", "crashed", "lane", "rewards", "acc", "ep_stats")

    def __init__(self, cfg, table=None):
        import torch

        from hwy.native import check, lib

        self.torch, self.dev = torch, torch.device("cuda", 0)
        DEV = self.dev
        self.cfg = cfg
        self.E, self.N, self.Fo = cfg.num_envs, cfg.obs_vehicles, cfg.obs_features()
        self.h = ctypes.c_void_p()
        check(lib().hwy_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "hwy_create")
        if table is not None:
            t = np.ascontiguousarray(table, np.float32)
            check(lib().hwy_set_pe_table(self.h, t.ctypes.data_as(ctypes.c_void_p), t.size),
                  "hwy_set_pe_table")
        self.obs = torch.zeros(self.E, self.N, self.Fo, device=DEV)
        self.rew = torch.zeros(self.E, device=DEV)
        self.term = torch.zeros(self.E, dtype=torch.uint8, device=DEV)
        self.trunc = torch.zeros(self.E, dtype=torch.uint8, device=DEV)
        self.er = torch.zeros(self.E, device=DEV)
        self.el = torch.zeros(self.E, dtype=torch.int32, device=DEV)
        self._info = None

    def reset(self, seeds=None, mask=None):
        """hwy_reset: seeds [E] (any integer dtype, taken as 64-bit words) or None for the
        schedule; mask [E] (nonzero = reset) or None for every env"""
        from hwy.native import check, lib, ptr

        torch = self.torch
        s = None if seeds is None else torch.as_tensor(
            np.ascontiguousarray(seeds).astype(np.uint64).view(np.int64), device=self.dev)
        m = None if mask is None else torch.as_tensor(np.asarray(mask).astype(np.uint8), device=self.dev)
        check(lib().hwy_reset(self.h, ptr(s), ptr(m), ptr(self.obs), None), "hwy_reset")
        torch.cuda.synchronize()
        return self.obs.cpu().numpy()

    def _actions(self, a):
        return self.torch.as_tensor(a, device=self.dev).contiguous()

    def _out(self):
        self.torch.cuda.synchronize()
        return tuple(getattr(self, k).cpu().numpy() for k in self.STEP_KEYS)

    def step(self, a):
        from hwy.native import check, lib, ptr

        at = self._actions(a)
        check(lib().hwy_step(self.h, ptr(at), ptr(self.obs), ptr(self.rew), ptr(self.term),
                             ptr(self.trunc), ptr(self.er), ptr(self.el), None), "hwy_step")
        return self._out()

    def _info_struct(self):
        from hwy.native import ptr

        torch, n, DEV = self.torch, self.E, self.dev
        if self._info is None:
            self.speed = torch.zeros(n, device=DEV)
            self.crashed = torch.zeros(n, dtype=torch.uint8, device=DEV)
            self.lane = torch.zeros(n, dtype=torch.int32, device=DEV)
            self.rewards = torch.zeros(n, 4, device=DEV)
            self.acc = torch.full((n, _abi.HWY_INFO_NACC), float("nan"), device=DEV)
            self.ep_stats = torch.full((n, _abi.HWY_INFO_NACC), float("nan"), device=DEV)
            self.final_obs = torch.full((n, self.N, self.Fo), float("nan"), device=DEV)
            self._info = _abi.HwyStepInfo(*[ptr(getattr(self, k)) for k in self.INFO_KEYS])
        return self._info

    def _info_out(self, extra=()):
        out = dict(zip(self.STEP_KEYS, self._out()))
        out.update({k: getattr(self, k).cpu().numpy() for k in self.INFO_KEYS + tuple(extra)})
        return out

    def step_info(self, a):
        """hwy_step_with_info: a dict of the step outputs and the info outputs."""
        from hwy.native import check, lib, ptr

        at, info = self._actions(a), self._info_struct()
        check(lib().hwy_step_with_info(self.h, ptr(at), ptr(self.obs), ptr(self.rew),
                                       ptr(self.term), ptr(self.trunc), ptr(self.er),
                                       ptr(self.el), ctypes.byref(info), None),
              "hwy_step_with_info")
        return self._info_out()

    def step_final(self, a, info=True):
        """hwy_step_with_final (with the info outputs unless info=False): the same dict plus
        "final_obs", whose rows are written only for the envs that finished."""
        from hwy.native import check, lib, ptr

        at, st = self._actions(a), self._info_struct()
        check(lib().hwy_step_with_final(self.h, ptr(at), ptr(self.obs), ptr(self.rew),
                                        ptr(self.term), ptr(self.trunc), ptr(self.er),
                                        ptr(self.el), ctypes.byref(st) if info else None,
                                        ptr(self.final_obs), None), "hwy_step_with_final")
        return self._info_out(("final_obs",))

    def set_seed_groups(self, seed_bases, envs_per_group):
        from hwy.native import check, lib

        b = np.ascontiguousarray(seed_bases, np.int64)
        check(lib().hwy_set_seed_groups(self.h, b.ctypes.data_as(ctypes.c_void_p), len(b),
                                        int(envs_per_group)), "hwy_set_seed_groups")

    def cut_episodes(self):
        """hwy_cut_episodes: (obs, ep_return, ep_length, cut)"""
        from hwy.native import check, lib, ptr

        if not hasattr(self, "cut"):
            self.cut = self.torch.zeros(self.E, dtype=self.torch.uint8, device=self.dev)
        check(lib().hwy_cut_episodes(self.h, ptr(self.obs), ptr(self.er), ptr(self.el),
                                     ptr(self.cut), None), "hwy_cut_episodes")
        self.torch.cuda.synchronize()
        return tuple(x.cpu().numpy() for x in (self.obs, self.er, self.el, self.cut))

    def state(self):
        from hwy.native import check, lib, ptr

        torch = self.torch
        out = torch.zeros(_abi.NFIELDS, self.E, 64, dtype=torch.int32, device=self.dev)
        check(lib().hwy_export_state(self.h, ptr(out), None), "export")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def set_state(self, st):
        from hwy.native import check, lib, ptr

        torch = self.torch
        t = torch.as_tensor(np.ascontiguousarray(st).view(np.int32), device=self.dev)
        check(lib().hwy_import_state(self.h, ptr(t), None), "import")
        torch.cuda.synchronize()

    def close(self):
        from hwy.native import lib

        lib().hwy_destroy(self.h)


def run_parity(cfg, steps, table=None, seed=0, action_fn=policy_actions, hook=None,
               init_state=None, start_hook=None):
    """hook (optional): called after every step's comparisons with
    (cfg, hip outputs, hip state, oracle outputs).  init_state (optional): a packed state both
    sides import after the reset; start_hook (optional): called with the kernel's state before
    the first step."""
    hip = HipEnv(cfg, table)
    ora = OracleEnv(cfg, table)
    V = cfg.vehicles_count + 1
    try:
        o_h = hip.reset()
        o_o = ora.reset()
        d = diff_state(hip.state(), ora.state, V)
        assert d is None, f"reset state: {d}"
        np.testing.assert_array_equal(o_h, o_o, err_msg="reset obs")
        if init_state is not None:
            hip.set_state(init_state)
            ora.state[...] = init_state
            d = diff_state(hip.state(), ora.state, V)
            assert d is None, f"imported state: {d}"
        if start_hook is not None:
            start_hook(hip.state())
        rng = np.random.default_rng(seed)
        stats = dict(crashes=0, dones=0, lane_changes=0)
        for t in range(steps):
            a = action_fn(rng, cfg.num_envs, t)
            rh = hip.step(a)
            ro = ora.step(a)
            hip_state = hip.state()
            d = diff_state(hip_state, ora.state, V)
            assert d is None, f"step {t}: {d}"
            np.testing.assert_array_equal(rh[0], ro[0], err_msg=f"obs at step {t}")
            np.testing.assert_array_equal(rh[1], ro[1], err_msg=f"reward at step {t}")
            np.testing.assert_array_equal(rh[2].astype(bool), ro[2], err_msg=f"terminated at step {t}")
            np.testing.assert_array_equal(rh[3].astype(bool), ro[3], err_msg=f"truncated at step {t}")
            np.testing.assert_array_equal(rh[4], ro[4], err_msg=f"episode return at step {t}")
            np.testing.assert_array_equal(rh[5], ro[5], err_msg=f"episode length at step {t}")
            stats["dones"] += int((ro[2] | ro[3]).sum())
            stats["crashes"] += int(ro[2].sum())
            st = ora.state
            stats["lane_changes"] += int((st[_abi.F_LANE, :, 1:V] != st[_abi.F_TLANE, :, 1:V]).sum())
            if hook is not None:
                hook(cfg, rh, hip_state, ro)
        return stats
    finally:
        hip.close()


# ------------------------------------------------------------------------------- actions
def wild(rng, E, t):
    """hard random steering: crashes, non-zero headings, cars leaving the road"""
    return np.tanh(rng.normal(size=(E, 2)) * 2.0).astype(np.float32)


def fast(rng, E, t):
    """throttle and a nearly straight wheel: the ego overtakes the traffic it starts behind"""
    return np.stack([rng.uniform(0.3, 1.0, E), np.tanh(rng.normal(size=E) * 0.05)],
                    axis=1).astype(np.float32)


def swerve(rng, E, t):
    """a hard turn to one side per env (alternating): off the road within a few steps"""
    side = np.where(np.arange(E) % 2 == 0, 1.0, -1.0)
    return np.stack([rng.uniform(-0.2, 0.2, E), side * rng.uniform(0.5, 1.0, E)],
                    axis=1).astype(np.float32)


# ------------------------------------------------------------------------------- the cases
ALL8 = ["presence", "x", "y", "vx", "vy", "cos_h", "sin_h", "heading"]
BASE_RANGES = {"x": [-100, 100], "y": [-100, 100], "vx": [-30, 30], "vy": [-30, 30]}


@dataclass
class Case:
    name: str
    cfg: dict                      # make_cfg keywords
    need: dict = field(default_factory=dict)   # coverage counter -> the least count
    cover: tuple = ()              # names of Checker.cov_* methods
    steps: int = 12
    actions: object = policy_actions
    seed: int = 0
    E: int = 16
    autoreset: bool = False        # off: the post-step state is the one the reward is of
    ignore: dict = field(default_factory=dict)  # hwy_config field -> the value a build that
    #                                dropped the case's switch would compute with (dropped_cfg)

    def make(self):
        kw = dict(self.cfg)
        cfg = make_cfg(E=self.E, autoreset=self.autoreset, **kw)
        kind = kw.get("pe", _abi.PE_NONE)
        table = None
        if kind != _abi.PE_NONE and kw.get("d", 0) > 0:
            table = pe_table_for(_abi.PE_DIST if kind == _abi.PE_DIST1 else kind, kw["d"],
                                 cfg.obs_vehicles, seed=3)
        return cfg, table

    def dropped_cfg(self):
        """the case's config as a step that ignored its switch would read it"""
        cfg, _ = self.make()
        for k, v in self.ignore.items():
            if k == "has_range":  # every feature mapped over the shipped config's ranges
                for f, (lo, hi) in enumerate(v):
                    cfg.has_range[f] = 1
                    cfg.features_range[f][0], cfg.features_range[f][1] = lo, hi
            elif k == "reward_speed_range":
                cfg.reward_speed_range[0], cfg.reward_speed_range[1] = v
            else:
                setattr(cfg, k, v)
        return cfg


def _cases():
    c = []

    def add(name, cfg, **kw):
        c.append(Case(name, cfg, **kw))

    for order in ("sorted", "shuffled"):
        add(f"absolute-{order}", dict(order=order, observation=dict(absolute=True)),
            cover=("absolute",), need=dict(x_absolute=1, y_absolute=1), ignore=dict(absolute=0))
        add(f"see_behind-{order}", dict(order=order, observation=dict(see_behind=True)),
            cover=("behind",), actions=fast, steps=20, E=24, seed=3, ignore=dict(see_behind=0),
            need=dict(behind=1, **({"behind_before_ahead": 1} if order == "sorted" else {})))
    add("raw", dict(observation=dict(normalize=False)), cover=("beyond_one",), need=dict(beyond_one=1),
        ignore=dict(normalize=1))
    add("unclipped", dict(observation=dict(clip=False, features_range=dict(BASE_RANGES, x=[-20, 20]))),
        cover=("beyond_one",), need=dict(beyond_one=1), ignore=dict(clip=1))
    add("partial-range", dict(observation=dict(features_range={"x": [-100, 100]})),
        cover=("partial",), need=dict(unmapped=1),
        ignore=dict(has_range=[(-100, 100), (-100, 100), (-30, 30), (-30, 30)]))
    add("all-8-features", dict(observation=dict(features=ALL8)), actions=wild, cover=("heading",),
        need=dict(heading=1))
    add("odd-feature-list", dict(observation=dict(features=["vx", "heading", "presence"])),
        actions=wild)
    add("N1", dict(N=1))
    add("N2-shuffled", dict(N=2, order="shuffled"))
    add("N3-shuffled", dict(N=3, order="shuffled"))
    add("N64-V11", dict(N=64, vehicles_count=10), cover=("zero_rows",), need=dict(zero_rows=1))
    # 16 lanes: Vehicle.create_random's spacing shrinks with e^(-5/40 lanes), so the 63 others
    # start within 200 m of the ego
    add("N64-V64", dict(N=64, vehicles_count=63, lanes_count=16, observation=dict(see_behind=True)),
        cover=("all_admitted",), need=dict(all_admitted=1))
    add("N64-V64-shuffled", dict(N=64, order="shuffled", vehicles_count=63, lanes_count=16,
                                 observation=dict(see_behind=True)),
        cover=("all_admitted",), need=dict(all_admitted=1))
    for name, kw in (("policy_frequency-5", dict(policy_frequency=5)),
                     ("policy_frequency-15", dict(policy_frequency=15)),
                     ("frames-10-over-3", dict(simulation_frequency=10, policy_frequency=3))):
        add(name, kw, steps=20, cover=("frames",), need=dict(speed_steps=100),
            ignore=dict(policy_freq=1))
    for name, kw, ig in (
            ("lanes1-start0", dict(lanes_count=1, initial_lane_id=0), dict(ego_spacing=1.0)),
            ("lanes2-start1", dict(lanes_count=2, initial_lane_id=1), dict(initial_lane_id=-1)),
            ("lanes8-start0-limit20", dict(lanes_count=8, initial_lane_id=0, speed_limit=20),
             dict(speed_limit=30.0)),
            ("lanes8-start7-spacing1", dict(lanes_count=8, initial_lane_id=7, ego_spacing=1),
             dict(ego_spacing=2.0))):
        add(name, dict(kw, max_episode_steps=4), autoreset=True, cover=("start",),
            need=dict(starts=16), ignore=ig)
    for name, kw, ig in (
            ("reward-unnormalised", dict(normalize_reward=False), dict(normalize_reward=1)),
            ("reward-on_road", dict(on_road_reward=0.3), dict(on_road_reward=0.0)),
            ("reward-weights", dict(collision_reward=-2, right_lane_reward=0.3, high_speed_reward=0.7),
             dict(right_lane_reward=0.1)),
            ("reward-speed-range", dict(reward_speed_range=[10, 20]),
             dict(reward_speed_range=(20.0, 30.0)))):
        add(name, dict(kw, vehicles_density=3), actions=wild, steps=16, E=24, cover=("crash",),
            need=dict(crash_steps=1, other_steps=1), ignore=ig)
    add("off-road", dict(offroad_terminal=True, lanes_count=2), actions=swerve, steps=12, E=24,
        cover=("offroad",), need=dict(offroad_terminations=3), ignore=dict(offroad_terminal=0))
    for kind, nm in ((_abi.PE_DIST, "dist"), (_abi.PE_ROPE, "rope")):
        add(f"fused-{nm}-ego_idx2", dict(order="shuffled", pe=kind, d=4, ego_idx=2),
            cover=("row2",), need=dict(row2_vehicle=1), ignore=dict(ego_idx=0))
    add("fused-dist1", dict(pe=_abi.PE_DIST1, d=4), ignore=dict(pe_kind=_abi.PE_DIST))
    add("fused-rope-8-of-8", dict(pe=_abi.PE_ROPE, d=8, observation=dict(features=ALL8)),
        actions=wild)
    add("fused-rope-identity", dict(pe=_abi.PE_ROPE, d=0))
    add("fused-rank-widest", dict(pe=_abi.PE_RANK, d=56, N=64, observation=dict(features=ALL8)))
    return c


CASES = _cases()


# ------------------------------------------------------------------------------- the checker
class Checker:
    """One case's outputs (the kernel's or the oracle's) against the float64 model, step by
    step; collects the coverage counts, the share of (env, step) pairs `uncertain` leaves out
    and the worst error against the derived bound.

    `shuffled` observations are compared in order, row by row: the model's unshuffled rows are
    moved to the rows tests/rng_model.py's `shuffle_dest` names for the seed and step in the
    state's words, then wrapped, so the fused wrapper reads the row that really stands at
    `ego_idx`.  That states the ordered comparison for `ego_idx >= 1` too; no case is compared
    as a set any more.  `rng` (optional) is the RngModel to take the permutation from."""

    def __init__(self, case, cfg, table, rng=None):
        self.case, self.cfg, self.table = case, cfg, table
        self.rng = rng or rm.RngModel()
        self.count = {k: 0 for k in case.need}
        self.pairs = self.left_out = 0
        self.worst = dict(obs=(0.0, 0.0), reward=(0.0, 0.0), terms=(0.0, 0.0))  # (error, bound)
        self.terminated_seen = set()
        self.t = 0

    # ---- comparison
    def _within(self, what, got, q):
        err = np.abs(np.asarray(got, np.float64) - q.v)
        tol = em.TOL_FACTOR * q.e
        if not err.size:
            return
        k = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        assert err[k] <= tol[k], (f"{self.case.name} step {self.t} {what} at {k}: got "
                                  f"{np.asarray(got)[k]!r}, model {q.v[k]!r}, error "
                                  f"{err[k]:.3g} > bound {tol[k]:.3g}")
        # the worst error seen, as a share of its bound (a zero bound means equal, asserted above)
        ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
        k = np.unravel_index(int(np.argmax(ratio)), err.shape)
        w = self.worst[what]
        if w[1] == 0.0 or ratio[k] > w[0] / w[1]:
            self.worst[what] = (float(err[k]), float(tol[k]))

    def _check_obs(self, obs, m, keep, state):
        cfg, table = self.cfg, self.table
        N, F = cfg.obs_vehicles, cfg.n_features
        rank = cfg.pe_kind == _abi.PE_RANK
        if rank:  # the appended columns are the table's row for the position, exactly
            t = np.asarray(table, np.float32).reshape(N, cfg.d_embed)
            np.testing.assert_array_equal(obs[:, :, F:], np.broadcast_to(t, obs[:, :, F:].shape))
        if cfg.order == _abi.ORDER_SHUFFLED and N > 2:
            m = self._shuffled(m, state)
        w = em.wrap_model(cfg, m, table)
        self._within("obs", obs[keep], w[keep])

    def _shuffled(self, m, state):
        """the model's rows in the kernel's order: slot q (row 1 + q) moved to the row
        rng_model's shuffle_dest gives for the seed and the step count in the state's words"""
        E, N = m.v.shape[:2]
        dest = self.rng.shuffle_dest(N, rm.state_seeds(state), state[_abi.F_ENV][:, _abi.E_STEP])
        ar = np.arange(E)[:, None]
        v, e = m.v.copy(), m.e.copy()
        v[ar, dest], e[ar, dest] = m.v[:, 1:], m.e[:, 1:]
        return em.Q(v, e)

    def check(self, out, state):
        """out: (obs, reward, terminated, truncated, ...) of one step; state: the packed state
        after it."""
        cfg = self.cfg
        obs, rew, term, trunc = (np.asarray(x) for x in out[:4])
        unc = em.uncertain(cfg, state)
        self.pairs += unc.size
        self.left_out += int(unc.sum())
        m = em.observe_model(cfg, state)
        self._check_obs(obs, m, ~unc, state)
        # the reward is of the state before an autoreset, which a reset env no longer holds
        done = term.astype(bool) | trunc.astype(bool)
        keep = ~unc & ~(done & bool(cfg.autoreset))
        terms, r, terminated = em.reward_model(cfg, state)
        self._within("reward", rew[keep], r[keep])
        np.testing.assert_array_equal(term.astype(bool)[keep], terminated[keep],
                                      err_msg=f"{self.case.name} step {self.t}: terminated")
        for name in self.case.cover:
            getattr(self, "cov_" + name)(out, state, m)
        self.t += 1

    def check_terms(self, rewards, state, keep=None):
        """the four terms hwy_step_with_info reports against reward_model's"""
        terms, _, _ = em.reward_model(self.cfg, state)
        keep = ~em.uncertain(self.cfg, state) if keep is None else keep
        self._within("terms", rewards[keep], terms[keep])

    def report(self):
        share = self.left_out / max(self.pairs, 1)
        w = self.worst
        return (f"{self.case.name}: worst obs error {w['obs'][0]:.3g} (bound {w['obs'][1]:.3g}), "
                f"reward {w['reward'][0]:.3g} (bound {w['reward'][1]:.3g}); uncertain "
                f"{self.left_out}/{self.pairs} = {100 * share:.2f} %; coverage {self.count}")

    def finish(self):
        print(self.report())
        for k, least in self.case.need.items():
            assert self.count[k] >= least, f"{self.case.name}: {k} occurred {self.count[k]} times, need {least}"
        # a cap, not a target: a case over it gets another seed or other actions
        assert self.left_out <= 0.05 * self.pairs, self.report()

    # ---- coverage ("must occur")
    def _col(self, name):
        ids = [int(self.cfg.feature_ids[f]) for f in range(self.cfg.n_features)]
        return ids.index(_abi.FEATURES[name])

    def cov_absolute(self, out, state, m):
        rel_cfg = type(self.cfg).from_buffer_copy(self.cfg)
        rel_cfg.absolute = 0
        rel = em.observe_model(rel_cfg, state)
        seen = np.concatenate([np.zeros((m.v.shape[0], 1), bool),
                               em.observed_vehicles(self.cfg, state) >= 0], 1)
        for name in ("x", "y"):
            f = self._col(name)
            differs = seen & (np.abs(m.v[:, :, f] - rel.v[:, :, f]) > 1e-3)
            if self.cfg.order == _abi.ORDER_SORTED:  # the kernel's value is the absolute one
                differs &= np.abs(out[0][:, :, f] - m.v[:, :, f]) < 1e-5
            self.count[name + "_absolute"] += int(differs.sum())

    def cov_beyond_one(self, out, state, m):
        self.count["beyond_one"] += int((np.abs(out[0]) > 1.0).sum())

    def cov_partial(self, out, state, m):
        assert [int(self.cfg.has_range[f]) for f in range(4)] == [1, 0, 0, 0]
        self.count["unmapped"] += int((np.abs(out[0][:, :, 1:]) > 1.0).any(-1).sum())

    def cov_behind(self, out, state, m):
        rows = em.observed_vehicles(self.cfg, state)
        x = state[_abi.F_X].view(np.float32).astype(np.float64)
        dx = np.take_along_axis(x, np.maximum(rows, 0), 1) - x[:, :1]
        behind = (rows >= 0) & (dx < -10.0)
        self.count["behind"] += int(behind.sum())
        if "behind_before_ahead" in self.count:  # sorted: a row behind before a farther row ahead
            ahead = (rows >= 0) & (dx > 0)
            later_ahead = np.cumsum(ahead[:, ::-1], 1)[:, ::-1] - ahead
            self.count["behind_before_ahead"] += int((behind & (later_ahead > 0)).sum())

    def cov_heading(self, out, state, m):
        self.count["heading"] += int((np.abs(out[0][:, :, self._col("heading")]) > 0.1).sum())

    def cov_zero_rows(self, out, state, m):
        missing = em.observed_vehicles(self.cfg, state) < 0
        assert not out[0][:, 1:][missing].any(), "a missing row is not all zero"
        self.count["zero_rows"] += int(missing.sum())

    def cov_all_admitted(self, out, state, m):
        n = (em.observed_vehicles(self.cfg, state) >= 0).sum(1)
        self.count["all_admitted"] += int((n == self.cfg.vehicles_count).sum())

    def cov_start(self, out, state, m):
        """the envs the step has just autoreset, against Vehicle.create_random's numbers (DESIGN
        §4's table): the ego in initial_lane_id at 25 m/s and 3 + U(0.9, 1.1) offsets down the
        road, offset = ego_spacing * (12 + 25) * e^(-5/40 lanes); the others at U(0.7, 0.8) of the
        speed limit"""
        cfg = self.cfg
        fresh = state[_abi.F_ENV][:, _abi.E_STEP] == 0
        V = cfg.vehicles_count + 1
        lane = state[_abi.F_LANE][fresh, 0].astype(np.int32)
        x, y, spd = (state[k].view(np.float32)[fresh].astype(np.float64)
                     for k in (_abi.F_X, _abi.F_Y, _abi.F_SPEED))
        assert (lane == cfg.initial_lane_id).all(), lane
        assert (y[:, 0] == 4.0 * cfg.initial_lane_id).all(), y[:, 0]
        assert (spd[:, 0] == 25.0).all()
        offset = cfg.ego_spacing * 37.0 * np.exp(-5.0 / 40.0 * cfg.lanes_count)
        j = x[:, 0] / offset - 3.0   # float32: a handful of roundings at <= 4 offsets
        assert (j >= 0.9 - 1e-5).all() and (j <= 1.1 + 1e-5).all(), (j.min(), j.max())
        lim = float(cfg.speed_limit)
        others = spd[:, 1:V]
        assert (others >= 0.7 * lim - 1e-5).all() and (others <= 0.8 * lim + 1e-5).all(), \
            (others.min(), others.max())
        self.count["starts"] += int(fresh.sum())

    def cov_frames(self, out, state, m):
        """the ego is a plain Vehicle: each frame adds acceleration * dt to its speed (SURVEY §8
        a1.5), so over one policy step an uncrashed ego gains acc * frames / simulation_frequency
        with frames = simulation_frequency // policy_frequency.  acc is the state's ego action
        word.  Bound: `frames` float32 additions at |v| <= 40 and as many products, doubled."""
        cfg = self.cfg
        frames = cfg.sim_freq // cfg.policy_freq
        dt = 1.0 / cfg.sim_freq
        spd = state[_abi.F_SPEED].view(np.float32)[:, 0].astype(np.float64)
        if getattr(self, "prev_speed", None) is not None:
            acc = state[_abi.F_ENV].view(np.float32)[:, _abi.E_EGO_ACC].astype(np.float64)
            flags = state[_abi.F_FLAGS][:, 0]
            clean = ((flags | self.prev_flags) & (_abi.FLAG_CRASHED | _abi.FLAG_IMPACT)) == 0
            clean &= (np.abs(spd) < 39.9) & (np.abs(acc) > 0.5)
            want = self.prev_speed + acc * frames * dt
            bound = 2.0 * frames * em.U * (40.0 + 2.0 * np.abs(acc) * dt)
            err = np.abs(spd - want)
            assert (err[clean] <= bound[clean]).all(), (self.t, err[clean].max(), bound[clean].min())
            self.count["speed_steps"] += int(clean.sum())
        self.prev_speed, self.prev_flags = spd, state[_abi.F_FLAGS][:, 0].copy()

    def cov_crash(self, out, state, m):
        crashed = (state[_abi.F_FLAGS][:, 0] & _abi.FLAG_CRASHED) != 0
        self.count["crash_steps"] += int(crashed.sum())
        self.count["other_steps"] += int((~crashed).sum())

    def cov_offroad(self, out, state, m):
        crashed = (state[_abi.F_FLAGS][:, 0] & _abi.FLAG_CRASHED) != 0
        for e in np.nonzero(np.asarray(out[2]).astype(bool))[0]:
            if e not in self.terminated_seen:  # autoreset is off: an env's first termination
                self.terminated_seen.add(e)
                self.count["offroad_terminations"] += int(not crashed[e])

    def cov_row2(self, out, state, m):
        F = self.cfg.n_features
        seen = np.sort(em.observed_vehicles(self.cfg, state) >= 0, 1)[:, ::-1]
        # with the ego at row 0 and >= 2 vehicles seen, shuffling puts a vehicle or a zero row at
        # row 2; count the envs where it is a vehicle (its unwrapped columns are not all zero)
        row2 = np.abs(out[0][:, 2, :F]).sum(-1) > 0 if self.cfg.pe_kind != _abi.PE_ROPE else \
            np.abs(out[0][:, 2]).sum(-1) > 0
        self.count["row2_vehicle"] += int((row2 & seen[:, 0]).sum())


def run_case_on_oracle(case):
    """The case on the CPU oracle alone, checked against the model: the Checker, finished."""
    cfg, table = case.make()
    ora = OracleEnv(cfg, table)
    ora.reset()
    ck = Checker(case, cfg, table)
    rng = np.random.default_rng(case.seed)
    for t in range(case.steps):
        out = ora.step(case.actions(rng, cfg.num_envs, t))
        ck.check(out, ora.state)
    return ck


# ------------------------------------------------------------------- the dynamics, frame by frame
# The cases of tests/dyn_model.py: sim_freq == policy_freq, so a step is one simulation frame,
# and autoreset off, so crashed vehicles keep being stepped.  Natural runs are 16 envs for 96
# frames; a crafted case imports hand-built states (<= 8 envs, 4 frames) for what traffic does
# not reach on its own.
def beyond_one(rng, E, t):
    """actions three times the usual ones: about a third of the components beyond +-1"""
    return (3.0 * policy_actions(rng, E, t)).astype(np.float32)


@dataclass
class DynCase:
    name: str
    cfg: dict
    need: dict                     # DynChecker counter -> the least count
    never: tuple = ()              # counters that must stay 0
    steps: int = 96
    E: int = 16
    actions: object = policy_actions
    seed: int = 0                  # of the actions and, through seed_base, of the traffic
    craft: object = None           # craft(cfg, reset state) -> (state, fixed actions [E, 2])

    def make(self):
        kw = dict(policy_frequency=15, seed_base=42 + 1000 * self.seed)   # the traffic's seeds
        kw.update(self.cfg)
        return make_cfg(E=self.E, autoreset=False, **kw)

    def start(self, cfg):
        """(the state to import after the reset or None, the action function)"""
        if self.craft is None:
            return None, self.actions
        ora = OracleEnv(cfg)
        ora.reset()
        st, a = self.craft(cfg, ora.state.copy())
        return st, (lambda rng, E, t: a)


_P = _abi.FLAG_PRESENT


def _clear(cfg, st):
    """every vehicle slot absent and zero; the ego far down the road on the last lane"""
    V = cfg.vehicles_count + 1
    st[:_abi.F_ENV, :, :V] = 0
    for e in range(st.shape[1]):
        _put(st, e, 0, 5000.0, 4.0 * (cfg.lanes_count - 1))


def _put(st, e, i, x, y, heading=0.0, speed=20.0, lane=None, tlane=None, tspeed=None, delta=4.0,
         timer=0.0, flags=_P):
    lane = int(round(y / 4.0)) if lane is None else lane
    for f, val in ((_abi.F_X, x), (_abi.F_Y, y), (_abi.F_HEADING, heading), (_abi.F_SPEED, speed),
                   (_abi.F_TSPEED, speed if tspeed is None else tspeed),
                   (_abi.F_DELTA, 0.0 if i == 0 else delta), (_abi.F_TIMER, timer)):
        st[f].view(np.float32)[e, i] = val
    st[_abi.F_LANE][e, i] = lane
    st[_abi.F_TLANE][e, i] = lane if tlane is None else tlane
    st[_abi.F_FLAGS][e, i] = flags


def craft_singles(cfg, st):
    """one vehicle's edges: the +-40 m/s clip, |v| < 1 at a fired timer, a saturated slip,
    headings next to +-pi, the road's two ends"""
    _clear(cfg, st)
    a = np.zeros((cfg.num_envs, 2), np.float32)
    for e, (spd, thr) in enumerate(((39.9, 1.0), (40.5, 1.0), (-40.5, -1.0), (40.5, -1.0))):
        _put(st, e, 0, 5000.0, 12.0, speed=spd)
        a[e] = (thr, 0.1)
    # 4: |v| < 1 behind a blocker at a fired timer stays; at 1.5 m/s it goes
    _put(st, 4, 1, 300.0, 4.0, speed=0.5, timer=1.2)
    _put(st, 4, 2, 308.0, 4.0, speed=0.5)
    _put(st, 4, 3, 400.0, 8.0, speed=1.5, timer=1.2)
    _put(st, 4, 4, 409.0, 8.0, speed=1.5)
    # 5: two lanes from the target at 2 m/s, from either side: slip and steering saturate
    _put(st, 5, 1, 300.0, 0.0, speed=2.0, tlane=2)
    _put(st, 5, 2, 400.0, 12.0, speed=2.0, tlane=1)
    _put(st, 5, 3, 500.0, 0.0, speed=0.005, tlane=2)   # not_zero(speed)
    _put(st, 5, 4, 600.0, 8.0, tspeed=35.0)            # v0 = the speed limit
    _put(st, 5, 5, 700.0, 4.0, speed=5.0, tspeed=-5.0)  # v0 = 0, not_zero(v0)
    # 6: headings next to +-pi and beyond
    for i, hd in enumerate((3.1, -3.1, 3.2, -3.2, 6.2), start=1):
        _put(st, 6, i, 300.0 + 100.0 * i, 4.0 * (i % 4), heading=hd, speed=10.0)
    # 7: x < 0 (on the lane down to -5, reachable from 0 on) and the last 5 m of the road
    _put(st, 7, 1, -3.0, 4.0, timer=1.2)            # wants to leave its lane but is at x < 0
    _put(st, 7, 2, 6.0, 4.0, speed=15.0)
    _put(st, 7, 3, -6.0, 8.0)                        # s < -5: on no lane, so not 4's front
    _put(st, 7, 4, -30.0, 8.0, speed=25.0)
    _put(st, 7, 5, 9994.0, 12.0, timer=1.2)          # reachable; its front leaves the lane at 10005
    _put(st, 7, 0, 10003.5, 12.0, speed=15.0)
    a[7] = (0.0, 0.0)
    return st, a


def craft_pairs(cfg, st):
    """two or three vehicles: not_zero's floor, the rectangles, the impact's frame, an absent
    slot, and the MOBIL gain, braking veto and pre-check radius next to their constants"""
    _clear(cfg, st)
    a = np.zeros((cfg.num_envs, 2), np.float32)
    # 0, 1: a follower at d = 0 and at d just under 0.01 (the front car 2.5 m aside: no overlap)
    for e, d in ((0, 0.0), (1, 0.009)):
        _put(st, e, 1, 300.0, 4.0)
        _put(st, e, 2, 300.0 + d, 6.5, lane=2)
    # 2: overlapping rectangles
    _put(st, 2, 1, 300.0, 4.0)
    _put(st, 2, 2, 303.0, 4.5)
    # 3: will intersect within the next frame; the impact lands one frame later
    _put(st, 3, 1, 300.0, 4.0, speed=30.0)
    _put(st, 3, 2, 307.5, 4.0, speed=5.0)
    # 4: an absent slot between two present ones keeps its words and is nobody's neighbour
    _put(st, 4, 1, 300.0, 4.0)
    _put(st, 4, 2, 310.0, 4.0, flags=0)
    _put(st, 4, 3, 320.0, 4.0, speed=15.0)
    # 5: a gain of 3 (40 / 154.53)^2 = 0.201: a lane change at 0.2, none at 0.202
    _put(st, 5, 1, 300.0, 4.0, timer=1.2)
    _put(st, 5, 2, 300.0 + 40.0 * np.sqrt(3.0 / 0.201), 4.0)
    # 6: the new follower would brake at 3 (40 / 48.87)^2 = 2.01: vetoed at 2, allowed at 2.02
    _put(st, 6, 1, 300.0, 4.0, timer=1.2)
    _put(st, 6, 2, 315.0, 4.0)
    _put(st, 6, 3, 300.0 - 40.0 / np.sqrt(2.01 / 3.0), 8.0)
    # 7: head-on at 6.655 m after the step (both crashed already: they coast with acc = -v):
    # outside sqrt(29) + 18.67 / 15 = 6.630, inside 1.01 sqrt(29) + 18.67 / 15 = 6.683
    _put(st, 7, 1, 300.0, 4.0, flags=_P | _abi.FLAG_CRASHED)
    _put(st, 7, 2, 309.3056, 4.0, heading=3.0, flags=_P | _abi.FLAG_CRASHED)
    return st, a


def _dyn_cases():
    full = dict(started=1, aborts=1, crossings=1, timer_resets=1, impacts=1, new_crashes=1, slow=1)
    some = dict(started=1, crossings=1, timer_resets=1)
    return [
        DynCase("dyn-default", {}, need=full),
        # seeds 6 and 5: with seed 0 these two leave out 7.9 % and 10.9 % of their pairs, nearly all
        # of them wrecks at rest bumper to bumper, whose will-intersect test sits on its edge
        DynCase("dyn-5-over-5", dict(simulation_frequency=5, policy_frequency=5), need=full, seed=6),
        DynCase("dyn-density-3", dict(vehicles_density=3), need=full, seed=5),
        DynCase("dyn-lanes-1", dict(lanes_count=1), need=dict(timer_resets=1),
                never=("started", "crossings")),
        DynCase("dyn-lanes-2", dict(lanes_count=2), need=some),
        DynCase("dyn-lanes-8", dict(lanes_count=8), need=some),
        DynCase("dyn-limit-20", dict(speed_limit=20), need=some),
        DynCase("dyn-V64", dict(vehicles_count=63), need=some),
        DynCase("dyn-V2", dict(vehicles_count=1), need=dict(timer_resets=1)),
        DynCase("dyn-actions-beyond-1", {}, need=dict(some, action_clipped=1), actions=beyond_one,
                seed=2),
        DynCase("dyn-crafted-singles", dict(vehicles_count=5), craft=craft_singles, E=8, steps=4,
                need=dict(over_40=4, slow_fired=1, started=1, absent=1, timer_resets=4, v0_clipped=2)),
        DynCase("dyn-crafted-pairs", dict(vehicles_count=5), craft=craft_pairs, E=8, steps=4,
                need=dict(new_crashes=4, impacts=2, impact_applied=2, started=2, absent=1,
                          timer_resets=2)),
    ]


DYN_CASES = _dyn_cases()
GROUPED_DYN = ("dyn-default", "dyn-lanes-8", "dyn-crafted-pairs")  # one hwy_step_group launch


class DynChecker:
    """One case's frames against dyn_model.frame_model: the after-state of every step within
    TOL_FACTOR times the model's bound of the same step's before-state (bound 0: equal), on the
    envs the model does not call uncertain; the branch counts; the worst error per field."""

    def __init__(self, case, cfg, consts=None):
        self.case, self.cfg, self.consts = case, cfg, consts
        self.count = {k: 0 for k in ("started", "aborts", "crossings", "timer_resets", "impacts",
                                     "new_crashes", "slow", "v0_clipped", "action_clipped",
                                     "over_40", "slow_fired", "absent", "impact_applied")}
        self.pairs = self.left_out = 0
        self.worst = {}
        self.why = {}
        self.t = 0

    def _exact(self, what, got, want, keep):
        bad = (got != want) & keep[:, None] if got.ndim == 2 else (got != want) & keep
        assert not bad.any(), (f"{self.case.name} frame {self.t} {what} at "
                               f"{np.argwhere(bad)[0].tolist()}: got {got[bad][0]!r}, model "
                               f"{want[bad][0]!r}")

    def _within(self, what, got, q, keep):
        got = np.asarray(got, np.float64)
        err = np.abs(got - q.v)
        tol = TOL * q.e
        k = keep[:, None] if got.ndim == 2 else keep
        bad = (err > tol) & k
        if bad.any():
            i = tuple(np.argwhere(bad)[0])
            raise AssertionError(f"{self.case.name} frame {self.t} {what} at {list(i)}: got "
                                 f"{got[i]!r}, model {q.v[i]!r}, error {err[i]:.3g} > bound "
                                 f"{tol[i]:.3g}")
        ratio = np.where((tol > 0) & k, err / np.where(tol > 0, tol, 1.0), 0.0)
        if ratio.size:
            i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
            w = self.worst.get(what, (0.0, 0.0))
            if w[1] == 0.0 or ratio[i] > w[0] / w[1]:
                self.worst[what] = (float(err[i]), float(tol[i]))

    def check(self, before, actions, after, reward):
        import dyn_model as dm

        cfg = self.cfg
        V = cfg.vehicles_count + 1
        model, unc = dm.frame_model(cfg, before, actions, self.consts)
        keep = ~unc
        for k, n in model["why"].items():
            self.why[k] = self.why.get(k, 0) + n
        self.pairs += unc.size
        self.left_out += int(unc.sum())
        for name, f in dm.FLOAT_FIELDS.items():
            self._within(name, after[f].view(np.float32)[:, :V], model[name], keep)
        for name, f in dm.INT_FIELDS.items():
            self._exact(name, after[f][:, :V].astype(np.int32).astype(np.int64), model[name], keep)
        fl = after[_abi.F_FLAGS][:, :V].astype(np.int64)
        self._exact("flags", fl & dm.FLAG_MASK, model["flags"], keep)
        # the order bits are the road order of the after-state's own positions: stored words,
        # exact, on every env
        self._exact("road order", fl >> _abi.FLAG_ORDER_SHIFT, dm.road_order(cfg, after),
                    np.ones_like(keep))
        eb, ea = before[_abi.F_ENV], after[_abi.F_ENV]
        everyone = np.ones_like(keep)
        self._exact("step count", ea[:, _abi.E_STEP].astype(np.int64),
                    eb[:, _abi.E_STEP].astype(np.int64) + 1, everyone)
        for w in (_abi.E_EPISODE, _abi.E_SEED_LO, _abi.E_SEED_HI):
            self._exact(f"env word {w}", ea[:, w], eb[:, w], everyone)
        fa = ea.view(np.float32)
        self._within("ego_acc", fa[:, _abi.E_EGO_ACC], model["ego_acc"], everyone)
        self._within("ego_steer", fa[:, _abi.E_EGO_STEER], model["ego_steer"], everyone)
        ret = em.Q(eb.view(np.float32)[:, _abi.E_RETURN].astype(np.float64)) + \
            em.Q(np.asarray(reward, np.float32).astype(np.float64))
        self._within("return", fa[:, _abi.E_RETURN], ret, everyone)
        self._cover(dm.unpack(cfg, before), dm.unpack(cfg, after), actions)
        self.t += 1

    def _cover(self, b, a, actions):
        c = self.count
        tr = b["present"].copy()
        tr[:, 0] = False
        steady = tr & ~b["crashed"] & (b["lane"] == b["target_lane"])
        fired = steady & (b["timer"] > 1.0)
        c["started"] += int((steady & (a["target_lane"] != b["lane"])).sum())
        c["aborts"] += int((tr & (b["lane"] != b["target_lane"]) & (a["target_lane"] == b["lane"])).sum())
        c["crossings"] += int((tr & (a["lane"] != b["lane"])).sum())
        c["timer_resets"] += int(fired.sum())
        c["impacts"] += int(a["impact"].sum())
        c["impact_applied"] += int((b["impact"] & b["present"] & a["crashed"]).sum())
        c["new_crashes"] += int((a["crashed"] & ~b["crashed"]).sum())
        c["slow"] += int((tr & (np.abs(b["speed"]) < 1.0)).sum())
        c["slow_fired"] += int((fired & (np.abs(b["speed"]) < 1.0)).sum())
        c["v0_clipped"] += int((tr & ((b["target_speed"] > float(self.cfg.speed_limit)) |
                                        (b["target_speed"] < 0.0))).sum())
        c["action_clipped"] += int((np.abs(actions) > 1.0).sum())
        c["over_40"] += int((np.abs(b["speed"][:, 0]) > 40.0).sum())
        c["absent"] += int((~b["present"]).sum())

    def report(self):
        share = self.left_out / max(self.pairs, 1)
        worst = ", ".join(f"{k} {e:.2e}/{b:.2e}" for k, (e, b) in self.worst.items() if b > 0)
        return (f"{self.case.name}: worst error/bound {worst}; uncertain {self.left_out}/"
                f"{self.pairs} = {100 * share:.2f} % by { {k: v for k, v in self.why.items() if v} }; counts "
                f"{ {k: v for k, v in self.count.items() if v} }")

    def finish(self):
        print(self.report())
        for k, least in self.case.need.items():
            assert self.count[k] >= least, f"{self.case.name}: {k} occurred {self.count[k]} times, need {least}"
        for k in self.case.never:
            assert self.count[k] == 0, f"{self.case.name}: {k} occurred {self.count[k]} times"
        # a cap, not a target: a case over it gets another seed or other inputs
        assert self.left_out <= 0.05 * self.pairs, self.report()


TOL = em.TOL_FACTOR
_TRACES = {}


def dyn_trace(case):
    """The case on the CPU oracle, once: [(state before, actions, state after, reward)] per
    frame.  Shared by the tests of tests/test_dyn_model.py and left unchanged."""
    if case.name not in _TRACES:
        cfg = case.make()
        init, action_fn = case.start(cfg)
        ora = OracleEnv(cfg)
        ora.reset()
        if init is not None:
            ora.state[...] = init
        rng = np.random.default_rng(case.seed)
        frames = []
        for t in range(case.steps):
            before = ora.state.copy()
            a = np.ascontiguousarray(action_fn(rng, cfg.num_envs, t), np.float32)
            out = ora.step(a)
            frames.append((before, a, ora.state.copy(), out[1].copy()))
        _TRACES[case.name] = (cfg, frames)
    return _TRACES[case.name]


def run_dyn_case_on_oracle(case, consts=None):
    """The case's oracle frames against the model (with `consts` over dyn_model.CONSTS): the
    DynChecker, not yet finished."""
    cfg, frames = dyn_trace(case)
    ck = DynChecker(case, cfg, consts)
    for before, a, after, rew in frames:
        ck.check(before, a, after, rew)
    return ck
