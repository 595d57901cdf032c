"""The env parity driver shared by the GPU parity tests, and the config-space case table with
its checker against tests/env_model.py (shared by the CPU and the GPU run of the cases).

torch and libhwy.so are imported only when a HipEnv is built, so the CPU tests can import the
case table and the checker without a GPU.
"""

from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

import env_model as em
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

    def reset(self, seeds=None):
        from hwy.native import check, lib, ptr

        torch = self.torch
        s = None if seeds is None else torch.as_tensor(seeds.astype(np.int64), device=self.dev)
        check(lib().hwy_reset(self.h, ptr(s), None, ptr(self.obs), None), "hwy_reset")
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


def run_parity(cfg, steps, table=None, seed=0, action_fn=policy_actions, hook=None):
    """hook (optional): called after every step's comparisons with
    (cfg, hip outputs, hip state, oracle outputs)."""
    hip = HipEnv(cfg, table)
    ora = OracleEnv(cfg, table)
    V = cfg.vehicles_count + 1
    try:
        o_h = hip.reset()
        o_o = ora.reset()
        d = diff_state(hip.state(), ora.state, V)
        assert d is None, f"reset state: {d}"
        np.testing.assert_array_equal(o_h, o_o, err_msg="reset obs")
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
def _perfect_matching(M):
    """Kuhn's augmenting paths on a boolean [n, n] matrix: the column of every row if each
    row gets its own, else None."""
    n = M.shape[0]
    owner = [-1] * n
    adj = [np.nonzero(M[i])[0] for i in range(n)]

    def place(i, seen):
        for j in adj[i]:
            if j in seen:
                continue
            seen.add(j)
            if owner[j] < 0 or place(owner[j], seen):
                owner[j] = i
                return True
        return False

    if not all(place(i, set()) for i in range(n)):
        return None
    col = [0] * n
    for j, i in enumerate(owner):
        col[i] = j
    return col


class Checker:
    """One case's outputs (the kernel's or the oracle's) against the float64 model, step by
    step; collects the coverage counts, the share of (env, step) pairs `uncertain` leaves out
    and the worst error against the derived bound."""

    def __init__(self, case, cfg, table):
        self.case, self.cfg, self.table = case, cfg, table
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

    def _rows_match(self, K, W):
        """[n, m] bool: kernel row i within the bound of model row j, every column"""
        err = np.abs(K[:, None, :].astype(np.float64) - W.v[None, :, :])
        return (err <= em.TOL_FACTOR * W.e[None, :, :]).all(-1)

    def _check_obs(self, obs, m, keep):
        cfg, table = self.cfg, self.table
        N, F = cfg.obs_vehicles, cfg.n_features
        rank = cfg.pe_kind == _abi.PE_RANK
        if rank:  # the appended columns are the table's row for the position, exactly
            t = np.asarray(table, np.float32).reshape(N, cfg.d_embed)
            np.testing.assert_array_equal(obs[:, :, F:], np.broadcast_to(t, obs[:, :, F:].shape))
        if not (cfg.order == _abi.ORDER_SHUFFLED and N > 2):
            w = em.wrap_model(cfg, m, table)
            self._within("obs", obs[keep], w[keep])
            return
        # shuffled: as a set.  Row 0 is the ego; every other kernel row matches exactly one model
        # row (so the zero-row counts are equal too).  The wrapper measures distances from the
        # row at ego_idx, so with ego_idx >= 1 the model row standing there is searched for.
        eg = int(cfg.ego_idx)
        for e in np.nonzero(keep)[0]:
            me = m[e]
            K = obs[e, :, :F] if rank else obs[e]
            zero = np.nonzero(~me.v[1:].any(-1))[0] + 1
            cands = [0] if eg == 0 else [j for j in range(1, N) if j not in zero[1:]]
            ok = False
            for c in cands:
                ref = em.Q(np.broadcast_to(me.v[c], me.v.shape), np.broadcast_to(me.e[c], me.e.shape))
                W = me if rank else em.wrap_rows(cfg, me, ref, table)
                M = self._rows_match(K, W)
                if not M[0, 0]:
                    continue
                M = M[1:, 1:].copy()
                if eg >= 1:  # position ego_idx holds model row c
                    keep_cell = M[eg - 1, c - 1]
                    M[eg - 1, :] = False
                    M[:, c - 1] = False
                    M[eg - 1, c - 1] = keep_cell
                col = _perfect_matching(M)
                if col is not None:
                    ok = True
                    # the figure reported is each row against the nearest model row it may be
                    # (rows closer to each other than the bound are interchangeable)
                    err = np.abs(K[:, None, :].astype(np.float64) - W.v[None]).sum(-1)
                    err[1:, 1:][~M] = np.inf
                    err[0, 1:] = err[1:, 0] = np.inf
                    self._within("obs", K, W[np.argmin(err, 1)])
                    break
            assert ok, (f"{self.case.name} step {self.t} env {e}: the kernel's rows are not a "
                        f"permutation of the model's rows within the bound\nkernel\n{obs[e]}\n"
                        f"model (before the wrapper)\n{me.v}")
            if cfg.pe_kind in (_abi.PE_NONE, _abi.PE_RANK):
                assert int((K[1:] == 0).all(-1).sum()) == len(zero), "zero-row counts differ"

    def check(self, out, state):
        """out: (obs, reward, terminated, truncated, ...) of one step; state: the packed state
        after it."""
        cfg = self.cfg
        obs, rew, term, trunc = (np.asarray(x) for x in out[:4])
        unc = em.uncertain(cfg, state)
        self.pairs += unc.size
        self.left_out += int(unc.sum())
        m = em.observe_model(cfg, state)
        self._check_obs(obs, m, ~unc)
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
