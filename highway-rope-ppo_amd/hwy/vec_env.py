"""HighwayVecEnv: thousands of lockstep highway-v0 envs on one MI355X, behind libhwy.so.

Replaces ``gym.make("highway-v0", config=cfg)`` (experiments/wrappers.py:80) with a batched,
device-resident env.  ``reset`` / ``step`` mirror the gymnasium 1.x contract the reference's
training loop uses (training/routine.py:18-26,127-135) with a leading env axis and torch device
tensors instead of numpy:

    obs, info = env.reset(seed=base)                     # obs: [E, N, F_out] float32
    obs, reward, terminated, truncated, info = env.step(actions)   # actions: [E, 2] in [-1, 1]

With ``autoreset=True`` finished envs restart inside the step kernel with the next seed of the
episode schedule (include/hwy.h) and ``info["episode_return"/"episode_length"]`` report the
finished episode (0 elsewhere).  Every call is asynchronous on the current HIP stream.

``info=True`` opts into upstream's per-step info (AbstractEnv._info / HighwayEnv._rewards) for
the ego of every env -- ``info["speed"]``, ``["crashed"]``, ``["lane"]``, ``["rewards"]`` (a dict
of the four unweighted terms) -- and ``info["episode_stats"]`` ([E, 8]: where an episode finished,
its sums of speed and of the four terms, its lane-change count and its crashed flag; the slots
are _abi.ACC_*).  The step then runs the info variant of the kernel (hwy_step_with_info), which
computes the same step and stores these besides.

``final_obs=True`` completes the autoreset contract: ``info["final_observation"]`` ([E, N, F_out])
holds, where ``info["_final_observation"]`` (= terminated | truncated) is set, the last observation
of the episode that just finished -- the row the in-kernel reset overwrote in ``obs``.  Other rows
keep what an earlier step wrote there.  The step then runs the final variant of the kernel
(hwy_step_with_final), with the info outputs too when ``info=True``.

``render`` draws the envs' current states as uint8 frames on the device (hwy_render: the frame
rule of include/hwy.h at the config's ``screen_width`` / ``screen_height`` / ``scaling`` /
``centering_position``), one launch for any number of envs.
"""

from __future__ import annotations

import ctypes
import copy
from typing import Any, Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

from . import _abi
from ._abi import (HWY_INFO_NACC, HWY_MAX_VEHICLES, NFIELDS, PE_NONE, REWARD_KEYS, HwyStepInfo,
                   config_from_dict)
from .gym import spaces
from .native import (HwyNativeError, HwyStepGroupPlan, HwyStepIO, check, lib, ptr,
                     stream_ptr)

INFO_FIELDS = tuple(n for n, _ in HwyStepInfo._fields_)


def alloc_step_info(num_envs: int, device) -> Dict[str, torch.Tensor]:
    """Device tensors for every output of hwy_step_with_info, keyed by hwy_step_info's fields."""
    E, kw = int(num_envs), dict(device=device)
    return {"speed": torch.zeros(E, dtype=torch.float32, **kw),
            "crashed": torch.zeros(E, dtype=torch.uint8, **kw),
            "lane": torch.zeros(E, dtype=torch.int32, **kw),
            "rewards": torch.zeros(E, 4, dtype=torch.float32, **kw),
            "acc": torch.zeros(E, HWY_INFO_NACC, dtype=torch.float32, **kw),
            "ep_stats": torch.zeros(E, HWY_INFO_NACC, dtype=torch.float32, **kw)}


def _info_ptrs(info: Dict[str, Any]) -> tuple:
    """hwy_step_info's pointers from a dict of caller-owned tensors (missing / None = NULL)."""
    unknown = set(info) - set(INFO_FIELDS)
    if unknown:
        raise ValueError(f"unknown step info outputs {sorted(unknown)}; known: {INFO_FIELDS}")
    return tuple(ptr(info.get(n)) for n in INFO_FIELDS)


def _check_final_obs(env, t: torch.Tensor) -> None:
    """A terminal-observation buffer of ``env``: E x N x F_out contiguous float32 on its device."""
    n = env.num_envs * env.obs_rows * env.obs_features
    if not (t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n):
        raise ValueError(f"final_obs must be a contiguous float32 device tensor of {n} elements "
                         f"(E x N x F_out), got {tuple(t.shape)} {t.dtype} on {t.device}")


def _dev_tensor(name: str, t, dtype, n: int, what: str, device) -> int:
    """The device pointer of ``t``, a contiguous ``dtype`` tensor of ``n`` elements (``what``: their
    layout, for the message) on ``device``; anything else is a ValueError."""
    if not (isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_contiguous()
            and t.numel() == n and t.device == torch.device(device)):
        raise ValueError(f"{name} must be a contiguous {dtype} tensor of {n} elements "
                         f"({what}) on {device}, got "
                         f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)} "
                         f"{getattr(t, 'dtype', None)} on {getattr(t, 'device', None)}")
    return t.data_ptr()


def _set_outputs(a, table, device) -> bool:
    """Set the pointers of args struct ``a`` from ``table``, rows of (field of ``a``, the name the
    caller knows it by, tensor or None, dtype, elements, layout): every tensor that is given goes
    through _dev_tensor.  Returns whether any was given."""
    given = False
    for field, name, t, dtype, n, what in table:
        if t is not None:
            setattr(a, field, _dev_tensor(name, t, dtype, n, what, device))
            given = True
    return given


def observe_args(num_envs: int, rows: int, fout: int, device, order=None, *, obs=None,
                 row_vehicle=None, row_values=None, veh_values=None) -> _abi.ObserveArgs:
    """hwy_observe_args for an env of ``num_envs`` x ``rows`` x ``fout`` on ``device`` from
    caller-owned tensors, every refusal a ValueError (no device call, no library call)."""
    a = _abi.ObserveArgs()
    a.order = _abi.observe_order(order)
    E, N = int(num_envs), int(rows)
    _set_outputs(a, (("obs", "obs", obs, torch.float32, E * N * int(fout), "E x N x F_out"),
                     ("row_vehicle", "row_vehicle", row_vehicle, torch.int32, E * N, "E x N"),
                     ("row_values", "row_values", row_values, torch.float32, E * N, "E x N"),
                     ("veh_values", "veh_values", veh_values, torch.float32,
                      E * HWY_MAX_VEHICLES, "E x 64")), device)
    if obs is None and row_vehicle is None and veh_values is None:
        raise ValueError("observe_into needs at least one of obs, row_vehicle and veh_values")
    if (row_values is None) != (veh_values is None):
        raise ValueError("row_values and veh_values go together")
    return a


TRAFFIC_OUTPUTS = _abi.TRAFFIC_VEHICLE_OUTPUTS + ("ego", "acc", "ep_stats")


def alloc_traffic(num_envs: int, device) -> Dict[str, torch.Tensor]:
    """Device tensors for every output of hwy_traffic, keyed by hwy_traffic_args' fields; ``acc``
    is zero-filled as the running reduction's contract asks."""
    E, kw = int(num_envs), dict(device=device)
    out = {n: torch.zeros(E, HWY_MAX_VEHICLES, dtype=torch.int32 if n in ("front", "rear")
                          else torch.float32, **kw) for n in _abi.TRAFFIC_VEHICLE_OUTPUTS}
    out["ego"] = torch.zeros(E, _abi.HWY_TRAFFIC_NEGO, dtype=torch.float32, **kw)
    out["acc"] = torch.zeros(E, _abi.HWY_TRAFFIC_NACC, dtype=torch.float32, **kw)
    out["ep_stats"] = torch.zeros(E, _abi.HWY_TRAFFIC_NACC, dtype=torch.float32, **kw)
    return out


def traffic_args(num_envs: int, device, *, restart=(), ttc_thresh=None, thw_thresh=None,
                 risk_horizon=None, near_range=None, **outputs) -> _abi.TrafficArgs:
    """hwy_traffic_args for ``num_envs`` envs on ``device`` from caller-owned tensors (``outputs``
    by hwy_traffic_args' field names, None = not wanted; ``restart`` up to three [E] uint8 masks),
    every refusal a ValueError (no device call, no library call)."""
    unknown = set(outputs) - set(TRAFFIC_OUTPUTS)
    if unknown:
        raise ValueError(f"unknown traffic outputs {sorted(unknown)}; known: {TRAFFIC_OUTPUTS}")
    a = _abi.TrafficArgs()
    E = int(num_envs)
    widths = {"ego": _abi.HWY_TRAFFIC_NEGO, "acc": _abi.HWY_TRAFFIC_NACC,
              "ep_stats": _abi.HWY_TRAFFIC_NACC}
    _set_outputs(a, [(n, n, outputs.get(n), torch.int32 if n in ("front", "rear")
                      else torch.float32, E * widths.get(n, HWY_MAX_VEHICLES),
                      f"E x {widths.get(n, HWY_MAX_VEHICLES)}") for n in TRAFFIC_OUTPUTS], device)
    if all(outputs.get(n) is None for n in TRAFFIC_OUTPUTS if n != "ep_stats"):
        raise ValueError("traffic_into needs at least one output besides ep_stats")
    masks = [m for m in (restart or ()) if m is not None]
    if len(masks) > 3:
        raise ValueError(f"at most three restart masks, got {len(masks)}")
    has_acc = outputs.get("acc") is not None
    if outputs.get("ep_stats") is not None and not has_acc:
        raise ValueError("ep_stats needs acc")
    if masks and not has_acc:
        raise ValueError("restart masks need acc")
    for k, m in enumerate(masks):
        a.restart[k] = _dev_tensor(f"restart[{k}]", m, torch.uint8, E, "E", device)
    given = {"ttc_thresh": ttc_thresh, "thw_thresh": thw_thresh, "risk_horizon": risk_horizon,
             "near_range": near_range}
    for name, default in _abi.TRAFFIC_DEFAULTS.items():
        val = default if given[name] is None else float(given[name])
        if not (0.0 < ctypes.c_float(val).value < float("inf")):  # as the float32 the call takes
            raise ValueError(f"{name} must be finite and > 0, got {val!r}")
        setattr(a, name, val)
    return a


def sense_args(num_envs: int, rows: int, fout: int, device, sensor, order=None, *, obs=None,
               row_vehicle=None, visible=None, hidden=None, counts=None) -> _abi.SenseArgs:
    """hwy_sense_args for an env of ``num_envs`` x ``rows`` x ``fout`` on ``device`` from a
    SensorModel (or its dict) and caller-owned tensors, every refusal a ValueError (no device
    call, no library call)."""
    a = _abi.SensorModel.from_dict(sensor).fill(_abi.SenseArgs())
    a.order = _abi.observe_order(order)
    E, N = int(num_envs), int(rows)
    if not _set_outputs(a, (
            ("obs", "obs", obs, torch.float32, E * N * int(fout), "E x N x F_out"),
            ("row_vehicle", "row_vehicle", row_vehicle, torch.int32, E * N, "E x N"),
            ("visible", "visible", visible, torch.uint8, E * HWY_MAX_VEHICLES, "E x 64"),
            ("hidden", "hidden", hidden, torch.float32, E * HWY_MAX_VEHICLES, "E x 64"),
            ("counts", "counts", counts, torch.int32, E * 4, "E x 4")), device):
        raise ValueError("sense_into needs at least one of obs, row_vehicle, visible, hidden and "
                         "counts")
    return a


def grid_args(num_envs: int, n_features: int, device, spec, *, out=None, cell_vehicle=None,
              veh_cell=None, counts=None) -> _abi.GridArgs:
    """hwy_grid_args for ``num_envs`` envs of ``n_features`` Kinematics features on ``device`` from
    a GridSpec (its dict, or True for the default) and caller-owned tensors, every refusal a
    ValueError (no device call, no library call)."""
    g = _abi.GridSpec.from_dict(spec)
    a = g.fill(_abi.GridArgs(), n_features)
    E, cells = int(num_envs), g.nx * g.ny
    if not _set_outputs(a, (
            ("grid", "out", out, torch.float32, E * a.row_stride, f"E x {a.row_stride}"),
            ("cell_vehicle", "cell_vehicle", cell_vehicle, torch.int32, E * cells,
             f"E x {g.nx} x {g.ny}"),
            ("veh_cell", "veh_cell", veh_cell, torch.int32, E * HWY_MAX_VEHICLES, "E x 64"),
            ("counts", "counts", counts, torch.int32, E * 4, "E x 4")), device):
        raise ValueError("grid_into needs at least one of out, cell_vehicle, veh_cell and counts")
    return a


def lidar_args(num_envs: int, n_features: int, device, spec, *, out=None, hit_vehicle=None,
               seen=None, counts=None) -> _abi.LidarArgs:
    """hwy_lidar_args for ``num_envs`` envs of ``n_features`` Kinematics features on ``device``
    from a LidarSpec (its dict, or True for the default) and caller-owned tensors, every refusal a
    ValueError (no device call, no library call)."""
    g = _abi.LidarSpec.from_dict(spec)
    a = g.fill(_abi.LidarArgs(), n_features)
    E = int(num_envs)
    if not _set_outputs(a, (
            ("obs", "out", out, torch.float32, E * a.row_stride, f"E x {a.row_stride}"),
            ("hit_vehicle", "hit_vehicle", hit_vehicle, torch.int32, E * g.cells,
             f"E x {g.cells}"),
            ("seen", "seen", seen, torch.float32, E * HWY_MAX_VEHICLES, "E x 64"),
            ("counts", "counts", counts, torch.int32, E * 4, "E x 4")), device):
        raise ValueError("lidar_into needs at least one of out, hit_vehicle, seen and counts")
    return a


def lookahead_args(num_envs: int, rows: int, fout: int, device, actions, horizon: int, *,
                   hold: bool = False, lazy: bool = False, gamma: float = 1.0, steps=None,
                   terminated=None, truncated=None, rewards=None, ret=None, ego_final=None,
                   obs=None, chosen=None, chosen_action=None) -> _abi.LookaheadArgs:
    """hwy_lookahead_args for an env of ``num_envs`` x ``rows`` x ``fout`` on ``device`` from
    caller-owned tensors, every refusal a ValueError (no device call, no library call).  K is read
    off ``actions``: [E, K, 2] with ``hold``, else [E, K, H, 2]."""
    E, N = int(num_envs), int(rows)
    try:
        H = int(horizon)
        g = float(gamma)
    except (TypeError, ValueError):
        raise ValueError(f"bad horizon {horizon!r} or gamma {gamma!r}") from None
    if H != horizon or not 1 <= H <= _abi.LOOKAHEAD_MAX_H:
        raise ValueError(f"horizon must be an integer in 1..{_abi.LOOKAHEAD_MAX_H}, "
                         f"got {horizon!r}")
    if not 0.0 <= g <= 1.0:  # a NaN fails
        raise ValueError(f"gamma must be finite and lie in [0, 1], got {gamma!r}")
    dev = torch.device(device)
    want = (E, -1, 2) if hold else (E, -1, H, 2)
    if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.float32
            and actions.is_contiguous() and actions.device == dev
            and actions.dim() == len(want) and actions.shape[1] >= 1
            and all(w in (-1, int(n)) for w, n in zip(want, actions.shape))):
        raise ValueError(f"actions must be a contiguous float32 tensor "
                         f"{'[E, K, 2]' if hold else '[E, K, H, 2]'} (E {E}, H {H}) on {dev}, got "
                         f"{tuple(actions.shape) if hasattr(actions, 'shape') else type(actions)} "
                         f"{getattr(actions, 'dtype', None)} on {getattr(actions, 'device', None)}")
    K = int(actions.shape[1])
    if K > _abi.LOOKAHEAD_MAX_K or E * K > _abi.LOOKAHEAD_MAX_BRANCHES:
        raise ValueError(f"K must lie in 1..{_abi.LOOKAHEAD_MAX_K} and E * K be at most "
                         f"{_abi.LOOKAHEAD_MAX_BRANCHES}, got K {K}, E {E}")
    a = _abi.LookaheadArgs()
    a.k, a.horizon, a.hold, a.lazy, a.gamma = K, H, int(bool(hold)), int(bool(lazy)), g
    a.actions = actions.data_ptr()
    if not _set_outputs(a, (
            ("steps", "steps", steps, torch.int32, E * K, "E x K"),
            ("terminated", "terminated", terminated, torch.uint8, E * K, "E x K"),
            ("truncated", "truncated", truncated, torch.uint8, E * K, "E x K"),
            ("rewards", "rewards", rewards, torch.float32, E * K * H, "E x K x H"),
            ("ret", "ret", ret, torch.float32, E * K, "E x K"),
            ("ego_final", "ego_final", ego_final, torch.float32, E * K * 4, "E x K x 4"),
            ("obs", "obs", obs, torch.float32, E * K * N * int(fout), "E x K x N x F_out"),
            ("chosen", "chosen", chosen, torch.int32, E, "E"),
            ("chosen_action", "chosen_action", chosen_action, torch.float32, E * 2, "E x 2")),
            dev):
        raise ValueError("lookahead_into needs at least one output: "
                         + ", ".join(_abi.LOOKAHEAD_OUTPUTS))
    if (lazy or chosen is not None) and (steps is None or terminated is None):
        raise ValueError("lazy and chosen need the steps and terminated outputs")
    if chosen_action is not None and chosen is None:
        raise ValueError("chosen_action needs chosen")
    return a


class HighwayVecEnv:
    """E lockstep highway-v0 envs with state resident in HBM (one wavefront per env)."""

    is_vector_env = True

    def __init__(self, config: Dict[str, Any], num_envs: int = 1,
                 device: Optional[torch.device] = None, autoreset: bool = True,
                 seed_base: int = 0, env_offset: int = 0, global_envs: Optional[int] = None,
                 pe_kind: int = PE_NONE, d_embed: int = 0, pe_table: Optional[np.ndarray] = None,
                 ego_idx: int = 0, pe_max_dist: float = 100.0, info: bool = False,
                 final_obs: bool = False):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        device = torch.device(device)
        if device.type != "cuda":
            raise HwyNativeError(
                f"HighwayVecEnv runs on a HIP device only (got {device}); there is no CPU path")
        if device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.config = copy.deepcopy(config)
        self.device = device
        self.num_envs = int(num_envs)
        self._handle = ctypes.c_void_p()
        self._cfg = config_from_dict(self.config, num_envs=num_envs, autoreset=autoreset,
                                     env_offset=env_offset, seed_base=seed_base,
                                     seed_stride=global_envs if global_envs else num_envs,
                                     pe_kind=pe_kind, d_embed=d_embed, ego_idx=ego_idx,
                                     pe_max_dist=pe_max_dist)
        self._pe_table = None if pe_table is None else np.ascontiguousarray(pe_table, np.float32)
        self._final_obs = bool(final_obs)
        self._create()
        self._alloc_buffers()
        # the opt-in step info: buffers owned by the env (None: step() is the plain hwy_step)
        self.info_buf = alloc_step_info(self.num_envs, self.device) if info else None
        self.action_space = spaces.Box(-1.0, 1.0, shape=(2,), dtype=np.float32)
        self._set_obs_space()

    # ------------------------------------------------------------------ setup
    def _create(self):
        # bumped whenever a launch argument a captured rollout graph bakes in changes (handle,
        # seed schedule, PE table): ppo/rollout.py re-captures then
        self.launch_version = getattr(self, "launch_version", 0) + 1
        with torch.cuda.device(self.device):
            h = ctypes.c_void_p()
            check(lib().hwy_create(ctypes.byref(self._cfg), self.device.index, ctypes.byref(h)),
                  "hwy_create")
            if self._pe_table is not None and self._pe_table.size:
                rc = lib().hwy_set_pe_table(h, self._pe_table.ctypes.data_as(ctypes.c_void_p),
                                            int(self._pe_table.size))
                if rc:
                    lib().hwy_destroy(h)
                    check(rc, "hwy_set_pe_table")
            self._handle = h

    def _alloc_buffers(self):
        E, N, Fo = self.num_envs, self.obs_rows, self.obs_features
        kw = dict(device=self.device)
        self.obs_buf = torch.zeros(E, N, Fo, dtype=torch.float32, **kw)
        self.reward_buf = torch.zeros(E, dtype=torch.float32, **kw)
        self.term_buf = torch.zeros(E, dtype=torch.uint8, **kw)
        self.trunc_buf = torch.zeros(E, dtype=torch.uint8, **kw)
        self.ep_ret_buf = torch.zeros(E, dtype=torch.float32, **kw)
        self.ep_len_buf = torch.zeros(E, dtype=torch.int32, **kw)
        # the opt-in terminal observations (None: step() never runs the final variant)
        self.final_obs_buf = (torch.zeros(E, N, Fo, dtype=torch.float32, **kw)
                              if getattr(self, "_final_obs", False) else None)

    def _set_obs_space(self):
        N, Fo = self.obs_rows, self.obs_features
        self.single_observation_space = spaces.Box(-np.inf, np.inf, shape=(N, Fo), dtype=np.float32)
        self.observation_space = self.single_observation_space

    @property
    def hwy_config(self) -> _abi.HwyConfig:
        return self._cfg

    @property
    def obs_rows(self) -> int:
        return int(self._cfg.obs_vehicles)

    @property
    def obs_features(self) -> int:
        return self._cfg.obs_features()

    @property
    def max_episode_steps(self) -> int:
        return int(self._cfg.max_steps)

    def enable_pe(self, kind: int, d: int, table: Optional[np.ndarray], ego_idx: int = 0,
                  max_dist: float = 100.0) -> None:
        """Fuse an observation wrapper into the step kernel (keeps the current env state)."""
        if self._cfg.pe_kind != PE_NONE:
            raise ValueError("an observation wrapper is already fused into this env")
        state = self.export_state() if self._handle else None
        old = self._handle
        new_cfg = _abi.HwyConfig.from_buffer_copy(self._cfg)
        new_cfg.pe_kind, new_cfg.d_embed = int(kind), int(d)
        new_cfg.ego_idx, new_cfg.pe_max_dist = int(ego_idx), float(max_dist)
        prev_cfg, prev_table = self._cfg, self._pe_table
        self._cfg = new_cfg
        self._pe_table = None if table is None else np.ascontiguousarray(table, np.float32)
        try:
            self._create()
        except Exception:
            self._cfg, self._pe_table, self._handle = prev_cfg, prev_table, old
            raise
        if old:
            lib().hwy_destroy(old)
        if state is not None:
            self.import_state(state)
        self._alloc_buffers()
        self._set_obs_space()

    def set_pe_table(self, table: np.ndarray) -> None:
        """Replace the fused wrapper's table (e.g. RankEmbedWrapper.to(device))."""
        t = np.ascontiguousarray(table, np.float32)
        torch.cuda.synchronize(self.device)
        check(lib().hwy_set_pe_table(self._handle, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
              "hwy_set_pe_table")
        self._pe_table = t
        self.launch_version += 1

    # ------------------------------------------------------------------ API
    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None,
              seeds: Optional[torch.Tensor] = None, mask: Optional[torch.Tensor] = None):
        """Reset all envs (or those where ``mask`` is set).

        ``seed`` (int) sets the schedule's base: env e starts episode 0 with seed
        ``seed + env_offset + e + 1`` (training/routine.py:127 for E = 1 is seed + episode_num).
        ``seeds`` ([E] int64 tensor) gives explicit per-env seeds instead.
        """
        if seed is not None:
            self.set_seed_schedule(int(seed))
        s = None
        if seeds is not None:
            s = torch.as_tensor(seeds, device=self.device).to(torch.int64).contiguous()
        m = None
        if mask is not None:
            m = torch.as_tensor(mask, device=self.device).to(torch.uint8).contiguous()
        check(lib().hwy_reset(self._handle, ptr(s), ptr(m), ptr(self.obs_buf), stream_ptr()),
              "hwy_reset")
        self._keep = (s, m)
        return self.obs_buf, {}

    def step(self, actions: torch.Tensor):
        a = actions
        if not (a.is_cuda and a.dtype == torch.float32 and a.is_contiguous()):
            a = torch.as_tensor(a, device=self.device, dtype=torch.float32).contiguous()
        if a.numel() != 2 * self.num_envs:
            raise ValueError(f"actions must have {self.num_envs}x2 elements, got {tuple(a.shape)}")
        self.step_into(a, self.obs_buf, self.reward_buf, self.term_buf, self.trunc_buf,
                       self.ep_ret_buf, self.ep_len_buf, info=self.info_buf,
                       final_obs=self.final_obs_buf)
        self._keep = a
        return self.obs_buf, self.reward_buf, self.term_buf, self.trunc_buf, self._info_dict()

    def _info_dict(self) -> Dict[str, Any]:
        """step()'s info from whichever of the env's own buffers exist."""
        info = {"episode_return": self.ep_ret_buf, "episode_length": self.ep_len_buf}
        if self.final_obs_buf is not None:
            info["final_observation"] = self.final_obs_buf
            info["_final_observation"] = (self.term_buf | self.trunc_buf).bool()
        b = self.info_buf
        if b is not None:
            info.update({"speed": b["speed"], "crashed": b["crashed"], "lane": b["lane"],
                         "rewards": {k: b["rewards"][:, i] for i, k in enumerate(REWARD_KEYS)},
                         "episode_stats": b["ep_stats"]})
        return info

    def step_into(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor,
                  terminated: torch.Tensor, truncated: torch.Tensor,
                  ep_return: Optional[torch.Tensor] = None,
                  ep_length: Optional[torch.Tensor] = None,
                  info: Optional[Dict[str, torch.Tensor]] = None,
                  final_obs: Optional[torch.Tensor] = None) -> None:
        """step() writing straight into caller-owned rollout slices (no copies; graph-safe).
        ``info``: caller-owned tensors for hwy_step_with_info's outputs, keyed by hwy_step_info's
        fields (alloc_step_info's layout; any subset, "ep_stats" needs "acc").
        ``final_obs``: a caller-owned contiguous float32 buffer of E x N x F_out floats for the
        terminal observations of the envs that finish in this step (hwy_step_with_final; rows of
        the other envs are not written); combines with ``info``."""
        if final_obs is not None:
            _check_final_obs(self, final_obs)
        si = None if info is None else ctypes.byref(HwyStepInfo(*_info_ptrs(info)))
        if final_obs is not None:
            name, more = "hwy_step_with_final", (si, ptr(final_obs))
        elif info is not None:
            name, more = "hwy_step_with_info", (si,)
        else:
            name, more = "hwy_step", ()
        check(getattr(lib(), name)(self._handle, ptr(actions), ptr(obs), ptr(reward),
                                   ptr(terminated), ptr(truncated), ptr(ep_return),
                                   ptr(ep_length), *more, stream_ptr()), name)

    def cut_episodes(self, obs: torch.Tensor, ep_return: Optional[torch.Tensor] = None,
                     ep_length: Optional[torch.Tensor] = None,
                     cut: Optional[torch.Tensor] = None) -> None:
        """End every running episode and start the schedule's next one (hwy_cut_episodes: the
        reference's cut at the update boundary, training/routine.py:125-132,153-156), writing
        into caller-owned device tensors (graph-safe).  Envs at step 0 are left alone: their obs
        rows are not written and their ``cut`` byte is 0."""
        check(lib().hwy_cut_episodes(self._handle, ptr(obs), ptr(ep_return), ptr(ep_length),
                                     ptr(cut), stream_ptr()), "hwy_cut_episodes")

    def set_seed_schedule(self, seed_base: int, env_offset: Optional[int] = None,
                          seed_stride: Optional[int] = None) -> None:
        """seed(env e, episode k) = seed_base + env_offset + e + 1 + seed_stride * k."""
        c = self._cfg
        c.seed_base = int(seed_base)
        if env_offset is not None:
            c.env_offset = int(env_offset)
        if seed_stride is not None:
            c.seed_stride = int(seed_stride)
        check(lib().hwy_set_seed_schedule(self._handle, c.seed_base, c.env_offset, c.seed_stride),
              "hwy_set_seed_schedule")
        self.launch_version += 1

    def set_seed_groups(self, seed_bases, envs_per_group: int = 1) -> None:
        """Split the E envs into experiment groups of ``envs_per_group`` consecutive envs, group
        g seeded as a solo handle of that many envs with ``set_seed_schedule(seed_bases[g])``
        would be: seed(env l of group g, episode k) = seed_bases[g] + l + 1 + envs_per_group*k
        (hwy_set_seed_groups; experiments/sweep.py).  ``seed_bases=None`` turns grouping off and
        puts back the seed stride the grouping replaced.  Per-group RankPE tables stay with groups
        of the same geometry; after any other call the handle refuses to run until set_pe_table
        is called again (include/hwy.h)."""
        if seed_bases is None:
            check(lib().hwy_set_seed_groups(self._handle, None, 0, 1), "hwy_set_seed_groups")
            if getattr(self, "_groups", None) is not None:
                # back to the stride the grouping replaced: with envs_per_group left in place the
                # envs of an ungrouped handle would reuse each other's episode seeds
                c = self._cfg
                c.seed_stride = int(self._ungrouped_stride)
                check(lib().hwy_set_seed_schedule(self._handle, c.seed_base, c.env_offset,
                                                  c.seed_stride), "hwy_set_seed_schedule")
            self._groups = None
        else:
            b = np.ascontiguousarray(np.asarray(seed_bases, dtype=np.int64))
            check(lib().hwy_set_seed_groups(self._handle, b.ctypes.data_as(ctypes.c_void_p),
                                            int(b.size), int(envs_per_group)),
                  "hwy_set_seed_groups")
            c = self._cfg
            if getattr(self, "_groups", None) is None:
                self._ungrouped_stride = int(c.seed_stride)
            c.seed_stride = int(envs_per_group)
            check(lib().hwy_set_seed_schedule(self._handle, c.seed_base, c.env_offset,
                                              c.seed_stride), "hwy_set_seed_schedule")
            self._groups = (b.copy(), int(envs_per_group))
        self.launch_version += 1

    def export_state(self) -> torch.Tensor:
        out = torch.empty(NFIELDS, self.num_envs, HWY_MAX_VEHICLES, dtype=torch.int32,
                          device=self.device)
        check(lib().hwy_export_state(self._handle, ptr(out), stream_ptr()), "hwy_export_state")
        return out

    def import_state(self, state: torch.Tensor) -> None:
        if isinstance(state, np.ndarray):
            state = torch.from_numpy(np.ascontiguousarray(state).view(np.int32))
        st = state.to(self.device)
        if st.dtype != torch.int32:
            raise ValueError("state must be int32/uint32 words")
        st = st.contiguous()
        if st.numel() != NFIELDS * self.num_envs * HWY_MAX_VEHICLES:
            raise ValueError("state has the wrong size")
        check(lib().hwy_import_state(self._handle, ptr(st), stream_ptr()), "hwy_import_state")
        self._keep = st

    def render(self, envs=None, *, width: Optional[int] = None, height: Optional[int] = None,
               channels: int = 3, shade: Optional[torch.Tensor] = None,
               out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Frames of the envs' current states as a uint8 device tensor [n, H, W, C] (hwy_render:
        the frame rule of include/hwy.h; one launch, no synchronisation, graph-capturable when
        ``envs`` is None or a device tensor).

        ``envs``: None for all E envs, a device int32 tensor of env ids (read by the kernel; an id
        outside 0..E-1 gives an all-background frame) or a sequence of ids (copied to the device).
        ``width`` / ``height`` default to the config's ``screen_width`` / ``screen_height`` (600,
        150); ``scaling`` and ``centering_position`` come from the config too (5.5, [0.3, 0.5]).
        ``channels``: 3 for RGB, 1 for luma.  ``shade``: a float32 device tensor of E x 64 values
        in vehicle order, tinting each vehicle toward (255, 220, 0).  ``out``: a contiguous uint8
        device tensor of n*H*W*C elements, 16-byte aligned, to write instead of a new one."""
        view = _abi.render_view(self.config)
        a = _abi.RenderArgs()
        a.width = int(view["width"] if width is None else width)
        a.height = int(view["height"] if height is None else height)
        a.channels = int(channels)
        a.scaling = view["scaling"]
        a.centering[0], a.centering[1] = view["centering"]
        ids = None
        if envs is None:
            a.n = self.num_envs
        else:
            ids = envs
            if not isinstance(ids, torch.Tensor):
                ids = torch.as_tensor(np.asarray(ids, dtype=np.int32).reshape(-1),
                                      device=self.device)
            if not (ids.is_cuda and ids.dtype == torch.int32 and ids.is_contiguous()
                    and ids.dim() == 1):
                raise ValueError("envs must be a contiguous 1-D int32 device tensor, a sequence "
                                 f"of env ids or None, got {tuple(ids.shape)} {ids.dtype} on "
                                 f"{ids.device}")
            a.n = int(ids.numel())
            a.env_ids = ptr(ids)
        if shade is not None:
            if not (shade.is_cuda and shade.dtype == torch.float32 and shade.is_contiguous()
                    and shade.numel() == self.num_envs * HWY_MAX_VEHICLES):
                raise ValueError(f"shade must be a contiguous float32 device tensor of "
                                 f"{self.num_envs} x {HWY_MAX_VEHICLES} elements, got "
                                 f"{tuple(shade.shape)} {shade.dtype} on {shade.device}")
            a.shade = ptr(shade)
        shape = (int(a.n), int(a.height), int(a.width), int(a.channels))
        if out is None:
            a.frames = 16  # any aligned address: the size check reads no memory
            nbytes = int(lib().hwy_render_frame_bytes(ctypes.byref(a)))
            check(0 if nbytes >= 0 else -1, "hwy_render")
            out = torch.empty(shape, dtype=torch.uint8, device=self.device)
        elif not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                  and out.numel() == shape[0] * shape[1] * shape[2] * shape[3]):
            raise ValueError(f"out must be a contiguous uint8 device tensor of {shape} elements, "
                             f"got {tuple(out.shape)} {out.dtype} on {out.device}")
        a.frames = ptr(out)
        check(lib().hwy_render(self._handle, ctypes.byref(a), stream_ptr()), "hwy_render")
        self._keep_render = (ids, shade, out)
        return out.view(shape)

    def _launch(self, fn: str, a, *keep) -> None:
        """One launch of entry point ``fn`` (hwy_<what>) with args struct ``a`` on the current
        stream; ``keep``: what ``a`` points into, kept alive on the env as ``_keep_<what>``."""
        check(getattr(lib(), fn)(self._handle, ctypes.byref(a), stream_ptr()), fn)
        setattr(self, "_keep_" + fn[len("hwy_"):], keep)

    def _filled(self, into: Callable, shape: tuple, dtype, out: Optional[torch.Tensor]):
        """``out`` (None: a new ``dtype`` tensor of ``shape``) after ``into(out)`` wrote it, viewed
        as ``shape``: the allocating form of an ``*_into``."""
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=self.device)
        into(out)
        return out.view(shape)

    def observe_into(self, order: Optional[str] = None, *, obs: Optional[torch.Tensor] = None,
                     row_vehicle: Optional[torch.Tensor] = None,
                     row_values: Optional[torch.Tensor] = None,
                     veh_values: Optional[torch.Tensor] = None) -> None:
        """Re-observe the envs' current states into caller-owned device tensors (hwy_observe:
        one launch, no synchronisation, graph-capturable).  ``order``: None for the env's own
        row order -- ``obs`` is then bit for bit what the last step / reset / cut wrote -- or
        "sorted" / "shuffled" to observe the same states under that order instead.
        ``obs`` [E, N, F_out] float32; ``row_vehicle`` [E, N] int32, the vehicle each row shows
        (-1 for an empty row, 0 in row 0); ``row_values`` [E, N] float32 in and ``veh_values``
        [E, 64] float32 out (both or neither), the per-row values scattered to the vehicles in
        ``render``'s ``shade`` layout, 0 for vehicles no row shows."""
        a = observe_args(self.num_envs, self.obs_rows, self.obs_features, self.device, order,
                         obs=obs, row_vehicle=row_vehicle, row_values=row_values,
                         veh_values=veh_values)
        self._launch("hwy_observe", a, obs, row_vehicle, row_values, veh_values)

    def observe(self, order: Optional[str] = None,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The current observation [E, N, F_out] under ``order`` (observe_into's ``obs``)."""
        return self._filled(lambda o: self.observe_into(order, obs=o),
                            (self.num_envs, self.obs_rows, self.obs_features), torch.float32, out)

    def row_vehicles(self, order: Optional[str] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The vehicle index each observation row shows, [E, N] int32 (-1: an empty row)."""
        return self._filled(lambda o: self.observe_into(order, row_vehicle=o),
                            (self.num_envs, self.obs_rows), torch.int32, out)

    def rows_to_vehicles(self, row_values: torch.Tensor, order: Optional[str] = None,
                         out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Per-row values [E, N] scattered to the vehicles the rows show, [E, 64] float32 (0 for
        the others): ready to pass as ``render(shade=...)``."""
        return self._filled(
            lambda o: self.observe_into(order, row_values=row_values, veh_values=o),
            (self.num_envs, HWY_MAX_VEHICLES), torch.float32, out)

    def traffic_into(self, *, restart=(), ttc_thresh: Optional[float] = None,
                     thw_thresh: Optional[float] = None, risk_horizon: Optional[float] = None,
                     near_range: Optional[float] = None, **outputs) -> None:
        """Neighbours, gaps, time-to-collision and headway of the envs' current states into
        caller-owned device tensors (hwy_traffic: one launch, no synchronisation,
        graph-capturable).  ``outputs`` by name, each optional: ``front`` / ``rear`` [E, 64] int32
        (the vehicle in front of / behind each vehicle on its own lane, -1 for none), ``gap``,
        ``closing``, ``ttc``, ``thw``, ``risk`` [E, 64] float32 (``risk`` is ready to pass as
        ``render(shade=...)``), ``ego`` [E, 16] float32 (_abi.EGO_* slots), ``acc`` [E, 8] float32
        in/out (the running per-episode reduction, _abi.TACC_* slots, zero-filled once by the
        caller) and ``ep_stats`` [E, 8] float32 (the finished episodes' rows).  ``restart``: up
        to three [E] uint8 masks, OR-ed, of the envs whose episode ended with the call that
        produced this state (a step's terminated and truncated, cut_episodes' cut).  Call it once
        per state the policy acts on: after reset, after every step, after a cut."""
        a = traffic_args(self.num_envs, self.device, restart=restart, ttc_thresh=ttc_thresh,
                         thw_thresh=thw_thresh, risk_horizon=risk_horizon, near_range=near_range,
                         **outputs)
        self._launch("hwy_traffic", a, outputs, restart)

    def traffic(self, **thresholds) -> Dict[str, torch.Tensor]:
        """The per-vehicle arrays and the ego row of the current states, a dict of fresh device
        tensors (traffic_into's ``front`` .. ``risk`` and ``ego``)."""
        out = alloc_traffic(self.num_envs, self.device)
        del out["acc"], out["ep_stats"]
        self.traffic_into(**thresholds, **out)
        return out

    def sense_into(self, sensor, order: Optional[str] = None, *,
                   obs: Optional[torch.Tensor] = None, row_vehicle: Optional[torch.Tensor] = None,
                   visible: Optional[torch.Tensor] = None, hidden: Optional[torch.Tensor] = None,
                   counts: Optional[torch.Tensor] = None) -> None:
        """Observe the envs' current states through ``sensor`` (a SensorModel or its dict) into
        caller-owned device tensors (hwy_sense: one launch, no synchronisation,
        graph-capturable).  ``order`` as in observe_into.  ``obs`` [E, N, F_out] float32 and
        ``row_vehicle`` [E, N] int32: observe_into's, of the vehicles as the sensor perceives
        them (hidden ones absent, x / y / speed with the sensor's noise); ``visible`` [E, 64]
        uint8; ``hidden`` [E, 64] float32, 1 where a present vehicle is not visible (ready to
        pass as ``render(shade=...)``); ``counts`` [E, 4] int32: present others, out of range,
        blocked, dropped.  With the null sensor ``obs`` and ``row_vehicle`` are observe_into's
        bit for bit."""
        a = sense_args(self.num_envs, self.obs_rows, self.obs_features, self.device, sensor,
                       order, obs=obs, row_vehicle=row_vehicle, visible=visible, hidden=hidden,
                       counts=counts)
        self._launch("hwy_sense", a, obs, row_vehicle, visible, hidden, counts)

    def sense(self, sensor, order: Optional[str] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The current observation [E, N, F_out] through ``sensor`` under ``order`` (sense_into's
        ``obs``)."""
        return self._filled(lambda o: self.sense_into(sensor, order, obs=o),
                            (self.num_envs, self.obs_rows, self.obs_features), torch.float32, out)

    def hidden_vehicles(self, sensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """[E, 64] float32, 1 where a present vehicle is hidden from ``sensor`` (sense_into's
        ``hidden``): ready to pass as ``render(shade=...)``."""
        return self._filled(lambda o: self.sense_into(sensor, hidden=o),
                            (self.num_envs, HWY_MAX_VEHICLES), torch.float32, out)

    def grid_into(self, spec, *, out: Optional[torch.Tensor] = None,
                  cell_vehicle: Optional[torch.Tensor] = None,
                  veh_cell: Optional[torch.Tensor] = None,
                  counts: Optional[torch.Tensor] = None) -> None:
        """The occupancy grid of the envs' current states (``spec``: a GridSpec, its dict, or
        True for the default) into caller-owned device tensors (hwy_grid, include/hwy.h: one
        launch, no synchronisation, graph-capturable).  ``out`` [E, spec.stride(F)] float32: per
        env the layers [C][nx][ny], the ego's own Kinematics row with ``ego_tail``, zero padding;
        ``cell_vehicle`` [E, nx, ny] int32: the vehicle that won each cell, -1 for none;
        ``veh_cell`` [E, 64] int32: each vehicle's flat cell, -1 outside the grid or absent;
        ``counts`` [E, 4] int32: other vehicles present, inside, inside but without their cell,
        outside."""
        a = grid_args(self.num_envs, int(self._cfg.n_features), self.device, spec, out=out,
                      cell_vehicle=cell_vehicle, veh_cell=veh_cell, counts=counts)
        self._launch("hwy_grid", a, out, cell_vehicle, veh_cell, counts)

    def grid(self, spec, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The current occupancy grid [E, spec.stride(F)] (grid_into's ``out``): the observation
        a grid-trained policy acts on."""
        return self.view(_abi.GridSpec.from_dict(spec), out)

    def grid_cells(self, spec) -> torch.Tensor:
        """[E, nx, ny] int32: the vehicle that won each cell of the current grid, -1 for none
        (grid_into's ``cell_vehicle``)."""
        g = _abi.GridSpec.from_dict(spec)
        return self._filled(lambda o: self.grid_into(g, cell_vehicle=o),
                            (self.num_envs, g.nx, g.ny), torch.int32, None)

    def lidar_into(self, spec, *, out: Optional[torch.Tensor] = None,
                   hit_vehicle: Optional[torch.Tensor] = None,
                   seen: Optional[torch.Tensor] = None,
                   counts: Optional[torch.Tensor] = None) -> None:
        """The ray-cast range observation of the envs' current states (``spec``: a LidarSpec, its
        dict, or True for the default) into caller-owned device tensors (hwy_lidar, include/hwy.h:
        one launch, no synchronisation, graph-capturable).  ``out`` [E, spec.stride(F)] float32:
        per env the cells' (distance, relative radial speed) pairs, the ego's own Kinematics row
        with ``ego_tail``, zero padding; ``hit_vehicle`` [E, cells] int32: the vehicle each cell
        returns, -1 for none; ``seen`` [E, 64] float32: 1.0 for the vehicles some undropped cell
        returns (render's ``shade`` layout); ``counts`` [E, 4] int32: other vehicles present,
        of them seen, cells with a return, cells dropped."""
        a = lidar_args(self.num_envs, int(self._cfg.n_features), self.device, spec, out=out,
                       hit_vehicle=hit_vehicle, seen=seen, counts=counts)
        self._launch("hwy_lidar", a, out, hit_vehicle, seen, counts)

    def lidar(self, spec, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The current lidar rows [E, spec.stride(F)] (lidar_into's ``out``): the observation a
        lidar-trained policy acts on."""
        return self.view(_abi.LidarSpec.from_dict(spec), out)

    def lidar_hits(self, spec) -> torch.Tensor:
        """[E, cells] int32: the vehicle each cell of the current lidar returns, -1 for none
        (lidar_into's ``hit_vehicle``)."""
        g = _abi.LidarSpec.from_dict(spec)
        return self._filled(lambda o: self.lidar_into(g, hit_vehicle=o),
                            (self.num_envs, g.cells), torch.int32, None)

    def view_width(self, spec) -> int:
        """Floats per env of what a policy under view ``spec`` (a SensorModel, a GridSpec or a
        LidarSpec) acts on: N * F_out through a sensor, ``spec.stride(F)`` of a grid or a lidar."""
        return _view_rule(spec)[2](self, spec)

    def view_into(self, spec, out: torch.Tensor) -> None:
        """The one launch that writes what a policy under view ``spec`` acts on, of the envs'
        current states, into ``out`` (E x view_width(spec) float32): sense_into's ``obs``,
        grid_into's ``out`` or lidar_into's ``out``."""
        into, keyword, _ = _view_rule(spec)
        getattr(self, into)(spec, **{keyword: out})

    def view(self, spec, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """view_into's rows [E, view_width(spec)], in ``out`` or a new tensor."""
        return self._filled(lambda o: self.view_into(spec, o),
                            (self.num_envs, self.view_width(spec)), torch.float32, out)

    def lookahead_into(self, actions: torch.Tensor, horizon: int, *, hold: bool = False,
                       lazy: bool = False, gamma: float = 1.0, **outputs) -> None:
        """What-if rollouts of the envs' current states into caller-owned device tensors
        (hwy_lookahead, include/hwy.h: no synchronisation, no allocation, graph-capturable; the
        env's own state is not written).  ``actions``: float32 [E, K, H, 2], or [E, K, 2] with
        ``hold`` (each held for all ``horizon`` steps).  Branch (e, k) is what ``horizon``
        autoreset-off steps of a copy of env e give, stopped at the first done step.
        ``outputs`` (any subset, at least one): ``steps`` [E, K] int32, ``terminated`` /
        ``truncated`` [E, K] uint8, ``rewards`` [E, K, H], ``ret`` [E, K] (discounted by
        ``gamma``), ``ego_final`` [E, K, 4], ``obs`` [E, K, N, F_out] float32, and the shield's
        ``chosen`` [E] int32 / ``chosen_action`` [E, 2] float32.  ``lazy``: candidates k >= 1 run
        only for envs whose candidate 0 terminated (the others hold steps 0 and zeros)."""
        unknown = set(outputs) - set(_abi.LOOKAHEAD_OUTPUTS)
        if unknown:
            raise ValueError(f"unknown lookahead outputs {sorted(unknown)}; known: "
                             f"{list(_abi.LOOKAHEAD_OUTPUTS)}")
        a = lookahead_args(self.num_envs, self.obs_rows, self.obs_features, self.device, actions,
                           horizon, hold=hold, lazy=lazy, gamma=gamma, **outputs)
        self._launch("hwy_lookahead", a, actions, outputs)

    def lookahead(self, actions, horizon: Optional[int] = None, gamma: float = 1.0,
                  obs: bool = False) -> Dict[str, torch.Tensor]:
        """What-if rollouts of the current states as a dict of new tensors (lookahead_into's
        outputs but the shield's; ``obs`` only when asked for).  ``actions``: [E, K, H, 2], or
        [E, K, 2] together with ``horizon`` (each action held for that many steps)."""
        a = torch.as_tensor(actions, device=self.device, dtype=torch.float32).contiguous()
        if a.dim() not in (3, 4) or a.shape[0] != self.num_envs:
            raise ValueError(f"actions must be [E, K, H, 2] or [E, K, 2] with E = {self.num_envs}, "
                             f"got {tuple(a.shape)}")
        hold = a.dim() == 3
        if hold and horizon is None:
            raise ValueError("actions [E, K, 2] are held for `horizon` steps: give horizon")
        H = int(a.shape[2]) if not hold else horizon
        if not hold and horizon is not None and int(horizon) != H:
            raise ValueError(f"horizon {horizon} differs from the actions' {H} steps")
        E, K, kw = self.num_envs, int(a.shape[1]), dict(device=self.device)
        out = {"steps": torch.empty(E, K, dtype=torch.int32, **kw),
               "terminated": torch.empty(E, K, dtype=torch.uint8, **kw),
               "truncated": torch.empty(E, K, dtype=torch.uint8, **kw),
               "rewards": torch.empty(E, K, max(int(H), 1), dtype=torch.float32, **kw),
               "ret": torch.empty(E, K, dtype=torch.float32, **kw),
               "ego_final": torch.empty(E, K, 4, dtype=torch.float32, **kw)}
        if obs:
            out["obs"] = torch.empty(E, K, self.obs_rows, self.obs_features, dtype=torch.float32,
                                     **kw)
        self.lookahead_into(a, H, hold=hold, gamma=gamma, **out)
        return out

    def shield_into(self, shield, actions: torch.Tensor, out_actions: torch.Tensor, *,
                    chosen: Optional[torch.Tensor] = None,
                    scratch: Optional[Dict[str, torch.Tensor]] = None) -> None:
        """The action the env should execute instead of ``actions`` [E, 2] under ``shield`` (a
        hwy.Shield or its dict), into ``out_actions`` [E, 2]: one copy into the preallocated
        candidate tensor and one hwy_lookahead call (hold mode, chosen / chosen_action), no
        synchronisation, graph-capturable.  Candidate 0 is the given action, the rest the
        shield's fallbacks, each held for the shield's horizon.  ``chosen`` [E] int32 receives
        the candidate picked (0: the policy's action stands).  ``scratch``: caller-owned
        ``cand`` [E, K, 2] float32, ``steps`` [E, K] int32, ``terminated`` [E, K] uint8 and
        ``chosen`` [E] int32 (default: the env's own, allocated once per shield)."""
        sh = _abi.Shield.from_dict(shield)
        E, K = self.num_envs, sh.k
        if not (isinstance(actions, torch.Tensor) and actions.dtype == torch.float32
                and actions.numel() == 2 * E and actions.device == self.device):
            raise ValueError(f"actions must be a float32 tensor of {E} x 2 elements on "
                             f"{self.device}")
        sc = scratch if scratch is not None else self._shield_scratch(sh)
        cand = sc["cand"]
        cand[:, 0, :].copy_(actions.view(E, 2))
        if chosen is None:
            chosen = sc["chosen"]
        self.lookahead_into(cand, sh.horizon, hold=True, lazy=sh.lazy, steps=sc["steps"],
                            terminated=sc["terminated"], chosen=chosen,
                            chosen_action=out_actions)

    def _shield_scratch(self, sh) -> Dict[str, torch.Tensor]:
        """The env's own candidate tensor (fallbacks filled in) and steps / terminated / chosen
        scratch for ``sh``, allocated on first use."""
        cache = self.__dict__.setdefault("_shield_cache", {})
        sc = cache.get(sh)
        if sc is None:
            E, K, kw = self.num_envs, sh.k, dict(device=self.device)
            cand = torch.zeros(E, K, 2, dtype=torch.float32, **kw)
            cand[:, 1:, :] = torch.tensor(sh.fallbacks, dtype=torch.float32, **kw)
            sc = cache[sh] = {"cand": cand,
                              "steps": torch.zeros(E, K, dtype=torch.int32, **kw),
                              "terminated": torch.zeros(E, K, dtype=torch.uint8, **kw),
                              "chosen": torch.zeros(E, dtype=torch.int32, **kw)}
        return sc

    def close(self) -> None:
        if self._handle:
            lib().hwy_destroy(self._handle)
            self._handle = ctypes.c_void_p()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    @property
    def unwrapped(self):
        return self


def _row_stride(env, spec) -> int:
    return spec.stride(int(env.hwy_config.n_features))


# The views: per record class, the ``*_into`` that writes what the policy acts on, the keyword it
# takes that buffer by, and the floats per env.  A new observation kind adds its line here.
_VIEWS = {
    _abi.SensorModel: ("sense_into", "obs", lambda env, spec: env.obs_rows * env.obs_features),
    _abi.GridSpec: ("grid_into", "out", _row_stride),
    _abi.LidarSpec: ("lidar_into", "out", _row_stride),
}
VIEW_RECORDS = {cls.NOUN: cls for cls in _VIEWS}  # by option name (ppo/options.py's views)


def _view_rule(spec) -> tuple:
    try:
        return _VIEWS[type(spec)]
    except KeyError:
        raise ValueError(f"a view is one of {[c.__name__ for c in _VIEWS]}, got {spec!r}") from None


def _info_array(iptrs, n: int):
    """hwy_step_info[n] from _info_ptrs' tuples (None: the caller wants no info)."""
    return None if iptrs is None else (HwyStepInfo * n)(*[HwyStepInfo(*p) for p in iptrs])


class _GroupVariant(NamedTuple):
    """One variant of the grouped step: its entry points, the size function of its second device
    table (None: it has none) and its prepare's arrays between ``io`` and ``n``."""
    prepare: str
    launch: str
    table_bytes: Optional[str]
    arrays: Callable


_GROUP_VARIANTS = {
    "plain": _GroupVariant("hwy_step_group_prepare", "hwy_step_group", None,
                           lambda iptrs, fptrs, n: ()),
    "info": _GroupVariant("hwy_step_group_info_prepare", "hwy_step_group_info",
                          "hwy_step_group_info_table_bytes",
                          lambda iptrs, fptrs, n: (_info_array(iptrs, n),)),
    "final": _GroupVariant("hwy_step_group_final_prepare", "hwy_step_group_final",
                           "hwy_step_group_final_table_bytes",
                           lambda iptrs, fptrs, n: (_info_array(iptrs, n),
                                                    (ctypes.c_void_p * n)(*fptrs))),
}


class GroupEnvStep:
    """HighwayVecEnv.step_into for several handles in ONE launch (hwy_step_group): the cells of a
    sweep batch (ppo/group.py GroupBatch), whose handles differ in observation width and fused
    wrapper.  Each env computes exactly what its own handle's step computes.  The launch
    parameters live in device tables per (variant, handle configurations, buffers) key, prepared on
    first use -- outside any graph capture, as GroupBatch's eager first rollout at a key does --
    so the launch itself is graph-capturable.  The variants (plain, info, final) differ only in
    their _GROUP_VARIANTS record."""

    def __init__(self, envs):
        self.envs = [e.unwrapped if hasattr(e, "unwrapped") else e for e in envs]
        self.n = len(self.envs)
        if self.n < 1:
            raise ValueError("GroupEnvStep needs at least one env")
        self._nb = int(lib().hwy_step_group_table_bytes(self.n))
        self._tables: Dict[Any, Any] = {}

    def launch(self, ios, infos=None, final_obs=None) -> None:
        """ios[i] = (actions, obs, reward, terminated, truncated, ep_return, ep_length) of env i,
        as step_into takes them (the last two may be None).  ``infos[i]``: env i's step info
        tensors as step_into's ``info`` (one dict per handle; the launch is then the info
        variant, hwy_step_group_info).  ``final_obs[i]``: env i's terminal-observation buffer as
        step_into's ``final_obs`` (the launch is then the final variant, hwy_step_group_final,
        with the info outputs too when ``infos`` is given)."""
        ptrs = tuple(tuple(ptr(x) for x in io) for io in ios)
        iptrs = fptrs = None
        if final_obs is not None:
            if len(final_obs) != self.n or (infos is not None and len(infos) != self.n):
                raise ValueError("one final_obs buffer (and one step info dict) per handle")
            for e, f in zip(self.envs, final_obs):
                _check_final_obs(e, f)
            fptrs = tuple(ptr(f) for f in final_obs)
        elif infos is not None and len(infos) != self.n:
            raise ValueError("one step info dict per handle")
        if infos is not None:
            iptrs = tuple(_info_ptrs(i) for i in infos)
        name = "final" if fptrs is not None else "plain" if iptrs is None else "info"
        v = _GROUP_VARIANTS[name]
        key = (name, tuple((e._handle.value, e.launch_version) for e in self.envs), ptrs, iptrs,
               fptrs)
        hit = self._tables.get(key)
        if hit is None:
            hit = self._tables[key] = self._prepare(v, ptrs, iptrs, fptrs)
        check(hit[0](*hit[1], stream_ptr()), v.launch)

    def _prepare(self, v, ptrs, iptrs, fptrs) -> tuple:
        """A cache entry: variant ``v``'s device tables filled for these buffers, as (the launch
        entry point, its arguments before the stream, what they point into)."""
        n, dev = self.n, self.envs[0].device
        hs = (ctypes.c_void_p * n)(*[e._handle.value for e in self.envs])
        arr = (HwyStepIO * n)(*[HwyStepIO(*p) for p in ptrs])
        tables = [torch.empty(self._nb, dtype=torch.uint8, device=dev)]
        if v.table_bytes is not None:
            tables.append(torch.empty(int(getattr(lib(), v.table_bytes)(n)), dtype=torch.uint8,
                                      device=dev))
        plan = HwyStepGroupPlan()
        tptrs = tuple(t.data_ptr() for t in tables)
        check(getattr(lib(), v.prepare)(hs, arr, *v.arrays(iptrs, fptrs, n), n, *tptrs,
                                        ctypes.byref(plan), stream_ptr()), v.prepare)
        return getattr(lib(), v.launch), (ctypes.byref(plan),) + tptrs, (plan, tables)
