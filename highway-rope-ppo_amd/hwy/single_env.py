"""HighwayEnv: the one-env, numpy-in/numpy-out facade of HighwayVecEnv.

This is what ``make_env`` returns when no ``num_envs`` override is given, so the reference's
own training loop (training/routine.py:121-151: per-episode ``env.reset(seed=...)``, numpy
``flat_state``, Python-float rewards) runs unchanged on the MI355X env.  Each call still executes
the HIP step kernel (E = 1) and synchronises once to hand numpy arrays back; use HighwayVecEnv
(``env_overrides={"num_envs": E}``) for throughput.
"""

from __future__ import annotations

from typing import Any, Dict, Optional

import numpy as np
import torch

from ._abi import REWARD_KEYS, GridSpec, LidarSpec, SensorModel
from .gym import Env, spaces
from .vec_env import HighwayVecEnv


class HighwayEnv(Env):
    """gymnasium-style single highway-v0 env backed by libhwy.so."""

    metadata = {"render_modes": ["rgb_array"]}

    def __init__(self, config: Dict[str, Any], device: Optional[torch.device] = None,
                 info: bool = False, render_mode: Optional[str] = None):
        if render_mode is not None and render_mode not in self.metadata["render_modes"]:
            # "human" included: there is no display to draw on
            raise ValueError(f"render_mode {render_mode!r} is not supported; supported: "
                             f"{self.metadata['render_modes']} (or None)")
        self.render_mode = render_mode
        self._vec = HighwayVecEnv(config, num_envs=1, device=device, autoreset=False, info=info)
        self._info = bool(info)
        self.config = self._vec.config
        self.action_space = spaces.Box(-1.0, 1.0, shape=(2,), dtype=np.float32)
        self.observation_space = self._vec.single_observation_space
        self._episode = 0
        self._seed_base = 0
        self._act = torch.zeros(1, 2, dtype=torch.float32, device=self._vec.device)
        self._seed_t = torch.zeros(1, dtype=torch.int64, device=self._vec.device)

    @property
    def device(self) -> torch.device:
        return self._vec.device

    @property
    def vec_env(self) -> HighwayVecEnv:
        return self._vec

    @property
    def max_episode_steps(self) -> int:
        return self._vec.max_episode_steps

    def enable_pe(self, kind, d, table, ego_idx=0, max_dist=100.0):
        self._vec.enable_pe(kind, d, table, ego_idx=ego_idx, max_dist=max_dist)
        self.observation_space = self._vec.single_observation_space

    def set_pe_table(self, table):
        self._vec.set_pe_table(table)

    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None):
        """``seed`` seeds this episode's traffic (gymnasium reset(seed=...) semantics)."""
        if seed is None:
            # gymnasium continues the env's RNG stream; here: next seed of the schedule
            self._episode += 1
            seed = self._seed_base + self._episode
        else:
            self._seed_base, self._episode = int(seed), 0
        self._seed_t.fill_(int(seed))
        obs, _ = self._vec.reset(seeds=self._seed_t)
        return obs[0].cpu().numpy(), {}

    def step(self, action):
        a = torch.as_tensor(np.asarray(action, dtype=np.float32).reshape(1, 2))
        self._act.copy_(a, non_blocking=False)
        obs, rew, term, trunc, _ = self._vec.step(self._act)
        parts = [rew.view(1), term.view(1).float(), trunc.view(1).float()]
        if self._info:  # upstream's AbstractEnv._info, in the same single transfer
            b = self._vec.info_buf
            parts += [b["speed"].view(1), b["crashed"].view(1).float(), b["rewards"].view(4)]
        host = torch.cat(parts).cpu().numpy()
        info = {}
        if self._info:
            info = {"speed": float(host[3]), "crashed": bool(host[4] > 0),
                    "action": np.asarray(action, dtype=np.float32).reshape(2).copy(),
                    "rewards": {k: float(host[5 + i]) for i, k in enumerate(REWARD_KEYS)}}
        return (obs[0].cpu().numpy(), float(host[0]), bool(host[1] > 0), bool(host[2] > 0), info)

    def render(self):
        """The current frame as an H x W x 3 uint8 numpy array with render_mode="rgb_array"
        (HighwayVecEnv.render: the frame rule of include/hwy.h at the config's view), None
        without a render mode, as gymnasium's envs do."""
        if self.render_mode is None:
            return None
        return self._vec.render()[0].cpu().numpy()

    def row_vehicles(self):
        """The vehicle index each row of the current observation shows, an [N] int32 numpy array
        (HighwayVecEnv.row_vehicles: 0 in row 0, -1 for an empty row)."""
        return self._vec.row_vehicles()[0].cpu().numpy()

    def traffic(self, **thresholds):
        """Gaps, time-to-collision and headway of the current state (HighwayVecEnv.traffic) as
        numpy: ``ego`` [16] float32 (hwy._abi.EGO_* slots) and the per-vehicle ``front``, ``rear``
        [64] int32 and ``gap``, ``closing``, ``ttc``, ``thw``, ``risk`` [64] float32."""
        return {k: t[0].cpu().numpy() for k, t in self._vec.traffic(**thresholds).items()}

    def view(self, spec):
        """What a policy under view ``spec`` (a hwy.SensorModel, GridSpec or LidarSpec) acts on at
        the current state (HighwayVecEnv.view), a float32 vector of view_width(spec)."""
        return self._vec.view(spec)[0].cpu().numpy()

    def sense(self, sensor):
        """view() through ``sensor`` (a hwy.SensorModel or its dict) as [N, F_out] rows."""
        return self.view(SensorModel.from_dict(sensor)).reshape(self.observation_space.shape)

    def grid(self, spec):
        """view() of the occupancy grid ``spec`` (a hwy.GridSpec, its dict, or True)."""
        return self.view(GridSpec.from_dict(spec))

    def lidar(self, spec):
        """view() of the lidar ``spec`` (a hwy.LidarSpec, its dict, or True)."""
        return self.view(LidarSpec.from_dict(spec))

    def lookahead(self, actions, gamma: float = 1.0, obs: bool = False):
        """What-if rollouts from the current state (HighwayVecEnv.lookahead): ``actions`` is a
        [K, H, 2] array of K action sequences; returns a dict of numpy arrays, ``steps``,
        ``terminated``, ``truncated``, ``ret`` [K], ``rewards`` [K, H], ``ego_final`` [K, 4] and,
        with ``obs``, ``obs`` [K, N, F_out].  The env itself does not move."""
        a = np.asarray(actions, dtype=np.float32)
        if a.ndim != 3 or a.shape[2] != 2:
            raise ValueError(f"actions must be [K, H, 2], got {a.shape}")
        out = self._vec.lookahead(a[None], gamma=gamma, obs=obs)
        return {k: t[0].cpu().numpy() for k, t in out.items()}

    def close(self):
        self._vec.close()
