"""Lockstep rollout of T policy steps over E device envs (the collection half of
training/routine.py:121-160, batched), optionally replayed as one HIP graph.

Per step t: ActorCritic.act on buf.states[t] with the rollout's pre-drawn noise (one hwy_ppo_act
launch writing the action / pre-tanh / log-prob / value rows), then hwy_step writing the next
observation, reward, flags and episode statistics straight into buf's row t (+1).  The 2T
launches have fixed arguments between updates, so from the second rollout on they are captured
once and replayed as a single graph: no host work per step and ~1 us instead of ~6 us between
dependent launches.  The graph is re-captured whenever something it baked in changes: the env
handle or its launch configuration (seed schedule, fused PE table), the acting weights (the
update's tile image or the flat parameters), or the buffers.

``episode_schedule="reference"`` adds the reference's cut at the update boundary
(training/routine.py:125-132,153-156): after the T steps every running episode is ended and the
schedule's next one started (hwy_cut_episodes), the new first observations going to ``next0``
-- a buffer of its own, since states[0..T] are the update's inputs -- with the cut episodes'
partial returns in ``cut_return``.  The cut step's ``dones`` stays 0, so GAE bootstraps it with
V(states[T]).  The next rollout starts from ``next0`` (``start_next``).  A reference rollout of
T > REFERENCE_GRAPH_CHUNK steps is issued as fixed chunk graphs of that many steps (the buffers
are static, so each chunk replays) instead of one graph of 2T launches.

``truncation="bootstrap"`` (default ``"terminal"``: a time limit is booked as terminal, as the
reference does, training/routine.py:135): step t runs the final variant of the env step, which
also writes the terminal observations of the envs that finished to ``buf.final_obs``, and then
``agent.value_masked`` stores V(final observation) of the truncated, not terminated rows in
``buf.boot_values[t]`` (0 elsewhere) with the weights that produced ``values[t]``.  Both launches
are part of the captured graph; PPOAgent.update_rollout then runs hwy_gae_boot.

``safety_stats=True``: one hwy_traffic launch after the reset that precedes the first rollout and
one after every env step, inside the captured graph, with that step's terminated / truncated as
restart masks: ``buf.traffic_acc`` carries the running per-episode reduction of the ego's
time-to-collision, headway, gap and distance, ``buf.traffic_stats[t]`` receives the rows of the
episodes that finished in step t (``traffic_after_reset`` / ``traffic_after_step``).  On the
reference schedule the launch of the last step waits for the cut and takes its ``cut`` as a
third mask, so the state the cut throws away is not measured, the cut episodes' rows land in
``traffic_stats[T - 1]`` beside the finished ones' (no env is both), and an env that had just
restarted is not counted twice.

``sensor=`` / ``grid=`` / ``lidar=`` (a hwy.SensorModel, GridSpec or LidarSpec, its dict, or True
for the default grid or lidar; at most one): the view the policy acts through.  One
``env.view_into`` launch (hwy_sense, hwy_grid or hwy_lidar) after every env step, inside the
captured graph, writes ``buf.states[t + 1]`` from the state the step left, and one on the reset
states the caller left writes ``buf.states[0]``; the env step itself is unchanged.  A sensor
overwrites the rows the step wrote there; a grid or a lidar replaces them: the step writes its
Kinematics rows into the env's own observation buffer and ``buf.states`` is ``spec.stride(F)``
wide.

``shield=`` (a hwy.Shield or its dict): the shield is part of the environment.  After the policy
acted, one hwy_lookahead call (``env.shield_into``) inside the captured graph rolls the policy's
action and the shield's fallbacks out from the env's state and writes the action the env executes
to ``buf.exec_actions[t]`` and the candidate picked to ``buf.chosen[t]``; the env step takes
``exec_actions[t]``.  ``buf.actions``, ``pre_tanh``, ``log_probs`` and ``values`` stay the
policy's own, so PPO's stored data is untouched.

Which of these options exclude each other, and why, is ppo/options.py's table.
"""

from __future__ import annotations

from typing import Optional

import torch

from utils.graphs import run_or_replay, run_or_replay_chunks

from . import options
from .options import EPISODE_SCHEDULES, TRUNCATIONS  # noqa: F401  (this module's names too)

# steps per captured graph of a reference-schedule rollout (2 launches per step)
REFERENCE_GRAPH_CHUNK = 256

check_episode_schedule = options.BY_NAME["episode_schedule"].normalise
check_truncation = options.BY_NAME["truncation"].normalise


def check_sensor(sensor, truncation: str = "terminal", episode_schedule: str = "lockstep"):
    """``sensor`` as a hwy.SensorModel (None: none), refusing what a sensed rollout does not do."""
    return options.checked("sensor", sensor, truncation=truncation,
                           episode_schedule=episode_schedule)


def check_shield(shield, truncation: str = "terminal", episode_schedule: str = "lockstep",
                 sensor=None):
    """``shield`` as a hwy.Shield (None: none), refusing what a shielded rollout does not do."""
    return options.checked("shield", shield, truncation=truncation,
                           episode_schedule=episode_schedule, sensor=sensor)


def check_grid(grid, truncation: str = "terminal", episode_schedule: str = "lockstep", sensor=None,
               shield=None):
    """``grid`` as a hwy.GridSpec (None: none), refusing what a grid rollout does not do."""
    return options.checked("grid", grid, truncation=truncation, episode_schedule=episode_schedule,
                           sensor=sensor, shield=shield)


def check_lidar(lidar, truncation: str = "terminal", episode_schedule: str = "lockstep",
                sensor=None, shield=None, grid=None):
    """``lidar`` as a hwy.LidarSpec (None: none), refusing what a lidar rollout does not do."""
    return options.checked("lidar", lidar, truncation=truncation,
                           episode_schedule=episode_schedule, sensor=sensor, shield=shield,
                           grid=grid)


def rollout_chunks(T: int, episode_schedule: str):
    """The (t0, t1) step ranges a rollout of T steps is issued (and captured) in: the whole
    rollout, or, for a long reference-schedule rollout, chunks of REFERENCE_GRAPH_CHUNK steps."""
    if episode_schedule != "reference" or T <= REFERENCE_GRAPH_CHUNK:
        return [(0, T)]
    return [(t0, min(T, t0 + REFERENCE_GRAPH_CHUNK)) for t0 in range(0, T, REFERENCE_GRAPH_CHUNK)]


def alloc_cut_buffers(owner, E: int, sd: int, device) -> None:
    """The fixed buffers of the reference schedule's cut on `owner` (a rollout or a group)."""
    owner.next0 = torch.zeros(E, sd, dtype=torch.float32, device=device)
    owner.cut_return = torch.zeros(E, dtype=torch.float32, device=device)
    owner.cut_length = torch.zeros(E, dtype=torch.int32, device=device)
    owner.cut = torch.zeros(E, dtype=torch.uint8, device=device)


def traffic_after_reset(env, buf) -> None:
    """hwy_traffic on the reset states: the zero-filled running reduction starts from them."""
    env.traffic_into(acc=buf.traffic_acc)


def traffic_after_step(env, buf, t: int, cut=None) -> None:
    """hwy_traffic on the states rollout step t left (``cut``: and the cut after it), the
    finished episodes' rows going to buf.traffic_stats[t]."""
    masks = (buf.terminated[t], buf.truncated[t]) + (() if cut is None else (cut,))
    env.traffic_into(acc=buf.traffic_acc, ep_stats=buf.traffic_stats[t], restart=masks)


class LockstepRollout:
    def __init__(self, agent, env, buf, use_graph: bool = True,
                 episode_schedule: str = "lockstep", episode_stats: bool = False,
                 truncation: str = "terminal", safety_stats: bool = False, sensor=None,
                 shield=None, grid=None, lidar=None):
        self.agent = agent
        self.env = env.unwrapped if hasattr(env, "unwrapped") else env
        self.buf = buf
        self.sensor = check_sensor(sensor, truncation, episode_schedule)
        # one hwy_lookahead call per env step, between acting and stepping
        self.shield = check_shield(shield, truncation, episode_schedule, sensor)
        self.grid = check_grid(grid, truncation, episode_schedule, sensor, shield)
        self.lidar = check_lidar(lidar, truncation, episode_schedule, sensor, shield, grid)
        # the view, whichever of the three is given: one env.view_into launch per env step (and
        # one now, on the reset states the caller left) writes what the policy acts on
        given = options.given_view(dict(sensor=self.sensor, grid=self.grid, lidar=self.lidar))
        self.view = None if given is None else given[1]
        # it replaces the step's rows, which then stay in the env's own buffer (a grid, a lidar),
        # or overwrites them where the step wrote them (a sensor)
        self.view_replaces = self.view is not None and self.view.REPLACES_ROWS
        if self.view_replaces:
            name, spec = given
            if not hasattr(self.env, "view_width"):
                raise ValueError(f"{name} needs a vector env (HighwayVecEnv)")
            width = self.env.view_width(spec)
            if buf.states.shape[-1] != width:
                raise ValueError(f"{name} needs a RolloutBuffer of state width {width} "
                                 f"({type(spec).__name__}.stride), got {buf.states.shape[-1]}")
        if self.shield is not None:
            if not hasattr(self.env, "shield_into"):
                raise ValueError("shield needs a vector env (HighwayVecEnv)")
            if getattr(buf, "exec_actions", None) is None:
                raise ValueError("shield needs a RolloutBuffer built with shield=True")
            self.env._shield_scratch(self.shield)  # allocated here, not inside a capture
        # the steps as hwy_step_with_info, the episodes' sums going to buf.ep_stats / buf.acc
        # (after a reference-schedule cut, buf.acc's rows of the cut envs hold their partial sums)
        self.episode_stats = bool(episode_stats)
        if self.episode_stats and buf.ep_stats is None:
            raise ValueError("episode_stats needs a RolloutBuffer built with episode_stats=True")
        # one hwy_traffic launch per env step (and one now, on the reset states the caller left)
        self.safety_stats = bool(safety_stats)
        if self.safety_stats and getattr(buf, "traffic_stats", None) is None:
            raise ValueError("safety_stats needs a RolloutBuffer built with safety_stats=True")
        self.truncation = check_truncation(truncation)
        if self.truncation == "bootstrap" and getattr(buf, "boot_values", None) is None:
            raise ValueError('truncation="bootstrap" needs a RolloutBuffer built with '
                             "truncation_bootstrap=True")
        self.use_graph = bool(use_graph) and self.buf.states.is_cuda
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._key = None
        self._seen = None  # key of the last eager run (capture once a key repeats)
        # the env step through a launch-parameter table (hwy_step_group with one handle): the
        # kernel reads the handle's configuration from device memory instead of its kernel
        # arguments, which spares its scalar registers (SGPR spills 114 -> 9) and runs ~4 %
        # faster per step, with the same results (tools/probe_step_group1.py)
        from hwy.vec_env import GroupEnvStep

        self._envstep = GroupEnvStep([self.env]) if hasattr(self.env, "_handle") else None
        self.episode_schedule = check_episode_schedule(episode_schedule)
        self._chunks = None  # reference schedule, long rollout: (graph, key, seen) per chunk
        # how the rollouts were issued (utils/graphs.py run_or_replay)
        self.stats = {"rollout_replay": 0, "rollout_eager": 0, "rollout_capture": 0}
        if self.episode_schedule == "reference":
            alloc_cut_buffers(self, buf.E, buf.states.shape[-1], buf.states.device)
        if self.safety_stats:
            traffic_after_reset(self.env, buf)
        if self.view is not None:
            self.env.view_into(self.view, buf.states[0])

    def _launch_key(self):
        from hwy.ppo_native import act_tiles, flat_params

        ag, env, buf = self.agent, self.env, self.buf
        flat = flat_params(ag)[0] if ag.backend != "torch" else None
        tiles = None
        if flat is not None and ag._act_fused_ok(buf.states[0]):
            # the image acting streams, brought in step with the parameters here, outside any
            # capture (as ExperimentGroup.rollout's act.tiles()): a replayed graph reads the
            # image's memory, so a write that retired an acting-only image (H = 256 before the
            # first fused update, where no address in this key moves) must be applied before it
            sd = ag.actor_critic.shared[0].weight
            tiles = act_tiles(ag, flat, sd.shape[1], sd.shape[0])
        params = tuple(p.data_ptr() for p in ag.actor_critic.parameters())
        key = (env._handle.value, getattr(env, "launch_version", 0), tiles, params,
               buf.states.data_ptr(), buf.noise.data_ptr(), buf.T, buf.E)
        if self.truncation == "bootstrap":
            key += (buf.final_obs.data_ptr(), buf.boot_values.data_ptr())
        if self.safety_stats:
            key += (buf.traffic_stats.data_ptr(), buf.traffic_acc.data_ptr())
        if self.view is not None:
            key += (self.view, env.obs_buf.data_ptr()) if self.view_replaces else (self.view,)
        if self.shield is not None:
            key += (self.shield, buf.exec_actions.data_ptr(), buf.chosen.data_ptr())
        return key

    def _steps(self, t0: int = 0, t1: Optional[int] = None) -> None:
        ag, env, buf = self.agent, self.env, self.buf
        E = buf.E
        obs_shape = env.obs_buf.shape[1:]
        t1 = buf.T if t1 is None else t1
        for t in range(t0, t1):
            ag.select_action(buf.states[t], out=(buf.actions[t], buf.pre_tanh[t],
                                                 buf.log_probs[t], buf.values[t]),
                             noise=buf.noise[t])
            executed = buf.actions[t]
            if self.shield is not None:
                executed = buf.exec_actions[t]
                env.shield_into(self.shield, buf.actions[t], executed, chosen=buf.chosen[t])
            # under a view that replaces them the step's rows stay in the env's own buffer
            next_obs = (env.obs_buf if self.view_replaces
                        else buf.states[t + 1].view(E, *obs_shape))
            io = (executed, next_obs, buf.rewards[t],
                  buf.terminated[t], buf.truncated[t], buf.ep_return[t], buf.ep_length[t])
            boot = self.truncation == "bootstrap"
            info = buf.step_info(t) if self.episode_stats else None
            final_obs = buf.final_obs if boot else None
            if self._envstep is not None:
                self._envstep.launch([io], infos=None if info is None else [info],
                                     final_obs=None if final_obs is None else [final_obs])
            else:
                env.step_into(*io, info=info, final_obs=final_obs)
            if boot:
                ag.value_masked(buf.final_obs, buf.truncated[t], buf.terminated[t],
                                out=buf.boot_values[t])
            if self.view is not None:
                env.view_into(self.view, buf.states[t + 1])
            if self.safety_stats and not (self.episode_schedule == "reference" and t == buf.T - 1):
                traffic_after_step(env, buf, t)
        if t1 < buf.T:
            return
        buf.finish_dones()
        if self.episode_schedule == "reference":
            self.next0.copy_(buf.states[buf.T])
            env.cut_episodes(self.next0.view(E, *obs_shape), self.cut_return, self.cut_length,
                             self.cut)
            if self.safety_stats:
                traffic_after_step(env, buf, buf.T - 1, cut=self.cut)

    def start_next(self) -> None:
        """states[0] of the next rollout: the last observation, or, on the reference schedule,
        the first observations after the cut."""
        buf = self.buf
        buf.states[0].copy_(self.next0 if self.episode_schedule == "reference"
                            else buf.states[buf.T])

    def run(self) -> None:
        """One rollout into buf (rows 0..T-1, states[1..T]); buf.states[0] holds the first obs."""
        self.buf.draw_noise(self.agent.generator)
        if not self.use_graph:
            self._steps()
            return
        key = self._launch_key()
        chunks = rollout_chunks(self.buf.T, self.episode_schedule)
        if len(chunks) > 1:  # a long reference rollout: one graph per chunk
            self._chunks = run_or_replay_chunks(self, True, key, chunks, self._steps, self._chunks)
            return
        self._graph, self._key, self._seen = run_or_replay(
            self, True, key, self._steps, self._graph, self._key, self._seen, "rollout")
