"""ExperimentRunner (reference experiments/runner.py:19-155) on the MI355X env.

Same launch sequence and status dict: acquire device -> seed -> logger -> make_env ->
``env.to(device)`` when the wrapper has it -> state/action dims -> PPOAgent ->
train_with_experiment_name -> {"status": "COMPLETED"|"FAILED", ...}.  Experiment.extra may carry
``num_envs`` (lockstep envs, > 1 selects the vectorised loop), ``num_minibatches`` and
``episode_schedule`` ("lockstep", the default, or "reference": episodes cut at the update
boundary and evaluations ahead of the update, training/routine.py; with it ``num_envs`` 1 runs
the vectorised loop on a one-env HighwayVecEnv, which is the reference's own episode stream)
and ``episode_stats`` (True: per-episode lengths, crashes, mean speeds and lane changes in the
metrics and a crash rate in the summary, training/routine.py; vectorised loop only) and
``safety_stats`` (True: one hwy_traffic launch per env step books every episode's least
time-to-collision, headway, gap and distance and its shares of critical and tailgating states in
the metrics, and a near-miss rate in the summary, training/routine.py; vectorised loop only, not
over a process group; training, rewards and weights are bit for bit those without it) and
``truncation`` ("terminal", the default and the reference's behaviour, or "bootstrap": GAE takes
V(final observation) at a time limit, ppo/rollout.py; launch() on the vectorised loop only --
a process group, launch_group and launch_batch refuse it) and ``attribution`` (True: after
training, training/routine.py's attribution() at the final weights on the evaluations' seeds goes
into the metrics JSON as ``attribution`` -- mean |input gradient| of acceleration, steering and
value per observed row, per distance rank and per feature column, with the share on the embedding
columns and on the ego row; training, rewards and weights are bit for bit those without it;
launch() on the vectorised loop only -- launch_group and launch_batch refuse it) and
``eval_orders`` (a list of "sorted" / "shuffled": after training, evaluate(num_episodes=10,
order=name) at the final weights goes into the metrics JSON as ``order_rewards[name]`` -- the
evaluation's episodes with the policy acting on the same worlds observed under that row order,
whatever order it trained on; it draws no random number, so everything else is bit for bit the
run without it; launch() on the vectorised loop only, refused by the grouped launches likewise)
and ``eval_sensors`` ({name: sensor dict}, hwy.SensorModel's fields ``los``, ``range``,
``dropout``, ``noise``, ``salt``: after training, evaluate(num_episodes=10, sensor=...) at the
final weights goes into the metrics JSON as ``sensor_rewards[name]`` -- the policy acting on what
that sensor perceives; the training is likewise unchanged, and the grouped launches refuse it) and
``sensor`` (one such dict: the run *trains* under it -- every state the policy acts on is sensed,
its own evaluations use the same sensor, the metrics carry it as ``sensor``; launch() on the
vectorised loop only, not over a process group, not with truncation "bootstrap" or the reference
schedule, refused by the grouped launches) and ``shield`` / ``eval_shields`` (a hwy.Shield's
dict, fields ``horizon``, ``fallbacks``, ``lazy``, and {name: such a dict or None}: the run trains
with the action shield inside its rollout, ``shield_rate`` per update and ``shield`` in the
metrics, and evaluate(num_episodes=10, shield=...) at the final weights goes in as
``shield_rewards[name]``; the same restrictions as ``sensor``, and not together with it) and
``grid`` (a hwy.GridSpec, its dict, or True for the default: the run trains on an occupancy grid of
the env states instead of the Kinematics rows -- hwy_grid inside the rollout, ``state_dim`` the
spec's stride, the run's own evaluations on the same grid, ``grid`` in the metrics; launch() on the
vectorised loop only, not over a process group, not with ``sensor``, ``shield``, truncation
"bootstrap" or the reference schedule, refused by the grouped launches).

Launched under torchrun (WORLD_SIZE > 1) one experiment spans the ranks, one GPU each: the
runner joins the process group (RCCL, or ``HWY_DIST_BACKEND``), gives rank r the envs
r*num_envs.. of world*num_envs on the shared seed schedule and hands the group to PPOAgent
(weights broadcast from rank 0, gradients and advantage statistics all-reduced).  Rank 0 logs,
evaluates and writes the artifacts; the other ranks' results carry ``rank``.  The reference
instead runs one single-GPU process per experiment and oversubscribes the GPUs
(SURVEY.md §8(f)).
"""

from __future__ import annotations

import logging
import time
import traceback
from typing import Any, Dict

import numpy as np
import torch

from hwy.gym import spaces
from ppo.agent import PPOAgent
from training.routine import train_with_experiment_name
from utils.logging_utils import setup_experiment_logger
from utils.reproducibility import set_random_seeds

from .config import Experiment
from .wrappers import make_env


# the grouped PPO step runs the 16-row-tile kernels: minibatches below 32 rows per compute unit,
# taken here, without a device, at an MI355X's 256 compute units (GroupStep refuses the rest)
GROUPED_MINIBATCH_ROWS = 32 * 256


class DevicePool:
    """One HIP device per process (torch.distributed rank or LOCAL_RANK), not oversubscribed."""

    def __init__(self, device: Any = None):
        import os

        if device is None and torch.cuda.is_available():
            device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0))
                                  % max(1, torch.cuda.device_count()))
        self.device = torch.device(device) if device is not None else torch.device("cpu")

    def acquire(self):
        import contextlib

        @contextlib.contextmanager
        def _cm():
            yield self.device

        return _cm()


class ExperimentRunner:
    def __init__(self, base_env_config: dict, device_pool=None):
        self.base_config = base_env_config
        self.pool = device_pool or DevicePool()

    @staticmethod
    def _process_group(device):
        """The torchrun world as a process group, or None for a single-process launch."""
        import os

        import torch.distributed as dist

        if int(os.environ.get("WORLD_SIZE", "1")) <= 1 and not dist.is_initialized():
            return None
        if not dist.is_initialized():
            backend = os.environ.get("HWY_DIST_BACKEND") or (
                "nccl" if device.type == "cuda" else "gloo")
            if backend == "nccl":
                torch.cuda.set_device(device)
                dist.init_process_group("nccl", device_id=device)
            else:
                dist.init_process_group(backend)
        return dist.group.WORLD if dist.get_world_size() > 1 else None

    def _create_agent(self, state_dim, action_dim, hp, logger, device, extra=None,
                      process_group=None, seed=None):
        extra = extra or {}
        # the KL target and the lr schedule (PPOAgent): passed only where a cell sets them
        control = {k: extra[k] for k in ("target_kl", "lr_anneal_updates")
                   if extra.get(k) is not None}
        return PPOAgent(state_dim=state_dim, action_dim=action_dim, lr=hp.lr, gamma=hp.gamma,
                        lam=hp.lam, eps_clip=hp.clip_eps, value_coef=hp.value_coef,
                        entropy_coef=hp.entropy_coef, max_grad_norm=hp.max_grad_norm,
                        epochs=hp.epochs, batch_size=hp.batch_size, hidden_dim=hp.hidden_dim,
                        logger=logger, device=device, process_group=process_group,
                        num_minibatches=extra.get("num_minibatches"), seed=seed, **control)

    def launch(self, exp: Experiment) -> Dict[str, Any]:
        results: Dict[str, Any] = {"experiment_name": exp.name, "status": "FAILED"}
        t0 = time.time()
        logger = None
        try:
            with self.pool.acquire() as device:
                group = self._process_group(device)
                rank, world = ((torch.distributed.get_rank(group),
                                torch.distributed.get_world_size(group))
                               if group is not None else (0, 1))
                set_random_seeds(exp.seed)
                if rank == 0:
                    logger = setup_experiment_logger(exp.name)
                else:
                    results["rank"] = rank
                    logger = logging.getLogger(f"hwy.{exp.name}.rank{rank}")
                    logger.addHandler(logging.NullHandler())
                    logger.propagate = False
                logger.info(f"[{exp.name}] Acquired device: {device} | Seed: {exp.seed}")
                logger.info(f"[{exp.name}] Condition: {exp.condition.name} | HPs: {exp.hp}")
                env = None
                agent = None
                try:
                    overrides = dict(exp.env_config_overrides)
                    if "num_envs" in exp.extra:
                        overrides.setdefault("num_envs", exp.extra["num_envs"])
                    if device.type == "cuda":
                        overrides.setdefault("device", device)
                    schedule = exp.extra.get("episode_schedule", "lockstep")
                    if schedule == "reference":
                        overrides.setdefault("vector_env", True)
                    stats_kw = ({"episode_stats": True} if exp.extra.get("episode_stats")
                                else {})
                    from ppo.rollout import check_truncation

                    truncation = check_truncation(exp.extra.get("truncation", "terminal"))
                    if truncation != "terminal":
                        if group is not None:
                            raise ValueError("extra['truncation']='bootstrap' does not run over "
                                             "a process group")
                        stats_kw["truncation"] = truncation
                    if exp.extra.get("safety_stats"):
                        if group is not None:
                            raise ValueError("extra['safety_stats'] does not run over a process "
                                             "group")
                        stats_kw["safety_stats"] = True
                    if exp.extra.get("attribution"):
                        stats_kw["attribution"] = True
                    if exp.extra.get("eval_orders"):
                        stats_kw["eval_orders"] = list(exp.extra["eval_orders"])
                    if exp.extra.get("eval_sensors"):
                        stats_kw["eval_sensors"] = dict(exp.extra["eval_sensors"])
                    if exp.extra.get("sensor") is not None:
                        if group is not None:
                            raise ValueError("extra['sensor'] does not run over a process group")
                        stats_kw["sensor"] = exp.extra["sensor"]
                    if exp.extra.get("eval_shields"):
                        stats_kw["eval_shields"] = dict(exp.extra["eval_shields"])
                    if exp.extra.get("shield") is not None:
                        if group is not None:
                            raise ValueError("extra['shield'] does not run over a process group")
                        stats_kw["shield"] = exp.extra["shield"]
                    grid = None
                    if exp.extra.get("grid") not in (None, False):
                        from hwy._abi import GridSpec

                        if group is not None:
                            raise ValueError("extra['grid'] does not run over a process group")
                        grid = stats_kw["grid"] = GridSpec.from_dict(exp.extra["grid"])
                    if group is not None:
                        e = int(overrides.get("num_envs", 1))
                        if e <= 1:
                            raise ValueError("a multi-rank experiment needs extra['num_envs'] > 1")
                        overrides.update(env_offset=rank * e, global_envs=world * e)
                    env = make_env(exp.condition, self.base_config, d_embed=exp.hp.d_embed,
                                   env_overrides=overrides)
                    if hasattr(env, "to") and callable(env.to):
                        env = env.to(device)
                    if not isinstance(env.observation_space, spaces.Box):
                        raise TypeError(f"Unsupported observation space: {type(env.observation_space)}")
                    state_dim = int(np.prod(env.observation_space.shape))
                    if grid is not None:  # the policy's input is the grid row, not the rows
                        if not hasattr(env.unwrapped, "grid_into"):
                            raise ValueError("extra['grid'] needs the vectorised loop "
                                             "(extra['num_envs'] > 1)")
                        state_dim = grid.stride(int(env.unwrapped.hwy_config.n_features))
                    action_dim = env.action_space.shape[0]
                    logger.info(f"[{exp.name}] state_dim={state_dim}, action_dim={action_dim}")
                    # every rank seeds the global RNGs with exp.seed (the RankPE table and the
                    # initial weights must agree), but each rank's sampling generator gets its
                    # own stream, so global env r*E+e does not replay env e's exploration noise
                    agent_seed = None if group is None else exp.seed * 1000003 + rank
                    agent = self._create_agent(state_dim, action_dim, exp.hp, logger, device,
                                               exp.extra, process_group=group, seed=agent_seed)
                    rewards, avg_rewards, metrics = train_with_experiment_name(
                        env=env, agent=agent, max_episodes=exp.max_episodes,
                        target_reward=exp.target_reward,
                        log_interval=exp.extra.get("log_interval", 20),
                        eval_interval=exp.extra.get("eval_interval", 50),
                        steps_per_update=exp.hp.steps_per_update, experiment_name=exp.name,
                        exp_seed=exp.seed, logger=logger,
                        **({} if schedule == "lockstep" else {"episode_schedule": schedule}),
                        **stats_kw)
                    results.update(status="COMPLETED", rewards=rewards, avg_rewards=avg_rewards,
                                   metrics_history=metrics)
                except Exception as e:
                    logger.error(f"[{exp.name}] Experiment execution failed!", exc_info=True)
                    results["error_message"] = str(e)
                    results["error_traceback"] = traceback.format_exc()
                finally:
                    # graphs holding RCCL collectives are freed while the communicator lives
                    if agent is not None and getattr(agent, "_fused", None) is not None:
                        agent._fused.release_graphs()
                    if env is not None:
                        env.close()
        except Exception as e:
            results["error_message"] = str(e)
            results["error_traceback"] = traceback.format_exc()
        results["duration_seconds"] = time.time() - t0
        if logger:
            logger.info(f"[{exp.name}] Run finished. Status: {results['status']}. "
                        f"Duration: {results['duration_seconds']:.2f}s")
        logging.shutdown()
        return results

    def launch_group(self, exps) -> list:
        """launch() for experiments that differ only in their seed (a sweep cell's seeds), run
        as ONE ExperimentGroup on this runner's device (ppo/group.py: the experiments batched into
        the env, acting and minibatch-step launches; each bit-identical to its solo launch()).
        The reference runs such a cell as len(exps) separate processes oversubscribing the GPUs
        (main.py:188-242, utils/device_pool.py:44-72).  Needs the vectorised loop
        (extra["num_envs"] > 1, or 1 with extra["episode_schedule"] = "reference") and the fused
        HIP learner; returns one status dict per experiment, in order."""
        return self.launch_batch([exps])[0]

    @staticmethod
    def check_batch(cells, own_schedules: bool = False) -> None:
        """launch_batch's argument checks (no device needed): within a cell the experiments
        differ only in seed and name and use the vectorised loop (num_envs > 1, or num_envs 1 on
        the reference episode schedule); across cells they share what one GroupBatch's launches
        share -- envs per experiment, rollout length and the episode schedule -- and the
        training schedule -- and extra["episode_stats"], which selects the env launch they
        share.  The condition and the hidden width may differ between cells.  The
        update's own schedule (batch_size, num_minibatches, epochs) must be shared too, unless
        ``own_schedules`` (what launch_batch passes): then it may differ between cells
        (hwy_ppo_sched_*), and each cell's minibatches must all be of one size, below the grouped
        step's 16-row-tile bound."""
        import math

        from ppo.agent import PPOAgent
        from ppo.rollout import check_episode_schedule, check_truncation

        for exps in cells:
            for e in exps:
                if check_truncation(e.extra.get("truncation", "terminal")) != "terminal":
                    raise ValueError(f"launch_group / launch_batch: extra['truncation']="
                                     f"{e.extra['truncation']!r} is not supported by the grouped "
                                     f"launches (experiment {e.name}); use launch()")

                if e.extra.get("attribution"):
                    raise ValueError(f"launch_group / launch_batch: extra['attribution'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("eval_orders"):
                    raise ValueError(f"launch_group / launch_batch: extra['eval_orders'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("eval_sensors"):
                    raise ValueError(f"launch_group / launch_batch: extra['eval_sensors'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("sensor") is not None:  # any sensor, the null one ({}) too
                    raise ValueError(f"launch_group / launch_batch: extra['sensor'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("grid") not in (None, False):  # any grid, the default one too
                    raise ValueError(f"launch_group / launch_batch: extra['grid'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("eval_shields"):
                    raise ValueError(f"launch_group / launch_batch: extra['eval_shields'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")
                if e.extra.get("shield") is not None:  # any shield, the default one ({}) too
                    raise ValueError(f"launch_group / launch_batch: extra['shield'] is not "
                                     f"supported by the grouped launches (experiment {e.name}); "
                                     f"use launch()")

        def episode_schedule(e):
            return check_episode_schedule(e.extra.get("episode_schedule", "lockstep"))

        for exps in cells:
            key = {(e.condition, repr(e.hp), repr(sorted(e.extra.items())),
                    repr(e.env_config_overrides), e.max_episodes, e.target_reward) for e in exps}
            if len(key) != 1:
                raise ValueError("launch_group: the experiments must differ only in seed and name")
            if (int(exps[0].extra.get("num_envs", 1)) <= 1
                    and episode_schedule(exps[0]) != "reference"):
                raise ValueError("launch_group needs extra['num_envs'] > 1 (the vectorised loop)")
        first = [c[0] for c in cells]
        if len({episode_schedule(e) for e in first}) != 1:
            raise ValueError("launch_batch: the cells must share extra['episode_schedule']")
        if len({bool(e.extra.get("episode_stats", False)) for e in first}) != 1:
            raise ValueError("launch_batch: the cells must share extra['episode_stats']")
        if len({bool(e.extra.get("safety_stats", False)) for e in first}) != 1:
            raise ValueError("launch_batch: the cells must share extra['safety_stats']")

        def shared(e):
            return (int(e.extra.get("num_envs", 1)), e.hp.steps_per_update, e.max_episodes,
                    e.target_reward, e.extra.get("eval_interval", 50))

        def schedule(e):
            return (e.hp.batch_size, e.hp.epochs, e.extra.get("num_minibatches"))

        if not own_schedules and any((shared(e), schedule(e)) != (shared(first[0]),
                                                                   schedule(first[0]))
                                     for e in first):
            raise ValueError("launch_batch: the cells must share num_envs, steps_per_update, "
                             "batch_size, epochs, num_minibatches, max_episodes, target_reward "
                             "and eval_interval (hidden_dim and the condition may differ)")
        for e in first:
            if shared(e) != shared(first[0]):
                raise ValueError(f"launch_batch: the cells must share num_envs, steps_per_update, "
                                 f"max_episodes, target_reward and eval_interval (the condition, "
                                 f"hidden_dim, batch_size, num_minibatches and epochs may differ): "
                                 f"cell {e.name} has {shared(e)}, cell {first[0].name} "
                                 f"{shared(first[0])}")
            E = int(e.extra.get("num_envs", 1))
            n = max(1, math.ceil(e.hp.steps_per_update / E)) * E
            # PPOAgent.minibatch_sizes, which reads only these two attributes
            sizes = PPOAgent.minibatch_sizes(
                type("_Partition", (), {"num_minibatches": e.extra.get("num_minibatches"),
                                        "batch_size": e.hp.batch_size})(), n)
            if len(set(sizes)) != 1:
                raise ValueError(f"launch_batch: cell {e.name} splits its {n} samples into "
                                 f"minibatches of {sorted(set(sizes))} rows; a grouped update "
                                 f"needs equal minibatches")
            if sizes[0] >= GROUPED_MINIBATCH_ROWS:
                raise ValueError(f"launch_batch: cell {e.name} has minibatches of {sizes[0]} rows; "
                                 f"the grouped step takes the 16-row tiles, minibatches below "
                                 f"{GROUPED_MINIBATCH_ROWS} rows")

    def launch_batch(self, cells) -> list:
        """launch_group for several cells at once: each cell (experiments that differ only in
        seed) becomes an ExperimentGroup, and the cells, which must share envs per experiment and
        rollout length (e.g. a sweep's conditions, whose state dims differ, across its hidden
        widths, batch sizes and epochs), are stepped together by one GroupBatch: one set of
        acting launches, one env launch and one grouped minibatch step for all their learners;
        cells whose batch_size, num_minibatches or epochs differ each keep their own minibatch
        schedule inside those steps (hwy_ppo_sched_*).  Every experiment stays bit-identical to
        its solo launch().  Returns one list of status dicts per cell."""
        import math

        from ppo.group import GroupBatch, build_group
        from training.routine import train_batch

        cells = [list(c) for c in cells]
        t0 = time.time()
        self.check_batch(cells, own_schedules=True)
        first = [c[0] for c in cells]
        schedule = first[0].extra.get("episode_schedule", "lockstep")
        # the default schedule passes no keyword: that path is the one without the feature
        sched_kw = {} if schedule == "lockstep" else {"episode_schedule": schedule}
        if first[0].extra.get("episode_stats"):
            sched_kw["episode_stats"] = True
        if first[0].extra.get("safety_stats"):
            sched_kw["safety_stats"] = True
        results = [[{"experiment_name": e.name, "status": "FAILED"} for e in exps]
                   for exps in cells]
        loggers = []
        groups = []
        try:
            with self.pool.acquire() as device:
                for exps in cells:
                    e0 = exps[0]
                    E = int(e0.extra.get("num_envs", 1))
                    cell_loggers = []
                    for e in exps:
                        set_random_seeds(e.seed)  # as launch() does before the logger
                        lg = setup_experiment_logger(e.name)
                        lg.info(f"[{e.name}] Acquired device: {device} | Seed: {e.seed} | group "
                                f"of {len(exps)}")
                        cell_loggers.append(lg)
                    loggers += cell_loggers
                    T = max(1, math.ceil(e0.hp.steps_per_update / E))
                    lg_iter = iter(cell_loggers)

                    def make_agent(sd, e0=e0, lg_iter=lg_iter):
                        return self._create_agent(sd, 2, e0.hp, next(lg_iter), device, e0.extra)

                    groups.append(build_group(e0.condition, self.base_config,
                                              [e.seed for e in exps], E, T, device, make_agent,
                                              d_embed=e0.hp.d_embed,
                                              env_overrides=e0.env_config_overrides,
                                              **sched_kw))
                stepper = groups[0] if len(groups) == 1 else GroupBatch(groups)
                e0 = first[0]
                outs = train_batch(stepper, groups, [e.name for c in cells for e in c],
                                   [e.seed for c in cells for e in c],
                                   max_episodes=e0.max_episodes, target_reward=e0.target_reward,
                                   log_interval=e0.extra.get("log_interval", 20),
                                   eval_interval=e0.extra.get("eval_interval", 50),
                                   loggers=loggers, **sched_kw)
                flat = [res for cell in results for res in cell]
                for res, (rewards, avg_rewards, metrics) in zip(flat, outs):
                    res.update(status="COMPLETED", rewards=rewards, avg_rewards=avg_rewards,
                               metrics_history=metrics)
        except Exception as ex:
            for cell in results:
                for res in cell:
                    res["error_message"] = str(ex)
                    res["error_traceback"] = traceback.format_exc()
        finally:
            for g in groups:
                g.close()
        for cell in results:
            for res in cell:
                res["duration_seconds"] = time.time() - t0
        logging.shutdown()
        return results
