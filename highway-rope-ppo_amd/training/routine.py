"""Training entry point (reference training/routine.py:14-297), on the MI355X env.

``train_with_experiment_name`` keeps the reference's signature, return value
``(rewards, avg_rewards, metrics_history)``, artifact names and schemas:
  * artifacts/highway-ppo/checkpoints/ppo_highway_{best,solved}_<exp>.pth  (:104-107, :208-222)
  * artifacts/highway-ppo/training_metrics_<exp>.json with the same keys  (:88-97, :246-251)
  * artifacts/highway-ppo/summary_<exp>.csv, header
    ``experiment,final_reward,max_reward,steps,best_model,plot``          (:282-295)
  * artifacts/highway-ppo/ppo_highway_rewards_<exp>.png                    (:254-279)

Two loops behind it:
  * a one-env facade env (make_env default) runs the reference's loop as written: per-episode
    ``env.reset(seed=exp_seed + episode_num)`` (:127), batch-1 select_action, list memory,
    ``agent.update(last_value)`` every ``steps_per_update`` steps;
  * a HighwayVecEnv (``num_envs`` > 1) runs E lockstep envs with in-kernel autoreset on the
    same seed schedule (env e's k-th episode gets exp_seed + 1 + e + E*k, = exp_seed +
    episode_num for E = 1), a device RolloutBuffer of T = ceil(steps_per_update / E) steps, and
    ``agent.update_rollout``.  Episode bookkeeping (logging / eval every ``eval_interval``
    completed episodes, best / solved checkpoints, moving average over the last 10 evals) follows
    the reference, with completed episodes counted in env order within each step.
Which option needs the vectorised loop, which a process group or the grouped launches refuse and
which exclude each other is ppo/options.py's table; train_with_experiment_name refuses from it in
one pass before anything runs.  What the options do:
``episode_schedule="reference"`` runs the reference's own schedule (:121-243): after each rollout
every running episode is cut (hwy_cut_episodes, ppo/rollout.py), booked with its partial return
after the rollout's finished episodes and bootstrapped with V of its last state; the next rollout
starts the schedule's next episodes; and the evaluation points that stream crosses are evaluated
before the update, on the weights that collected it (:173-175).  With one env and T =
``steps_per_update`` that is the reference's episode stream, seeds exp_seed + episode_num.  The
default, "lockstep", is the loop above.
``episode_stats=True`` steps the envs with hwy_step_with_info and books, per episode and in the
order of ``episode_rewards`` (cut episodes included), ``episode_lengths``, ``episode_crashed``,
``episode_mean_speed`` (sum of the ego's speed over the episode's steps / its length) and
``episode_lane_changes`` into metrics_history, and a ``crash_rate`` column (over the last 100
episodes) into the summary.  The training itself is unchanged, bit for bit.
``safety_stats=True`` issues one hwy_traffic launch per env step (ppo/rollout.py) and books, per
episode likewise, ``episode_min_ttc``, ``episode_min_headway``, ``episode_min_gap``,
``episode_min_distance`` (the least time-to-collision, time headway, bumper-to-bumper gap to the
front vehicle and centre distance to any vehicle over the states the policy acted on; +inf,
written to the JSON as null, where the episode never had a front vehicle),
``episode_ttc_critical_share`` and ``episode_tailgating_share`` (the share of those states with
ttc < 2 s and headway < 1 s), and a ``near_miss_rate`` column (the share of the last 100 episodes
whose least ttc was below 2 s) into the summary.  The training itself is unchanged, bit for bit.
``safety_profile`` measures the same over evaluate()'s episodes.
``evaluate`` runs ``num_episodes`` deterministic episodes seeded exp_seed + 1000 + k (:14-29),
as one batched env for the vectorised path; ``safety_profile``, ``shield_profile`` and
``attribution`` run the same episodes through the same loop (_run_episodes).
``attribution`` reports what the policy looks at: the mean |input gradient| of acceleration,
steering and value per observed row, per distance rank and per feature column
(PPOAgent.input_gradients at every step).  ``attribution=True`` books it, at the final weights on
the evaluations' seeds, as ``attribution`` in the metrics; it runs after training and draws no
random number, so the training is unchanged, bit for bit.
``visualize_agent`` (:32-58) runs deterministic episodes seeded exp_seed + 2000 + k and, with
``out_dir``, records their frames (HighwayVecEnv.render, one launch per step); there is no window.
``attribution="value"`` (or another of ATTRIBUTION_OUTPUTS) tints every vehicle of every frame by
the policy's input-gradient mass on the observation row that shows it (``attribution_shade``).
``tint="ttc"`` tints them by hwy_traffic's ``risk`` instead (1 - ttc / 4 s below 4 s, else 0),
``tint="hidden"`` with ``sensor=`` the vehicles that sensor does not see (hwy_sense's ``hidden``).
``evaluate(..., order= | sensor= | shield= | grid= | lidar=)`` runs the evaluation's episodes with
the policy acting on the same worlds observed under that row order (HighwayVecEnv.observe), as that
sensor perceives them (HighwayVecEnv.sense; it combines with ``order``), with that shield picking
what the env executes (HighwayVecEnv.shield_into), or on the occupancy grid or the ray-cast range
observation of the states (HighwayVecEnv.view); ``eval_orders``, ``eval_sensors`` and
``eval_shields`` book such evaluations at the final weights as ``order_rewards``,
``sensor_rewards`` and ``shield_rewards``.
``sensor`` / ``grid`` / ``lidar`` (the views: at most one) and ``shield`` train under one: the
rollout applies it at every step (ppo/rollout.py), the run's own evaluations use the same one and
the metrics carry it under its name; under a grid or a lidar the policy's input is
``spec.stride(F)`` wide; a shielded run's updates also carry ``shield_rate`` and the summary its
last value.  ``shield_profile`` counts, on unshielded episodes, the crashes a shield could still
have avoided.
"""

from __future__ import annotations

import json
import logging
import math
import os
import time

import numpy as np
import torch

from ppo import options
from ppo.options import (SAFETY_KEYS, STATS_KEYS, check_eval_orders,  # noqa: F401
                         check_eval_sensors, check_eval_shields)
from utils.logging_utils import ensure_artifacts_dir, setup_experiment_logger

CONTROL_KEYS = tuple(o.name for o in options.OPTIONS if o.on_agent)


def _is_vector(env) -> bool:
    return bool(getattr(env.unwrapped, "is_vector_env", False))


def _flat_dim(env) -> int:
    return int(np.prod(env.observation_space.shape))


# ---------------------------------------------------------------------------------- evaluation
# evaluate()'s refusal of anything beside a view that replaces the rows, by the view's option
_EVALUATE_ALONE = {
    "grid": "evaluate(grid=...) does not go with order, sensor or shield: a grid has no row order, "
            "and the other combinations are not built",
    "lidar": "evaluate(lidar=...) does not go with order, sensor, shield or grid: a lidar has no "
             "row order and its own sensor errors, and the other combinations are not built",
}


def evaluate(env, agent, num_episodes=10, render=False, exp_seed: int = 0, order=None,
             sensor=None, shield=None, tape=None, grid=None, lidar=None):
    """Mean return of deterministic episodes seeded exp_seed + 1000 + k.  ``order`` ("sorted" or
    "shuffled"; vector envs only): the same episodes with the policy acting on the states
    re-observed under that row order (HighwayVecEnv.observe) instead of the step's own rows.
    ``sensor`` (a hwy.SensorModel or its dict; vector envs only): the policy acts on the states as
    that sensor perceives them (HighwayVecEnv.sense), under ``order`` when that is given too.
    ``shield`` (a hwy.Shield or its dict; vector envs only, not with ``sensor`` or ``order``): the
    policy acts, the shield picks what the env executes (HighwayVecEnv.shield_into) and the return
    is the executed episode's.  ``tape`` (with ``shield``): a list that receives, per step, the
    exported state before it, the policy's actions, the executed actions and the shield's choice
    as host arrays (tests); a taped evaluation is always run.
    ``grid`` / ``lidar`` (a hwy.GridSpec / hwy.LidarSpec, its dict, or True for the default; with
    nothing else of these): the policy acts on the occupancy grid / the ray-cast range observation
    of the states (HighwayVecEnv.view; on the one-env facade HighwayEnv.view per step)."""
    from hwy._abi import observe_order

    vector = _is_vector(env)
    given = dict(order=order, sensor=sensor, shield=shield, grid=grid, lidar=lidar)
    for n in _EVALUATE_ALONE:
        given[n] = options.BY_NAME[n].normalise(given[n])
    # a view that replaces the rows goes alone: the last one given refuses whatever precedes it
    own = next((n for n in reversed(_EVALUATE_ALONE) if given[n] is not None), None)
    if own is not None:
        if any(given[n] is not None for n in list(given)[:list(given).index(own)]):
            raise ValueError(_EVALUATE_ALONE[own])
    else:
        # the view the policy acts through is named after the first of these that is given
        view = next((n for n, v in (("shield", shield), ("sensor", sensor), ("order", order))
                     if v is not None), None)
        if view is not None and not vector:
            raise ValueError(f"evaluate({view}=...) needs a HighwayVecEnv (num_envs > 1, or "
                             "make_env's vector_env key for one env)")
        if shield is not None:
            if sensor is not None or order is not None:
                raise ValueError("evaluate(shield=...) does not go with sensor or order: the "
                                 "combination is not tested")
            shield = options.BY_NAME["shield"].normalise(shield)
        elif view is not None:
            sensor = options.BY_NAME["sensor"].normalise(sensor)
            observe_order(order)  # ValueError for anything but None / "sorted" / "shuffled"
    if vector:
        return _evaluate_vector(env, agent, num_episodes, exp_seed, **options.given(
            order=order, sensor=sensor, shield=shield, tape=None if shield is None else tape,
            **{n: given[n] for n in _EVALUATE_ALONE}))
    spec = given.get(own)  # the view the policy acts on instead of the step's rows
    totals = []
    for ep in range(num_episodes):
        state, _ = env.reset(seed=exp_seed + 1000 + ep)
        flat = state.reshape(-1) if spec is None else env.unwrapped.view(spec)
        done, ep_reward = False, 0.0
        while not done:
            action, _, _, _ = agent.select_action(flat, deterministic=True)
            nxt, reward, terminated, truncated, _ = env.step(action)
            done = terminated or truncated
            flat = nxt.reshape(-1) if spec is None else env.unwrapped.view(spec)
            ep_reward += reward
        totals.append(ep_reward)
    return float(np.mean(totals))


def _eval_env_like(env, num_episodes: int):
    """A num_episodes-wide copy of env (same config and fused wrapper), no autoreset."""
    from hwy.vec_env import HighwayVecEnv

    base = env.unwrapped
    cfg = base.hwy_config
    ev = HighwayVecEnv(base.config, num_envs=num_episodes, device=base.device, autoreset=False,
                       pe_kind=cfg.pe_kind, d_embed=cfg.d_embed, ego_idx=cfg.ego_idx,
                       pe_max_dist=cfg.pe_max_dist, pe_table=base._pe_table)
    return ev


def _cached_env(env, attr: str, num_episodes: int, make=None):
    """The num_episodes-wide env of ``env``, made once (``make``, default _eval_env_like) and kept
    on it in the dict ``attr``: ``_eval_envs`` (evaluate), ``_attr_envs``, ``_safety_envs``."""
    base = env.unwrapped
    cache = getattr(base, attr, None)
    if cache is None:
        cache = {}
        setattr(base, attr, cache)
    ev = cache.get(num_episodes)
    if ev is None:
        ev = cache[num_episodes] = (make or _eval_env_like)(env, num_episodes)
    return ev


def _eval_key(agent, num_episodes, exp_seed):
    """Identity of a deterministic evaluation: the same weights (no update since, no torch-side
    parameter write) on the same seeds give the same return, bit for bit."""
    params = tuple((p.data_ptr(), p._version) for p in agent.actor_critic.parameters())
    # on the fused path every p.data is a view of one flat buffer: writes through that buffer
    # (the fused optimizer, a copy into it) bump only the buffer's counter
    flat = getattr(agent, "_flat", None)
    flat_v = (flat[0].data_ptr(), flat[0]._version) if flat is not None else None
    # in-place writes through .data bump neither: PPOAgent.params_written() counts them
    writes = getattr(agent, "_torch_param_writes", 0)
    return (getattr(agent, "updates", None), params, flat_v, num_episodes, exp_seed, writes)


def _evaluate_vector(env, agent, num_episodes, exp_seed, order=None, sensor=None, shield=None,
                     grid=None, tape=None, lidar=None):
    """_run_eval_vector behind a memo.  With thousands of lockstep envs many eval points (every
    eval_interval completed episodes) fall between two updates; the evaluation is deterministic,
    so a repeat at unchanged weights reuses the last result instead of re-running the episodes.
    Each variant has a memo of its own on the env and neither reads nor writes another's: the
    plain one is the pair ``_eval_memo``; the others are dicts of such pairs, ``_eval_<name>_memo``:
    a view's by spec (``_eval_grid_memo``, ``_eval_lidar_memo``; ``_eval_sensor_memo`` by (sensor,
    order)), ``_eval_shield_memo`` by shield and ``_eval_order_memo`` by order, one entry per
    value ever evaluated on this env, never dropped (a handful for eval_sensors; a caller
    sweeping many may clear the dict).  A taped run bypasses the memo."""
    base = env.unwrapped
    key = _eval_key(agent, num_episodes, exp_seed)
    view = options.given_view(dict(sensor=sensor, grid=grid, lidar=lidar))
    if shield is not None:
        name, slot = "shield", (shield,)
    elif view is not None:  # the rows a sensor overwrites differ by their order too
        name, slot = view[0], (view[1],) if view[1].REPLACES_ROWS else (view[1], order)
    elif order is not None:
        name, slot = "order", (order,)
    else:
        name, slot = None, None
    attr = "_eval_memo" if name is None else f"_eval_{name}_memo"
    memo = getattr(base, attr, None)
    if slot is None:
        hit = memo
    else:
        key += slot
        slot = slot[0] if len(slot) == 1 else slot
        if memo is None:
            memo = {}
            setattr(base, attr, memo)
        hit = memo.get(slot)
    if tape is None and hit is not None and hit[0] == key and key[0] is not None:
        return hit[1]
    r = _run_eval_vector(env, agent, num_episodes, exp_seed, **options.given(
        order=order, sensor=sensor, shield=shield, tape=tape, grid=grid, lidar=lidar))
    if slot is None:
        base._eval_memo = (key, r)
    else:
        memo[slot] = (key, r)
    return r


def _run_episodes(ev, first_seed: int, act, after_step=None):
    """One deterministic episode per env of ``ev`` (no autoreset), seeded first_seed + k, all in
    lockstep: ``act(obs, alive)`` gets the current observation and the mask of the episodes still
    running and returns the actions the env executes; ``after_step(alive, terminated, truncated)``,
    if given, sees each step's flags with the mask as it was when the step was taken.  Returns the
    episodes' returns [n] (float64, on the device), summed under the mask."""
    n, dev = ev.num_envs, ev.device
    seeds = torch.arange(n, device=dev, dtype=torch.int64) + first_seed
    obs, _ = ev.reset(seeds=seeds)
    alive = torch.ones(n, dtype=torch.bool, device=dev)
    total = torch.zeros(n, dtype=torch.float64, device=dev)
    for k in range(ev.max_episode_steps + 1):
        obs, r, te, tr, _ = ev.step(act(obs, alive).contiguous())
        total += torch.where(alive, r.double(), torch.zeros_like(total))
        if after_step is not None:
            after_step(alive, te, tr)
        alive &= ~(te.bool() | tr.bool())
        # the host learns "all done" every 8 steps (one sync instead of eight): the steps after
        # every episode ended add nothing to total (alive is all False), so the result is the same
        if k % 8 == 7 and not bool(alive.any()):
            break
    return total


def _shield_tape(tape, ev, alive, actions, executed, chosen, **more) -> None:
    """One step of evaluate(shield=...)'s / shield_profile's ``tape``, as host arrays."""
    if tape is not None:
        host = dict(actions=actions, executed=executed, chosen=chosen, **more, alive=alive)
        tape.append(dict(state=ev.export_state().cpu().numpy(),
                         **{k: v.cpu().numpy().copy() for k, v in host.items()}))


def shield_profile(env, agent, shield, num_episodes=10, exp_seed: int = 0, tape=None):
    """What ``shield`` would have done on evaluate()'s episodes, which run *unshielded*: the
    look-ahead (every candidate, HighwayVecEnv.lookahead_into in hold mode) is called on every
    state an episode acts on and never overrides.  Returns a dict: ``episodes``; ``crashes``, the
    episodes that ended terminated; ``avoidable``, the crashed episodes in whose last acted-on
    state some fallback was safe; ``states``, the states acted on; ``would_override``, those of
    them where the shield would have replaced the policy's action (its candidate 0 terminates
    within the horizon); ``mean_steps0``, the mean steps candidate 0 survives over those states;
    ``reward``, evaluate()'s mean return.  ``tape``: as in evaluate(shield=...), the executed
    actions being the policy's."""
    if not _is_vector(env):
        raise ValueError("shield_profile needs a HighwayVecEnv (num_envs > 1, or make_env's "
                         "vector_env key for one env)")
    shield = options.BY_NAME["shield"].normalise(shield)
    n = int(num_episodes)
    ev = _cached_env(env, "_eval_envs", n)
    dev = ev.device
    K = shield.k
    cand = torch.zeros(n, K, 2, dtype=torch.float32, device=dev)
    cand[:, 1:, :] = torch.tensor(shield.fallbacks, dtype=torch.float32, device=dev)
    steps = torch.zeros(n, K, dtype=torch.int32, device=dev)
    term = torch.zeros(n, K, dtype=torch.uint8, device=dev)
    chosen = torch.zeros(n, dtype=torch.int32, device=dev)
    count = torch.zeros(5, dtype=torch.int64, device=dev)  # crashes, avoidable, states, overrides, steps0

    def act(obs, alive):
        a, _, _, _ = agent.select_action(obs.reshape(n, -1), deterministic=True)
        a = a.contiguous()
        cand[:, 0, :].copy_(a.view(n, 2))
        ev.lookahead_into(cand, shield.horizon, hold=True, steps=steps, terminated=term,
                          chosen=chosen)
        _shield_tape(tape, ev, alive, a, a, chosen, steps=steps, terminated=term)
        return a

    def after_step(alive, te, tr):
        crashed = alive & te.bool()
        count[0] += crashed.sum()
        count[1] += (crashed & (term[:, 1:] == 0).any(dim=1)).sum()  # some fallback was safe
        count[2] += alive.sum()
        count[3] += (alive & (chosen != 0)).sum()
        count[4] += torch.where(alive, steps[:, 0].long(), torch.zeros_like(steps[:, 0].long())).sum()

    total = _run_episodes(ev, exp_seed + 1000, act, after_step)
    c = [int(x) for x in count.cpu().tolist()]
    return {"episodes": n, "crashes": c[0], "avoidable": c[1], "states": c[2],
            "would_override": c[3], "mean_steps0": c[4] / max(c[2], 1),
            "reward": float(total.mean().item())}


def _run_eval_vector(env, agent, num_episodes, exp_seed, order=None, sensor=None, shield=None,
                     tape=None, grid=None, lidar=None):
    ev = _cached_env(env, "_eval_envs", num_episodes)
    dev = ev.device
    seen = None  # a view or an order given: the states as observed under it, in its own buffer
    view = options.given_view(dict(grid=grid, lidar=lidar))  # one that replaces the rows
    if shield is not None:  # the executed actions and the shield's choice
        executed = torch.zeros(num_episodes, 2, dtype=torch.float32, device=dev)
        chosen = torch.zeros(num_episodes, dtype=torch.int32, device=dev)

    def act(obs, alive):
        nonlocal seen
        if view is not None:
            obs = seen = ev.view(view[1], out=seen)
        elif sensor is not None:
            obs = seen = ev.sense(sensor, order=order, out=seen)
        elif order is not None:
            obs = seen = ev.observe(order=order, out=seen)
        a, _, _, _ = agent.select_action(obs.reshape(num_episodes, -1), deterministic=True)
        if shield is None:
            return a
        policy_a = a.contiguous()  # the shield picks what the env executes
        ev.shield_into(shield, policy_a, executed, chosen=chosen)
        _shield_tape(tape, ev, alive, policy_a, executed, chosen)
        return executed

    return float(_run_episodes(ev, exp_seed + 1000, act).mean().item())


# ---------------------------------------------------------------------------------- visualisation
def _vec_base(env):
    """The HighwayVecEnv behind env: itself, or the one inside the one-env facade."""
    base = env.unwrapped
    return getattr(base, "vec_env", base)


def save_frames(path_stem: str, frames: np.ndarray, fps: int = 15) -> list:
    """One episode's frames [T + 1, H, W, 3] as ``<stem>.npy``, and as an animated
    ``<stem>.gif`` when PIL is importable (MP4 is not offered: no encoder is a dependency).
    Returns the paths written."""
    np.save(path_stem + ".npy", frames)
    paths = [path_stem + ".npy"]
    try:
        from PIL import Image
    except ImportError:
        return paths
    imgs = [Image.fromarray(f) for f in frames]
    imgs[0].save(path_stem + ".gif", save_all=True, append_images=imgs[1:],
                 duration=max(1, int(round(1000 / fps))), loop=0)
    return paths + [path_stem + ".gif"]


def attribution_shade(vec_env, grad, order=None):
    """Per-vehicle tint [E, 64] float32 (HighwayVecEnv.render's ``shade``) from one output's input
    gradients ``grad`` [E, N * F_out] (PPOAgent.input_gradients(obs)[name]) at ``vec_env``'s
    current states: per env, the row mass is the sum over the row's F_out columns of |grad|
    divided by the env's largest row mass (0 where that largest mass is 0), scattered to the
    vehicles the rows show (rows_to_vehicles under ``order``; None: the env's own)."""
    E, N = vec_env.num_envs, vec_env.obs_rows
    mass = grad.detach().reshape(E, N, -1).abs().sum(dim=2)
    top = mass.max(dim=1, keepdim=True).values
    rel = torch.where(top > 0, mass / top, torch.zeros_like(mass))
    return vec_env.rows_to_vehicles(rel.to(torch.float32).contiguous(), order=order)


VISUALIZE_TINTS = ("ttc", "hidden", "lidar")
TINT_NEEDS = {"hidden": "sensor", "lidar": "lidar"}  # the view whose launch computes the tint


def visualize_agent(env, agent, num_episodes=3, exp_seed: int = 0, logger=None, out_dir=None,
                    attribution=None, tape=None, tint=None, sensor=None, grid=None, lidar=None):
    """Deterministic episodes of a trained agent, seeded exp_seed + 2000 + ep, on a fresh env of
    ``env``'s config and fused wrapper (reference training/routine.py:32-58, which opens a
    render_mode="human" window; there is no display here).  All ``num_episodes`` run as one
    vector env without autoreset, stepped as evaluate() steps its episodes.  With ``out_dir``
    every step's frames are drawn in one launch (HighwayVecEnv.render) and episode ep's frames --
    the reset frame and one per step up to its own end, [T + 1, H, W, 3] -- are written to
    ``out_dir/viz_episode_<ep + 1>.npy`` (and ``.gif`` when PIL is importable).  Logs
    ``viz_episode=%d reward=%.2f`` per episode and returns the rewards.  ``attribution``: None, or
    one of ATTRIBUTION_OUTPUTS to tint each frame's vehicles by that output's input-gradient mass
    at the frame's own observation (attribution_shade; both are the state after the step).
    ``tint``: None, or "ttc" to tint each frame's vehicles by their time-to-collision risk at the
    frame's state (HighwayVecEnv.traffic_into's ``risk``), or "hidden" to tint the vehicles
    ``sensor`` does not see at the frame's state (HighwayVecEnv.sense_into's ``hidden``); not
    together with ``attribution``.  ``sensor`` (a hwy.SensorModel or its dict): the policy acts on
    what that sensor perceives, as in evaluate(sensor=...); "hidden" needs it.  ``grid`` /
    ``lidar`` (a hwy.GridSpec / hwy.LidarSpec, its dict, or True for the default): the policy acts
    on the occupancy grid / the ray-cast range observation of the states, as in evaluate(grid=...);
    not with another view or ``attribution`` (whose overlay is per Kinematics row);
    ``tint="lidar"`` with a lidar tints the vehicles some cell of it returns at the frame's state
    (HighwayVecEnv.lidar_into's ``seen``).
    ``tape``: a list that receives, per grabbed step, (observation, exported state, the episodes
    still recording) as clones (tests)."""
    if attribution is not None and attribution not in ATTRIBUTION_OUTPUTS:
        raise ValueError(f"attribution must be None or one of {ATTRIBUTION_OUTPUTS}, got "
                         f"{attribution!r}")
    if tint is not None and tint not in VISUALIZE_TINTS:
        raise ValueError(f"tint must be None or one of {VISUALIZE_TINTS}, got {tint!r}")
    if tint is not None and attribution is not None:
        raise ValueError("tint and attribution both shade the vehicles: give one of them")
    views = dict(sensor=sensor, grid=grid, lidar=lidar)
    for i, name in enumerate(options.VIEWS):  # each refuses the views before it, and its tint
        views[name] = options.BY_NAME[name].normalise(views[name])
        before = options.VIEWS[:i]
        if views[name] is not None and before and (
                attribution is not None or any(views[b] is not None for b in before)):
            raise ValueError(f"visualize_agent({name}=...) does not go with {', '.join(before)} "
                             "or attribution")
        if views[name] is None and TINT_NEEDS.get(tint) == name:
            raise ValueError(f'tint="{tint}" needs a {name}')
    view = options.given_view(views)

    if logger is None:
        logger = logging.getLogger(__name__)
    logger.info("Visualizing agent...")
    n = int(num_episodes)
    if n < 1:
        return []
    ev = _eval_env_like(_vec_base(env), n)
    try:
        dev = ev.device
        seeds = torch.arange(n, device=dev, dtype=torch.int64) + (exp_seed + 2000)
        def acted_on(obs):
            """What the policy acts on at the state whose rows are ``obs``: under a view its rows,
            in ``obs``'s shape where it overwrites them."""
            if view is None:
                return obs
            rows = ev.view(view[1])
            return rows if view[1].REPLACES_ROWS else rows.view_as(obs)

        obs = acted_on(ev.reset(seeds=seeds)[0])
        alive = torch.ones(n, dtype=torch.bool, device=dev)
        total = torch.zeros(n, dtype=torch.float64, device=dev)
        frames = [[] for _ in range(n)]
        running = [True] * n

        def grab():
            shade = None
            if attribution is not None:
                g = agent.input_gradients(obs.reshape(n, -1))[attribution]
                shade = attribution_shade(ev, g)
            elif tint == "ttc":
                shade = torch.empty(n, 64, dtype=torch.float32, device=dev)
                ev.traffic_into(risk=shade)
            elif tint == "hidden":
                shade = ev.hidden_vehicles(views["sensor"])
            elif tint == "lidar":
                shade = torch.empty(n, 64, dtype=torch.float32, device=dev)
                ev.lidar_into(views["lidar"], seen=shade)
            host = ev.render(shade=shade).cpu().numpy()
            if tape is not None:
                tape.append((obs.clone(), ev.export_state(), list(running)))
            for ep in range(n):
                if running[ep]:
                    frames[ep].append(host[ep])

        if out_dir is not None:
            grab()
        for _ in range(ev.max_episode_steps + 1):
            a, _, _, _ = agent.select_action(obs.reshape(n, -1), deterministic=True)
            obs, r, te, tr, _ = ev.step(a.contiguous())
            obs = acted_on(obs)
            total += torch.where(alive, r.double(), torch.zeros_like(total))
            if out_dir is not None:
                grab()  # the frame after this step, for the episodes that took it
            alive &= ~(te.bool() | tr.bool())
            running = alive.cpu().tolist()
            if not any(running):
                break
        rewards = [float(x) for x in total.cpu().tolist()]
    finally:
        ev.close()
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
    for ep, rew in enumerate(rewards):
        if out_dir is not None:
            save_frames(os.path.join(out_dir, f"viz_episode_{ep + 1}"), np.stack(frames[ep]))
        logger.info("viz_episode=%d reward=%.2f", ep + 1, rew)
    return rewards


# ---------------------------------------------------------------------------------- attribution
ATTRIBUTION_OUTPUTS = ("acceleration", "steering", "value")


def attribution_from(base_obs, grads, alive, n_base_features, ego_idx=0, features=None,
                     absolute=False):
    """One step's contribution to the attribution statistic, on torch tensors of any device.

    ``base_obs`` (B, N, F): the un-embedded Kinematics rows the policy saw (before any RankPE /
    DistPE / RoPE wrapper); ``grads`` (3, B, N * F_out): the input gradients of (acceleration,
    steering, value) with respect to the wrapped, flattened observation
    (PPOAgent.input_gradients); ``alive`` (B,) bool: the samples that count; ``n_base_features``
    = F.  Returns float64 sums and the sample count, so that steps add up:

      by_row[k][n][f]   sum over alive samples of |grad_k[n, f]|, rows as observed
      by_rank[k][r][f]  the same with each sample's rows reordered by rank: rank 0 is row
                        ``ego_idx``; every other non-empty row follows by (sqrt(x^2 + y^2) in
                        float64, row index) ascending, x and y being base columns 0 and 1; rows
                        whose F base features are all exactly 0.0 (absent vehicles) come last, by
                        row index.  None unless the base features begin with x, y (``features``,
                        the observation config's list; None: they do) and are relative to the ego
                        (``absolute`` False)
      count             alive samples (int64 tensor)

    attribution_stats turns summed results into the reported numbers."""
    B, N, F = base_obs.shape
    if F != n_base_features:
        raise ValueError(f"base_obs has {F} features per row, n_base_features says {n_base_features}")
    if grads.dim() != 3 or grads.shape[0] != 3 or grads.shape[1] != B or grads.shape[2] % N:
        raise ValueError(f"grads must be (3, {B}, {N} * F_out), got {tuple(grads.shape)}")
    Fo = grads.shape[2] // N
    if Fo < F:
        raise ValueError(f"grads have {Fo} columns per row, fewer than the {F} base features")
    if not 0 <= ego_idx < N:
        raise ValueError(f"ego_idx {ego_idx} outside the {N} rows")
    g = grads.reshape(3, B, N, Fo).abs().double()
    w = alive.to(g.device).reshape(1, B, 1, 1).double()
    g = g * w
    out = {"by_row": g.sum(dim=1), "by_rank": None,
           "count": alive.to(torch.int64).sum()}
    ranked = (F >= 2 and not absolute
              and (features is None or list(features[:2]) == ["x", "y"]))
    if ranked:
        b = base_obs.double()
        dist = torch.sqrt(b[..., 0] * b[..., 0] + b[..., 1] * b[..., 1])
        cls = torch.where((base_obs == 0).all(dim=-1), 2, 1)
        cls[:, ego_idx] = 0
        dist = torch.where(cls == 1, dist, torch.zeros_like(dist))
        # (class, distance, row index) ascending: two stable sorts, the minor key first
        by_dist = torch.argsort(dist, dim=1, stable=True)
        by_cls = torch.argsort(torch.gather(cls, 1, by_dist), dim=1, stable=True)
        order = torch.gather(by_dist, 1, by_cls)  # order[b, r]: the row at rank r
        idx = order.to(g.device).reshape(1, B, N, 1).expand(3, B, N, Fo)
        out["by_rank"] = torch.gather(g, 2, idx).sum(dim=1)
    return out


def attribution_add(total, part):
    """Sum of two attribution_from results (``total`` may be None)."""
    if total is None:
        return dict(part)
    return {"by_row": total["by_row"] + part["by_row"],
            "by_rank": (None if total["by_rank"] is None or part["by_rank"] is None
                        else total["by_rank"] + part["by_rank"]),
            "count": total["count"] + part["count"]}


def attribution_stats(sums, n_base_features, ego_idx=0):
    """The reported numbers of summed attribution_from results, as plain Python: ``by_row`` and
    ``by_rank`` divided by the sample count (mean |gradient| per observed row / rank and feature
    column, nested lists [3][N][F_out]; zeros without a sample), ``pe_share[k]`` the mass on the
    embedding columns f >= F over the total mass (None when the observation has none, F_out == F)
    and ``ego_share[k]`` row ``ego_idx``'s mass over the total (shares are None where the total
    is 0), ``samples`` the count; k indexes ATTRIBUTION_OUTPUTS."""
    n = int(sums["count"])
    by_row = sums["by_row"].detach().cpu()
    F = n_base_features
    Fo = by_row.shape[2]
    mean = (lambda t: (t / n if n else torch.zeros_like(t)).tolist())
    # total = base + embedding mass, so that a share is exactly 1.0 when the rest is exactly 0
    pe = by_row[:, :, F:].sum(dim=(1, 2))
    total = by_row[:, :, :F].sum(dim=(1, 2)) + pe
    share = (lambda part: [float(p / t) if float(t) > 0.0 else None
                           for p, t in zip(part, total)])
    return {
        "outputs": list(ATTRIBUTION_OUTPUTS),
        "by_row": mean(by_row),
        "by_rank": None if sums["by_rank"] is None else mean(sums["by_rank"].detach().cpu()),
        "pe_share": None if Fo == F else share(pe),
        "ego_share": share(by_row[:, ego_idx, :].sum(dim=1)),
        "samples": n,
    }


def _attribution_env_like(env, num_episodes: int):
    """_eval_env_like without the fused observation wrapper: the env emits the un-embedded rows,
    and attribution applies the wrapper with the stand-alone op (hwy.ops.obs_pe), whose rows are
    the fused env's bit for bit."""
    from hwy.vec_env import HighwayVecEnv

    base = env.unwrapped
    return HighwayVecEnv(base.config, num_envs=num_episodes, device=base.device, autoreset=False)


def _obs_wrapper_of(env):
    """env's fused observation wrapper as a function of un-embedded rows (..., N, F): the
    stand-alone op with the env's kind, width, ego row, distance scale and table."""
    from hwy import ops

    base = env.unwrapped
    cfg = base.hwy_config
    kind, d = int(cfg.pe_kind), int(cfg.d_embed)
    if kind == ops.PE_NONE:
        return lambda b: b
    table = None if base._pe_table is None else torch.as_tensor(base._pe_table, device=base.device)
    ego, max_dist = int(cfg.ego_idx), float(cfg.pe_max_dist)
    return lambda b: ops.obs_pe(b, kind, d, ego, max_dist, table)


def attribution(env, agent, num_episodes=10, exp_seed: int = 0, tape=None):
    """What the policy looks at, over exactly evaluate()'s episodes (seeds exp_seed + 1000 + k,
    deterministic acting): at every step of every running episode the input gradients of
    (acceleration, steering, value) (PPOAgent.input_gradients), accumulated as mean |gradient|
    per observed row and per distance rank and feature column (attribution_from /
    attribution_stats).  Returns attribution_stats' dict plus ``mean_reward``, which equals
    evaluate(env, agent, num_episodes, exp_seed).  Vector envs only.  ``tape``: a list that
    receives every step's (base_obs, observation, alive) clones (tests)."""
    if not _is_vector(env):
        raise ValueError("attribution needs a HighwayVecEnv (num_envs > 1, or make_env's "
                         "vector_env key for one env)")
    base = env.unwrapped
    cfg = base.hwy_config
    ev = _cached_env(env, "_attr_envs", num_episodes, _attribution_env_like)
    wrap = _obs_wrapper_of(env)
    from hwy._abi import _OBS_DEFAULTS

    features = (base.config.get("observation") or {}).get("features") or _OBS_DEFAULTS["features"]
    F = ev.obs_features
    sums = None

    def act(base_obs, alive):
        nonlocal sums
        obs = wrap(base_obs).reshape(num_episodes, -1)
        g = agent.input_gradients(obs)
        grads = torch.stack([g[n] for n in ATTRIBUTION_OUTPUTS])
        sums = attribution_add(sums, attribution_from(
            base_obs, grads, alive, F, int(cfg.ego_idx), features=features,
            absolute=bool(cfg.absolute)))
        if tape is not None:
            tape.append((base_obs.clone(), obs.clone(), alive.clone()))
        return agent.select_action(obs, deterministic=True)[0]

    total = _run_episodes(ev, exp_seed + 1000, act)
    out = attribution_stats(sums, F, int(cfg.ego_idx))
    out["mean_reward"] = float(total.mean().item())
    return out


_attribution = attribution  # train_with_experiment_name's keyword shadows the name


# ---------------------------------------------------------------------------------- safety
def safety_row(row) -> tuple:
    """One episode's SAFETY_KEYS values from its hwy_traffic reduction row [8] (float32): the
    four minima as they are, the two counts over the states counted (0 of 0 states: 0)."""
    from hwy._abi import (TACC_MIN_DISTANCE, TACC_MIN_GAP, TACC_MIN_THW, TACC_MIN_TTC, TACC_N,
                          TACC_TAILGATING, TACC_TTC_CRITICAL)

    n = max(float(row[TACC_N]), 1.0)
    return (float(row[TACC_MIN_TTC]), float(row[TACC_MIN_THW]), float(row[TACC_MIN_GAP]),
            float(row[TACC_MIN_DISTANCE]), float(row[TACC_TTC_CRITICAL]) / n,
            float(row[TACC_TAILGATING]) / n)


def near_miss_rate(min_ttc, ttc_thresh=None, last: int = 100) -> float:
    """Share of the last ``last`` booked episodes whose least time-to-collision was below
    ``ttc_thresh`` (default: hwy_traffic's, 2 s); 0 with none booked."""
    from hwy._abi import TRAFFIC_DEFAULTS

    thresh = TRAFFIC_DEFAULTS["ttc_thresh"] if ttc_thresh is None else float(ttc_thresh)
    tail = [v for v in list(min_ttc)[-last:]]
    return float(np.mean([v is not None and v < thresh for v in tail])) if tail else 0.0


def _safety_stream(dones, traffic_stats, cut=None):
    """The hwy_traffic reduction rows of one rollout's episode stream, in _episode_ends' /
    _episode_stream's order: the rows of the episodes that finished in the [T, E] rollout
    (traffic_stats [T, E, 8]), then, on the reference schedule, those of the episodes cut at its
    end, which the last step's launch wrote to traffic_stats[T - 1] (ppo/rollout.py)."""
    d = dones.cpu().numpy() != 0
    stats = traffic_stats.cpu().numpy()
    rows = stats[d]
    if cut is not None:
        rows = np.concatenate([rows, stats[-1][cut.cpu().numpy() != 0]])
    return rows


def _book_safety(mh, rows, i) -> None:
    """Episode i of a _safety_stream into metrics_history's SAFETY_KEYS lists."""
    for k, v in zip(SAFETY_KEYS, safety_row(rows[i])):
        mh[k].append(v)


def _json_ready(mh: dict) -> dict:
    """metrics_history as it is written: a non-finite SAFETY_KEYS entry (an episode without a
    front vehicle has no least ttc) becomes null; everything else is the dict's own."""
    if not any(k in mh for k in SAFETY_KEYS):
        return mh
    out = dict(mh)
    for k in SAFETY_KEYS:
        if k in out:
            out[k] = [v if math.isfinite(v) else None for v in out[k]]
    return out


def safety_profile(env, agent, num_episodes=10, exp_seed: int = 0):
    """How close the policy drives, over exactly evaluate()'s episodes (seeds exp_seed + 1000 +
    k, deterministic acting): hwy_traffic on every state the policy acts on, reduced per episode.
    Returns ``episodes`` -- a dict of SAFETY_KEYS (without the ``episode_`` prefix) plus
    ``states`` and ``reward``, each a list with one value per episode -- their means as
    ``mean_<key>`` (+inf where an episode's value is), ``near_miss_rate`` and ``mean_reward``,
    which equals evaluate(env, agent, num_episodes, exp_seed).  It runs on an env of its own and
    leaves evaluate()'s memo alone.  Vector envs only."""
    if not _is_vector(env):
        raise ValueError("safety_profile needs a HighwayVecEnv (num_envs > 1, or make_env's "
                         "vector_env key for one env)")
    from hwy._abi import HWY_TRAFFIC_NACC, TACC_N

    ev = _cached_env(env, "_safety_envs", num_episodes)
    acc = torch.zeros(num_episodes, HWY_TRAFFIC_NACC, dtype=torch.float32, device=ev.device)
    rows = torch.zeros_like(acc)

    def act(obs, alive):
        nonlocal rows
        # the state the policy is about to act on; a finished episode's row stays as it ended
        ev.traffic_into(acc=acc)
        rows = torch.where(alive[:, None], acc, rows)
        return agent.select_action(obs.reshape(num_episodes, -1), deterministic=True)[0]

    total = _run_episodes(ev, exp_seed + 1000, act)
    host = rows.cpu().numpy()
    names = [k[len("episode_"):] for k in SAFETY_KEYS]
    per = {n: [] for n in names}
    for row in host:
        for n, v in zip(names, safety_row(row)):
            per[n].append(v)
    per["states"] = [int(x) for x in host[:, TACC_N]]
    per["reward"] = [float(x) for x in total.cpu().tolist()]
    out = {"episodes": per}
    out.update({f"mean_{n}": float(np.mean(per[n])) for n in names})
    out["near_miss_rate"] = near_miss_rate(per["min_ttc"], last=num_episodes)
    out["mean_reward"] = float(total.mean().item())
    return out


def evaluate_many(items, num_episodes=5):
    """evaluate(env, agent, num_episodes, exp_seed) for every (env, agent, exp_seed) of `items`,
    each result exactly what evaluate returns for it alone: the evaluations that are not memoised
    run together, one set of grouped acting launches (hwy_ppo_group_act, or hwy_ppo_mixed_act
    when their hidden widths differ) and one grouped env launch (hwy_step_group) per step over all
    their evaluation envs, the same kernels and the same per-episode float64 sums as the solo
    loop.  Falls back to one evaluate per item where the items cannot share launches: torch
    acting, a single item, or (_run_eval_group, agents of one width) weight tile images that only
    some agents have -- agents of different widths never take that fallback, because
    GroupAct.tiles() gives those without an image an acting-only one (hwy_ppo_act's two weight
    paths give the same bits: tests/test_mixed_group_gpu.py)."""
    out = [None] * len(items)
    todo = []
    for i, (env, agent, seed) in enumerate(items):
        key = _eval_key(agent, num_episodes, seed)
        memo = getattr(env.unwrapped, "_eval_memo", None)
        if memo is not None and memo[0] == key and key[0] is not None:
            out[i] = memo[1]
        else:
            todo.append(i)
    grouped, solo = [], []
    for i in todo:
        env, agent, _ = items[i]
        ok = (_is_vector(env) and getattr(agent, "backend", "torch") != "torch"
              and agent.device.type == "cuda")
        (grouped if ok else solo).append(i)
    if len(grouped) < 2:
        solo, grouped = sorted(solo + grouped), []
    for i in solo:
        out[i] = evaluate(items[i][0], items[i][1], num_episodes=num_episodes,
                          exp_seed=items[i][2])
    if grouped:
        res = _run_eval_group([items[i] for i in grouped], num_episodes)
        for i, r in zip(grouped, res):
            env, agent, seed = items[i]
            env.unwrapped._eval_memo = (_eval_key(agent, num_episodes, seed), r)
            out[i] = r
    return out


def _run_eval_group(items, num_episodes):
    """_run_eval_vector for several experiments in lockstep (evaluate_many)."""
    from hwy.ppo_native import GroupAct
    from hwy.vec_env import GroupEnvStep

    rows = []
    n, k = num_episodes, len(items)
    agents = [a for _, a, _ in items]
    evs = [_cached_env(env, "_eval_envs", n) for env, _, _ in items]
    dev = evs[0].device
    act = GroupAct(agents, n)
    tiles = act.tiles()
    if any((t is None) != (tiles[0] is None) for t in tiles):  # one acting kernel per launch
        return [_run_eval_vector(env, agent, n, seed) for env, agent, seed in items]
    rew = torch.empty(k * n, device=dev)
    te = torch.empty(k * n, dtype=torch.uint8, device=dev)
    tr = torch.empty(k * n, dtype=torch.uint8, device=dev)
    ios, keep = [], []  # keep: the act outputs the kernels write through raw addresses
    for j, ((env, agent, seed), ev) in enumerate(zip(items, evs)):
        seeds = torch.arange(n, device=dev, dtype=torch.int64) + (seed + 1000)
        obs, _ = ev.reset(seeds=seeds)  # the eval handle's obs_buf, read and rewritten in place
        a = torch.empty(n, 2, device=dev)
        pre = torch.empty(n, 2, device=dev)
        lp = torch.empty(n, device=dev)
        val = torch.empty(n, device=dev)
        sl = slice(j * n, (j + 1) * n)
        keep.append((a, pre, lp, val))
        rows.append((obs.data_ptr(), None, a.data_ptr(), pre.data_ptr(), lp.data_ptr(),
                     val.data_ptr()))
        ios.append((a, obs, rew[sl], te[sl], tr[sl], None, None))
    step = GroupEnvStep(evs)
    alive = torch.ones(k * n, dtype=torch.bool, device=dev)
    total = torch.zeros(k * n, dtype=torch.float64, device=dev)
    for s_ in range(max(ev.max_episode_steps for ev in evs) + 1):
        act.launch(rows, tiles)
        step.launch(ios)
        total += torch.where(alive, rew.double(), torch.zeros_like(total))
        alive &= ~(te.bool() | tr.bool())
        if s_ % 8 == 7 and not bool(alive.any()):
            break
    res = [float(total[j * n:(j + 1) * n].mean().item()) for j in range(k)]
    del keep
    return res


# ---------------------------------------------------------------------------------- artifacts
def _save_artifacts(artifacts_dir, checkpoint_dir, experiment_name, metrics_history,
                    training_episodes, episode_rewards, eval_episodes, rewards, avg_rewards,
                    target_reward, total_steps, logger, exp_prefix):
    metrics_path = os.path.join(artifacts_dir, f"training_metrics_{experiment_name}.json")
    with open(metrics_path, "w") as f:
        json.dump(_json_ready(metrics_history), f, indent=2)
    logger.info(f"{exp_prefix} Metrics saved to {metrics_path}")
    plot_path = os.path.join(artifacts_dir, f"ppo_highway_rewards_{experiment_name}.png")
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt

        plt.figure(figsize=(12, 8))
        plt.plot(training_episodes, episode_rewards, alpha=0.3, label="Training Reward", color="gray")
        if len(episode_rewards) > 20:
            sm = np.convolve(episode_rewards, np.ones(20) / 20, mode="valid")
            plt.plot(training_episodes[19:], sm, label="Training (Moving Avg)")
        plt.plot(eval_episodes, rewards, "ro-", label="Eval Reward")
        plt.plot(eval_episodes, avg_rewards, "go-", label="Eval Moving Avg")
        plt.axhline(y=target_reward, color="r", linestyle="--", label="Target Reward")
        plt.xlabel("Episode")
        plt.ylabel("Reward")
        plt.title(f"Training Progress ({experiment_name})")
        plt.legend()
        plt.grid(alpha=0.3)
        plt.savefig(plot_path, bbox_inches="tight")
        plt.close()
        logger.info(f"{exp_prefix} Training plot saved to {plot_path}")
    except Exception as e:  # plotting is cosmetic
        logger.warning(f"{exp_prefix} plot failed: {e}")
    csv_path = os.path.join(artifacts_dir, f"summary_{experiment_name}.csv")
    best_model_path = os.path.join(checkpoint_dir, f"ppo_highway_best_{experiment_name}.pth")
    head, tail = "", ""
    if "episode_crashed" in metrics_history:  # episode_stats runs only
        head, tail = ",crash_rate", f",{crash_rate(metrics_history['episode_crashed']):.4f}"
    if "episode_min_ttc" in metrics_history:  # safety_stats runs only
        head = f"{head},near_miss_rate"
        tail = f"{tail},{near_miss_rate(metrics_history['episode_min_ttc']):.4f}"
    for k in CONTROL_KEYS:  # runs with a KL target / an lr schedule only
        if k in metrics_history:
            head, tail = f"{head},{k}", f"{tail},{metrics_history[k]}"
    if "shield" in metrics_history:  # shielded runs only: the last update's share of overrides
        ups = [u["shield_rate"] for u in metrics_history["policy_updates"] if "shield_rate" in u]
        head, tail = f"{head},shield_rate", f"{tail},{(ups[-1] if ups else 0.0):.4f}"
    with open(csv_path, "w") as f:
        f.write(f"experiment,final_reward,max_reward,steps,best_model,plot{head}\n")
        f.write(f"{experiment_name},{avg_rewards[-1]:.4f},{max(avg_rewards):.4f},{total_steps},"
                f"{best_model_path},{os.path.basename(plot_path)}{tail}\n")
    logger.info(f"{exp_prefix} Summary CSV saved to {csv_path}")


def crash_rate(crashed, last: int = 100) -> float:
    """Share of the last ``last`` booked episodes that ended in a crash (0 with none booked)."""
    tail = list(crashed)[-last:]
    return float(np.mean(tail)) if tail else 0.0


def _stats_stream(dones, ep_length, ep_stats, cut=None, cut_length=None, acc=None):
    """The per-episode statistics of one rollout's episode stream, in _episode_ends' /
    _episode_stream's order: for the episodes that finished in the [T, E] rollout their ep_stats
    rows ([T, E, 8], hwy_step_with_info) and lengths, then, on the reference schedule, for the
    episodes cut at its end the running sums ``acc`` [E, 8] as the cut left them, with the cut's
    lengths (a cut episode has not crashed: a crash would have ended it).  Returns the [n, 8]
    float32 sums (slot 6: crashed) and the [n] lengths."""
    d = dones.cpu().numpy() != 0
    sums = ep_stats.cpu().numpy()[d]
    lens = ep_length.cpu().numpy()[d]
    if cut is not None:
        c = cut.cpu().numpy() != 0
        sums = np.concatenate([sums, acc.cpu().numpy()[c]])
        lens = np.concatenate([lens, cut_length.cpu().numpy()[c]])
    return sums, lens


def _book_stats(mh, sums, lens, i) -> None:
    """Episode i of a _stats_stream into metrics_history's four lists."""
    from hwy._abi import ACC_CRASHED, ACC_LANE_CHANGES, ACC_SPEED

    n = int(lens[i])
    mh["episode_lengths"].append(n)
    mh["episode_crashed"].append(bool(sums[i, ACC_CRASHED] != 0))
    mh["episode_mean_speed"].append(float(np.float64(sums[i, ACC_SPEED]) / max(n, 1)))
    mh["episode_lane_changes"].append(int(sums[i, ACC_LANE_CHANGES]))


class _EvalTracker:
    """Eval / moving-average / checkpoint bookkeeping of routine.py:172-222."""

    def __init__(self, env, agent, exp_seed, target_reward, checkpoint_dir, experiment_name,
                 metrics_history, logger, exp_prefix, start_time, shield=None, view=None):
        self.env, self.agent, self.exp_seed = env, agent, exp_seed
        # the shield or the view (options.given_view's pair) the run trains under, never both:
        # its own evaluations use it too
        self.eval_kw = options.given(shield=shield, **dict([view] if view else []))
        self.target_reward = target_reward
        self.checkpoint_dir, self.name = checkpoint_dir, experiment_name
        self.mh, self.logger, self.prefix, self.t0 = metrics_history, logger, exp_prefix, start_time
        self.rewards, self.avg_rewards, self.eval_episodes = [], [], [0]
        self.best = -float("inf")
        self.solved = False

    def _evaluate(self):
        return evaluate(self.env, self.agent, num_episodes=5, exp_seed=self.exp_seed,
                        **self.eval_kw)

    def initial(self, r=None):
        if r is None:
            r = self._evaluate()
        self.rewards.append(r)
        self.avg_rewards.append(r)
        self.mh["eval_rewards"].append(r)
        self.mh["avg_eval_rewards"].append(r)
        self.mh["eval_episode_numbers"].append(0)
        self.mh["timestamps"].append(0)
        self.logger.info(f"{self.prefix} initial_eval reward={r:.2f}")

    def on_episode(self, episode_num, r=None):
        """r: the evaluation's result when the caller ran it (evaluate_many), else evaluated here."""
        self.logger.info(f"{self.prefix} Evaluating at episode {episode_num}...")
        if r is None:
            r = self._evaluate()
        self.rewards.append(r)
        self.eval_episodes.append(episode_num)
        elapsed = time.time() - self.t0
        avg = float(np.mean(self.rewards[-10:])) if len(self.rewards) >= 10 else float(np.mean(self.rewards))
        self.avg_rewards.append(avg)
        self.mh["eval_rewards"].append(r)
        self.mh["avg_eval_rewards"].append(avg)
        self.mh["eval_episode_numbers"].append(episode_num)
        self.mh["timestamps"].append(elapsed)
        self.logger.info("%s eval episode=%d reward=%.2f avg_reward=%.2f time=%.2fs", self.prefix,
                         episode_num, r, avg, elapsed)
        if avg >= self.target_reward and not self.solved and len(self.rewards) >= 10:
            self.logger.info(f"{self.prefix} Environment solved in {episode_num} episodes! avg reward={avg:.2f}")
            self.agent.save(os.path.join(self.checkpoint_dir, f"ppo_highway_solved_{self.name}.pth"))
            self.solved = True
        if avg > self.best:
            self.best = avg
            self.agent.save(os.path.join(self.checkpoint_dir, f"ppo_highway_best_{self.name}.pth"))
            self.logger.info(f"{self.prefix} New best model saved, avg reward={self.best:.2f}")


# ---------------------------------------------------------------------------------- training
def train_with_experiment_name(env, agent, max_episodes=500, target_reward=0.0, log_interval=20,
                               eval_interval=50, steps_per_update=2048, experiment_name="",
                               exp_seed: int = 0, logger=None, episode_schedule="lockstep",
                               episode_stats: bool = False, truncation: str = "terminal",
                               attribution: bool = False, eval_orders=None,
                               safety_stats: bool = False, sensor=None, eval_sensors=None,
                               shield=None, eval_shields=None, grid=None, lidar=None):
    group = getattr(agent, "_dist", None)
    # every option normalised, and every refusal (ppo/options.py's table, in its ROUTINE_ORDER)
    opts = options.check_run(
        dict(episode_schedule=episode_schedule, episode_stats=episode_stats,
             truncation=truncation, attribution=attribution, eval_orders=eval_orders,
             safety_stats=safety_stats, sensor=sensor, eval_sensors=eval_sensors, shield=shield,
             eval_shields=eval_shields, grid=grid, lidar=lidar, **_controls_of(agent)),
        lambda: _is_vector(env), group is not None)
    if logger is None:
        logger = setup_experiment_logger(experiment_name)
    exp_prefix = f"[{experiment_name}]" if experiment_name else ""
    logger.info(f"{exp_prefix} Starting training for experiment: {experiment_name}")
    metrics_history = _new_metrics(experiment_name, opts)
    start_time = time.time()
    artifacts_dir = ensure_artifacts_dir()
    checkpoint_dir = os.path.join(artifacts_dir, "checkpoints")
    os.makedirs(checkpoint_dir, exist_ok=True)
    tracker = _EvalTracker(env, agent, exp_seed, target_reward, checkpoint_dir, experiment_name,
                           metrics_history, logger, exp_prefix, start_time, shield=opts["shield"],
                           view=options.given_view(opts))
    rank, _ = _rank_world(group)
    if rank == 0:
        logger.info(f"{exp_prefix} Performing initial evaluation...")
        tracker.initial()
    if not _is_vector(env) and group is not None:
        raise ValueError("a process group needs the vectorised env (num_envs > 1)")
    loop = _train_vector if _is_vector(env) else _train_single
    # the default passes no keyword: that path is the one without the feature
    loop_kw = options.given(**{o.name: opts[o.name] for o in options.OPTIONS if o.rollout})
    episode_rewards, training_episodes, total_steps = loop(
        env, agent, max_episodes, log_interval, eval_interval, steps_per_update, exp_seed, logger,
        exp_prefix, metrics_history, tracker, start_time, **loop_kw)
    if rank != 0:
        return tracker.rewards, tracker.avg_rewards, metrics_history
    if opts["attribution"]:  # after training, at the final weights, on the evaluations' seeds
        metrics_history["attribution"] = _attribution(env, agent, num_episodes=5,
                                                      exp_seed=exp_seed)
    # likewise: the final weights under each row order, sensor and shield (None: unshielded),
    # over evaluate()'s episodes
    for key, view, variants in (("order_rewards", "order", {n: n for n in opts["eval_orders"]}),
                                ("sensor_rewards", "sensor", opts["eval_sensors"]),
                                ("shield_rewards", "shield", opts["eval_shields"])):
        if variants:
            metrics_history[key] = {
                name: evaluate(env, agent, num_episodes=10, exp_seed=exp_seed,
                               **({} if v is None else {view: v}))
                for name, v in variants.items()}
    _save_artifacts(artifacts_dir, checkpoint_dir, experiment_name, metrics_history,
                    training_episodes, episode_rewards, tracker.eval_episodes, tracker.rewards,
                    tracker.avg_rewards, target_reward, total_steps, logger, exp_prefix)
    return tracker.rewards, tracker.avg_rewards, metrics_history


def _controls_of(agent) -> dict:
    """The agent's KL target and lr schedule (None: not set), by option name."""
    return {k: getattr(agent, k, None) for k in CONTROL_KEYS}


def _new_metrics(experiment_name, values) -> dict:
    """metrics_history as a run starts it: the reference's keys, then what the given options of
    ``values`` (by name) add -- the default's metrics stay what they were."""
    return {"experiment_name": experiment_name, "episode_rewards": [], "eval_rewards": [],
            "avg_eval_rewards": [], "policy_updates": [], "episode_numbers": [],
            "eval_episode_numbers": [], "timestamps": [], **options.initial_metrics(values)}


def _book_episode(mh, episode_rewards, training_episodes, episode_num, ret, i, stats, safety,
                  logger, prefix, log_interval, total_steps, start_time) -> None:
    """One finished (or cut) episode into a run's records: its return and number, its row ``i``
    of the rollout's _stats_stream ``stats`` and _safety_stream ``safety`` (None: the run does
    not book them), and the log line."""
    episode_rewards.append(ret)
    training_episodes.append(episode_num)
    mh["episode_rewards"].append(ret)
    mh["episode_numbers"].append(episode_num)
    if stats is not None:
        _book_stats(mh, *stats, i)
    if safety is not None:
        _book_safety(mh, safety, i)
    _log_episode(logger, prefix, episode_num, ret, episode_rewards, log_interval, total_steps,
                 start_time)


def _log_episode(logger, prefix, episode_num, ep_reward, episode_rewards, log_interval,
                 total_steps, start_time):
    if episode_num % log_interval == 0:
        logger.info("%s episode=%d reward=%.2f avg_reward=%.2f steps=%d time=%.2fs", prefix,
                    episode_num, ep_reward, np.mean(episode_rewards[-log_interval:]), total_steps,
                    time.time() - start_time)


def _train_single(env, agent, max_episodes, log_interval, eval_interval, steps_per_update,
                  exp_seed, logger, prefix, mh, tracker, start_time):
    """The reference loop (routine.py:121-243) on the one-env facade."""
    episode_rewards, training_episodes = [], []
    total_steps = episode_num = 0
    done, flat_state = True, None
    while episode_num < max_episodes:
        steps_collected = 0
        t_update = time.time()
        while steps_collected < steps_per_update and episode_num < max_episodes:
            episode_num += 1
            state, _ = env.reset(seed=exp_seed + episode_num)
            flat_state = state.reshape(-1)
            ep_reward, done = 0.0, False
            while not done and steps_collected < steps_per_update:
                action, pre_tanh, log_prob, value = agent.select_action(flat_state)
                nxt, reward, terminated, truncated, _ = env.step(action)
                done = terminated or truncated
                flat_next = nxt.reshape(-1)
                agent.memory.store(flat_state, action, pre_tanh, reward, flat_next, log_prob, done, value)
                flat_state = flat_next
                ep_reward += reward
                steps_collected += 1
                total_steps += 1
            episode_rewards.append(ep_reward)
            training_episodes.append(episode_num)
            mh["episode_rewards"].append(ep_reward)
            mh["episode_numbers"].append(episode_num)
            _log_episode(logger, prefix, episode_num, ep_reward, episode_rewards, log_interval,
                         total_steps, start_time)
            if episode_num % eval_interval == 0:
                tracker.on_episode(episode_num)
        final_value = 0.0
        if not done:
            with torch.no_grad():
                _, _, v = agent.actor_critic.forward(flat_state)
                final_value = float(v.cpu().item())
        upd = agent.update(last_value=final_value)
        mh["policy_updates"].append({"episode": episode_num, "steps": steps_collected,
                                     "time": time.time() - t_update, **upd})
    return episode_rewards, training_episodes, total_steps


def _train_vector(env, agent, max_episodes, log_interval, eval_interval, steps_per_update,
                  exp_seed, logger, prefix, mh, tracker, start_time, episode_schedule="lockstep",
                  episode_stats=False, truncation="terminal", safety_stats=False, sensor=None,
                  shield=None, grid=None, lidar=None):
    """E lockstep envs, device rollout of T steps, batched PPO update.

    sensor / grid / lidar (at most one, the view): the rollout writes the rows the policy acts on
    with one env.view_into launch on the reset states and one after every env step
    (ppo/rollout.py); under a grid or a lidar the rollout buffer's states are ``spec.stride(F)``
    wide.

    shield: after the policy acted, the rollout's shield (one hwy_lookahead call per step,
    ppo/rollout.py) picks the action the env executes; PPO's stored actions, log-probs and values
    stay the policy's.  Every update's metrics carry ``shield_rate``, the share of the rollout's
    steps the shield overrode.

    safety_stats: the rollout issues one hwy_traffic launch per env step and every booked
    episode's reduction row goes to mh's SAFETY_KEYS lists (read before the next rollout).

    truncation "bootstrap": the rollout also stores V(final observation) of the truncated rows
    (ppo/rollout.py) and the update's GAE bootstraps them (hwy_gae_boot) instead of booking a
    time limit as terminal.

    episode_stats: the rollout steps with hwy_step_with_info and every booked episode's
    statistics go to mh's STATS_KEYS lists (read before the update and the next rollout).

    episode_schedule "reference": the rollout ends with the cut; its episode stream (finished,
    then cut episodes) is booked and its evaluations run before the update; the next rollout
    starts from the cut's first observations.

    With a process group on the agent (one rank per GPU, envs env_offset = rank*E of world*E),
    every rank steps its own E envs and joins the update's collectives; the episode stream is
    gathered so all ranks count the same episodes and stop after the same update, and rank 0
    alone evaluates and writes artifacts.  What the caller has already refused (a process group
    or another option an option does not go with) is ppo/options.py's table."""
    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout

    group = getattr(agent, "_dist", None)
    rank, world = _rank_world(group)
    bootstrap = truncation == "bootstrap"
    reference = episode_schedule == "reference"
    base = env.unwrapped
    E = base.num_envs
    view = options.given_view(dict(sensor=sensor, grid=grid, lidar=lidar))
    own = view is not None and view[1].REPLACES_ROWS  # the rollout writes states[0] itself
    sd = base.view_width(view[1]) if own else _flat_dim(env)
    T = max(1, math.ceil(steps_per_update / E))
    buf = RolloutBuffer(T, E, sd, 2, base.device, **options.given(
        episode_stats=episode_stats, safety_stats=safety_stats, truncation_bootstrap=bootstrap,
        shield=None if shield is None else True))
    base.set_seed_schedule(exp_seed)
    obs, _ = env.reset()
    if not own:
        buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, base, buf, use_graph=getattr(agent, "use_graphs", True),
                           **options.given(episode_schedule=episode_schedule,
                                           episode_stats=episode_stats, safety_stats=safety_stats,
                                           truncation=truncation, sensor=sensor, shield=shield,
                                           grid=grid, lidar=lidar))
    episode_rewards, training_episodes = [], []
    total_steps = episode_num = 0
    while episode_num < max_episodes:
        t_update = time.time()
        roll.run()
        total_steps += T * E * world
        stats = safety = None
        if episode_stats:
            stats = _stats_stream(buf.dones, buf.ep_length, buf.ep_stats, **(
                {"cut": roll.cut, "cut_length": roll.cut_length, "acc": buf.acc}
                if reference else {}))
        if safety_stats:
            safety = _safety_stream(buf.dones, buf.traffic_stats, roll.cut if reference else None)
        if reference:  # the stream's evaluations run below, ahead of the update (:173-175)
            stream = _episode_stream(buf.dones, buf.ep_return, roll.cut, roll.cut_return)
            upd = None
        else:
            upd = agent.update_rollout(buf, agent.value(buf.states[T]))
            # episode bookkeeping, in (step, global env) order -- identical on every rank
            stream = _episode_ends(buf.dones, buf.ep_return, group)
        for i, r in enumerate(stream):
            if episode_num >= max_episodes:
                break
            episode_num += 1
            _book_episode(mh, episode_rewards, training_episodes, episode_num, float(r), i, stats,
                          safety, logger, prefix, log_interval, total_steps, start_time)
            if episode_num % eval_interval == 0 and rank == 0:
                tracker.on_episode(episode_num)
        if reference:
            upd = agent.update_rollout(buf, agent.value(buf.states[T]))
        if shield is not None:  # the share of this rollout's steps the shield overrode
            upd = dict(upd, shield_rate=float((buf.chosen != 0).float().mean().item()))
        mh["policy_updates"].append({"episode": episode_num, "steps": T * E * world,
                                     "time": time.time() - t_update, **upd})
        roll.start_next()
    return episode_rewards, training_episodes, total_steps


def train_group(group, experiment_names, exp_seeds, max_episodes=500, target_reward=0.0,
                log_interval=20, eval_interval=50, loggers=None, episode_schedule="lockstep",
                episode_stats=False, safety_stats=False):
    """train_with_experiment_name for every experiment of an ExperimentGroup (ppo/group.py) at
    once: one grouped rollout + update per iteration, then each experiment's bookkeeping exactly
    as _train_vector does it on its own [T, E] slice (episode stream in (step, env) order,
    evaluation every ``eval_interval`` episodes on its own eval envs, best / solved checkpoints,
    artifacts).  An experiment that reaches ``max_episodes`` stops where its solo run stops; the
    group keeps stepping it (its later state is never read) until every experiment is done.
    Returns, per experiment, the reference's (rewards, avg_rewards, metrics_history), each equal
    to its solo run's: the group's experiments are bit-identical to solo runs
    (tests/test_group_gpu.py) and evaluation draws no random numbers."""
    return train_batch(group, [group], experiment_names, exp_seeds, max_episodes=max_episodes,
                       target_reward=target_reward, log_interval=log_interval,
                       eval_interval=eval_interval, loggers=loggers,
                       episode_schedule=episode_schedule,
                       **options.given(episode_stats=episode_stats, safety_stats=safety_stats))


def train_batch(stepper, groups, experiment_names, exp_seeds, max_episodes=500, target_reward=0.0,
                log_interval=20, eval_interval=50, loggers=None, episode_schedule="lockstep",
                episode_stats=False, safety_stats=False):
    """train_group over the experiments of several ExperimentGroups stepped together: `stepper`
    is the ExperimentGroup itself (groups = [it]) or a GroupBatch over `groups` (ppo/group.py:
    the cells of one hidden width in one set of launches).  experiment_names / exp_seeds /
    loggers list every group's experiments in group order; each experiment's bookkeeping is its
    solo run's, on its own [T, E] slice of its group's rollout.  episode_schedule "reference"
    (the groups must have been built with it): each experiment's stream is its finished then
    its cut episodes, and the due evaluations run, still as one evaluate_many, ahead of the
    update.  episode_stats (the groups must have been built with it): each experiment's
    per-episode statistics are booked beside its returns, as _train_vector books them.
    safety_stats (likewise): each experiment's hwy_traffic reduction rows, from its own slice of
    its group's traffic_stats."""
    if any(bool(getattr(g, "safety_stats", False)) != bool(safety_stats) for g in groups):
        raise ValueError(f"train_batch: every group must be built with safety_stats="
                         f"{bool(safety_stats)}")
    if safety_stats and any(getattr(a, "_dist", None) is not None
                            for g in groups for a in g.agents):
        raise ValueError("safety_stats does not run over a process group")

    if any(bool(getattr(g, "episode_stats", False)) != bool(episode_stats) for g in groups):
        raise ValueError(f"train_batch: every group must be built with episode_stats="
                         f"{bool(episode_stats)}")

    reference = options.BY_NAME["episode_schedule"].normalise(episode_schedule) == "reference"
    if any(getattr(g, "episode_schedule", "lockstep") != episode_schedule for g in groups):
        raise ValueError(f"train_batch: every group must be built with episode_schedule="
                         f"{episode_schedule!r}")
    if reference and any(getattr(a, "_dist", None) is not None for g in groups for a in g.agents):
        raise ValueError("episode_schedule='reference' does not run over a process group")
    members = [(g, j) for g in groups for j in range(g.G)]
    if len(experiment_names) != len(members) or len(exp_seeds) != len(members):
        raise ValueError(f"train_batch: {len(members)} experiments, "
                         f"{len(experiment_names)} names, {len(exp_seeds)} seeds")
    artifacts_dir = ensure_artifacts_dir()
    checkpoint_dir = os.path.join(artifacts_dir, "checkpoints")
    os.makedirs(checkpoint_dir, exist_ok=True)
    start_time = time.time()
    runs = []
    for k, (grp, j) in enumerate(members):
        name = experiment_names[k]
        logger = loggers[k] if loggers else setup_experiment_logger(name)
        prefix = f"[{name}]" if name else ""
        logger.info(f"{prefix} Starting training for experiment: {name} (group of {grp.G}, "
                    f"batch of {len(members)})")
        mh = _new_metrics(name, dict(episode_stats=episode_stats, safety_stats=safety_stats,
                                     **_controls_of(grp.agents[j])))
        tracker = _EvalTracker(grp.solo_envs[j], grp.agents[j], int(exp_seeds[k]),
                               target_reward, checkpoint_dir, name, mh, logger, prefix, start_time)
        logger.info(f"{prefix} Performing initial evaluation...")
        runs.append({"name": name, "logger": logger, "prefix": prefix, "mh": mh,
                     "tracker": tracker, "episode_rewards": [], "training_episodes": [],
                     "episode_num": 0, "total_steps": 0, "done": max_episodes <= 0,
                     "group": grp, "j": j, "pending": []})
    # every experiment's evaluations run together (evaluate_many: the same results as one
    # evaluate each -- deterministic episodes, no random numbers drawn)
    first = evaluate_many([(r["tracker"].env, r["tracker"].agent, r["tracker"].exp_seed)
                           for r in runs])
    for r, v in zip(runs, first):
        r["tracker"].initial(v)
    while not all(r["done"] for r in runs):
        t_update = time.time()
        stepper.rollout()
        if not reference:
            upds = _flat_updates(stepper, groups)
        for k, r in enumerate(runs):
            if r["done"]:
                continue
            grp, j = r["group"], r["j"]
            E, T = grp.E, grp.T
            r["total_steps"] += T * E
            sl = slice(j * E, (j + 1) * E)
            if reference:
                stream = _episode_stream(grp.buf.dones[:, sl], grp.buf.ep_return[:, sl],
                                         grp.cut[sl], grp.cut_return[sl])
            else:
                stream = _episode_ends(grp.buf.dones[:, sl], grp.buf.ep_return[:, sl])
            stats = safety = None
            if episode_stats:
                cut_kw = ({"cut": grp.cut[sl], "cut_length": grp.cut_length[sl],
                           "acc": grp.buf.acc[sl]} if reference else {})
                stats = _stats_stream(grp.buf.dones[:, sl], grp.buf.ep_length[:, sl],
                                      grp.buf.ep_stats[:, sl], **cut_kw)
            if safety_stats:
                safety = _safety_stream(grp.buf.dones[:, sl], grp.buf.traffic_stats[:, sl],
                                        grp.cut[sl] if reference else None)
            for i, ret in enumerate(stream):
                if r["episode_num"] >= max_episodes:
                    break
                r["episode_num"] += 1
                _book_episode(r["mh"], r["episode_rewards"], r["training_episodes"],
                              r["episode_num"], float(ret), i, stats, safety, r["logger"],
                              r["prefix"], log_interval, r["total_steps"], start_time)
                if r["episode_num"] % eval_interval == 0:
                    r["pending"].append(r["episode_num"])
            if reference:
                r["booked"] = True
                continue
            r["mh"]["policy_updates"].append({"episode": r["episode_num"], "steps": T * E,
                                              "time": time.time() - t_update, **upds[k]})
            if r["episode_num"] >= max_episodes:
                r["done"] = True
        # this iteration's evaluations (weights unchanged since its update -- on the reference
        # schedule since the previous one: they run ahead of this iteration's): one per
        # experiment that crossed an evaluation point, all together; a second point in the same
        # iteration evaluates the same weights and gets the same (memoised) value
        due = [r for r in runs if r["pending"]]
        if due:
            vals = evaluate_many([(r["tracker"].env, r["tracker"].agent, r["tracker"].exp_seed)
                                  for r in due])
            for r, v in zip(due, vals):
                for ep in r["pending"]:
                    r["tracker"].on_episode(ep, v)
                r["pending"] = []
        if reference:
            upds = _flat_updates(stepper, groups)
            for r, upd in zip(runs, upds):
                if not r.pop("booked", False):
                    continue
                r["mh"]["policy_updates"].append({"episode": r["episode_num"],
                                                  "steps": r["group"].T * r["group"].E,
                                                  "time": time.time() - t_update, **upd})
                if r["episode_num"] >= max_episodes:
                    r["done"] = True
    out = []
    for r in runs:
        tr = r["tracker"]
        _save_artifacts(artifacts_dir, checkpoint_dir, r["name"], r["mh"], r["training_episodes"],
                        r["episode_rewards"], tr.eval_episodes, tr.rewards, tr.avg_rewards,
                        target_reward, r["total_steps"], r["logger"], r["prefix"])
        out.append((tr.rewards, tr.avg_rewards, r["mh"]))
    return out


def _flat_updates(stepper, groups):
    """stepper.update's metrics, one per experiment in group order."""
    upds = stepper.update(return_metrics=True)
    if len(groups) > 1 or stepper is not groups[0]:  # a GroupBatch: one list per group
        upds = [m for per_group in upds for m in per_group]
    return upds


def _rank_world(group):
    if group is None:
        return 0, 1
    return torch.distributed.get_rank(group), torch.distributed.get_world_size(group)


def _episode_ends(dones, rets, group=None):
    """Returns of the episodes that ended in a [T, E] rollout, in (step, env) order.

    Over a process group each rank's [T, E] slice is all-gathered and laid side by side, so
    every rank sees the [T, world*E] stream one process stepping all world*E envs (rank r's at
    r*E..) would, and counts the same episodes in the same order."""
    pack = torch.stack([dones.to(torch.float64), rets.to(torch.float64)])
    if group is not None:
        if torch.distributed.get_backend(group) == "gloo":
            pack = pack.cpu()
        parts = [torch.empty_like(pack) for _ in range(torch.distributed.get_world_size(group))]
        torch.distributed.all_gather(parts, pack.contiguous(), group=group)
        pack = torch.cat(parts, dim=2)
    pack = pack.cpu().numpy()
    return pack[1][pack[0] != 0]


def _episode_stream(dones, rets, cut, cut_rets):
    """The reference schedule's episode stream of one rollout: the returns of the episodes that
    finished in the [T, E] rollout, in (step, env) order (_episode_ends), then those of the
    episodes cut at its end (cut [E] nonzero), in env order, each with its partial return
    (reference training/routine.py:153-156 books the unfinished episode like any other)."""
    ends = _episode_ends(dones, rets)
    pack = torch.stack([cut.to(torch.float64), cut_rets.to(torch.float64)]).cpu().numpy()
    return np.concatenate([ends, pack[1][pack[0] != 0]])
