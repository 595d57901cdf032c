"""ExperimentGroup: G independent PPO experiments of one condition on one GPU, stepped together.

The reference runs a sweep as one process per experiment (experiments/runner.py:46-155 under
main.py:188-242's joblib / SLURM fan-out, utils/device_pool.py:44-72 oversubscribing each GPU
16x).  At the reference's own update statistics (E = 16 envs x T = 128 steps = 2,048 samples,
minibatches of 64) one experiment is far too small to fill an MI355X: every launch of its rollout
and update runs a handful of workgroups.  A group batches G such experiments -- a condition's
seeds -- into the launches themselves:

  * one env handle of G*E envs, experiment g owning envs [g*E, (g+1)*E) with its own episode
    seed schedule (hwy_set_seed_groups) and, for RankPE, its own rank table;
  * one acting launch per rollout step for all G policies (hwy_ppo_group_act);
  * one GAE launch over the [T, G*E] rollout;
  * per minibatch step four launches for all G learners (hwy_ppo_group_step), each learner
    reading its own minibatch through its own permutation mapped into the grouped rollout.

Every experiment keeps its own weights, Adam state, torch generator (sampling noise and the
minibatch permutation) and advantage normalisation, drawn in its solo run's order, and the
kernels run the solo calls' bodies per learner, so each experiment is bit for bit its solo run
(training/routine.py's _train_vector with the same seed): tests/test_group_gpu.py.

``episode_schedule="reference"`` cuts every experiment's running episodes at the update boundary
as ppo/rollout.py does for a solo run (hwy_cut_episodes on the group's handle, seed groups
included); with it one env per experiment (E = 1, T = steps_per_update) is the reference's own
stream.
"""

from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch

from utils.graphs import capture as graph_capture
from utils.graphs import run_or_replay as _graph_run
from utils.graphs import run_or_replay_chunks as _graph_run_chunks

from . import options
from .agent import RolloutBuffer
from .rollout import (alloc_cut_buffers, check_episode_schedule, rollout_chunks,
                      traffic_after_reset, traffic_after_step)


class ExperimentGroup:
    def __init__(self, agents: Sequence, env, seeds: Sequence[int], envs_per_experiment: int,
                 rollout_len: int, use_graphs: bool = True, rank_tables=None,
                 episode_schedule: str = "lockstep", episode_stats: bool = False,
                 safety_stats: bool = False):
        from hwy.ppo_native import GroupAct

        self.episode_schedule = check_episode_schedule(episode_schedule)
        # one hwy_traffic launch on the group's handle after every env step, every experiment's
        # per-episode reduction in buf.traffic_stats / buf.traffic_acc (ppo/rollout.py)
        self.safety_stats = bool(safety_stats)
        # the env steps as hwy_step_with_info, every experiment's episode sums in buf.ep_stats /
        # buf.acc (ppo/rollout.py)
        self.episode_stats = bool(episode_stats)

        self.agents = list(agents)
        self.G, self.E, self.T = len(self.agents), int(envs_per_experiment), int(rollout_len)
        self.env = env.unwrapped if hasattr(env, "unwrapped") else env
        if self.env.num_envs != self.G * self.E:
            raise ValueError(f"the group env needs {self.G} x {self.E} envs, has {self.env.num_envs}")
        if len(seeds) != self.G:
            raise ValueError("one seed per experiment")
        a0 = self.agents[0]
        dims = {(ag.actor_critic.shared[0].weight.shape, ag.epochs, ag.batch_size,
                 ag.num_minibatches) for ag in self.agents}
        if len(dims) != 1 or any(ag.device != a0.device for ag in self.agents):
            raise ValueError("a group's experiments share learner dims, epochs, batch size, device")
        self.dev = a0.device
        self.seeds = [int(s) for s in seeds]
        # per-experiment episode seed schedules: group g as a solo handle of E envs seeded with
        # set_seed_schedule(seeds[g]) (training/routine.py:_train_vector)
        self.env.set_seed_groups(self.seeds, self.E)
        if rank_tables is not None:
            import numpy as np

            self.env.set_pe_table(np.concatenate([np.asarray(t, np.float32).reshape(-1)
                                                  for t in rank_tables]))
        N, Fo = self.env.obs_rows, self.env.obs_features
        self.sd = N * Fo
        self.buf = RolloutBuffer(self.T, self.G * self.E, self.sd, 2, self.dev, **options.given(
            episode_stats=self.episode_stats, safety_stats=self.safety_stats))
        self.use_graphs = bool(use_graphs)
        self.act = GroupAct(self.agents, self.E)
        GE = self.G * self.E
        # the bootstrap value row's outputs (deterministic act on states[T]); fixed buffers, so
        # their argument tables are prepared once
        self._boot = tuple(torch.empty(*s, device=self.dev) for s in ((GE, 2), (GE, 2), (GE,), (GE,)))
        self._noise_tmp = torch.empty(self.T, self.E, 2, device=self.dev)
        self._roll_graph = None
        self._roll_key = None
        self._roll_seen = None
        self._roll_chunks = None  # reference schedule, long rollout: (graph, key, seen) per chunk
        if self.episode_schedule == "reference":
            alloc_cut_buffers(self, GE, self.sd, self.dev)
        self._upd = None  # the update's static inputs and argument structs (pre_update)
        self.iterations = 0
        # how the rollouts / updates were issued (graph replays vs eager runs vs captures, and
        # argument-table preparations): a sweep that keeps re-preparing shows here
        self.stats = {"rollout_replay": 0, "rollout_eager": 0, "rollout_capture": 0,
                      "update_prepare": 0, "update_capture": 0}
        obs, _ = self.env.reset()
        self.buf.states[0].copy_(obs.reshape(GE, self.sd))
        if self.safety_stats:
            traffic_after_reset(self.env, self.buf)

    # ------------------------------------------------------------------ rollout
    def _draw_noise(self) -> None:
        """Each experiment's T x E x 2 sampling noise from its own generator, exactly as its
        solo RolloutBuffer.draw_noise draws it."""
        buf, E = self.buf, self.E
        for g, ag in enumerate(self.agents):
            torch.randn(self._noise_tmp.shape, generator=ag.generator, device=self.dev,
                        out=self._noise_tmp)
            buf.noise[:, g * E:(g + 1) * E].copy_(self._noise_tmp)

    def act_rows(self, t: int, deterministic: bool = False):
        """This group's acting rows at rollout step t (GroupAct.rows_of), or, deterministic, the
        bootstrap row states[T] into the fixed bootstrap outputs."""
        buf = self.buf
        if deterministic:
            return self.act.rows_of(buf.states[self.T], self._boot, None)
        return self.act.rows_of(buf.states[t], (buf.actions[t], buf.pre_tanh[t], buf.log_probs[t],
                                                buf.values[t]), buf.noise[t])

    def env_io(self, t: int):
        """step_into's buffers for rollout step t (hwy_step's arguments)."""
        buf, env = self.buf, self.env
        obs_shape = env.obs_buf.shape[1:]
        return (buf.actions[t], buf.states[t + 1].view(self.G * self.E, *obs_shape),
                buf.rewards[t], buf.terminated[t], buf.truncated[t], buf.ep_return[t],
                buf.ep_length[t])

    def env_step(self, t: int) -> None:
        self.env.step_into(*self.env_io(t), info=self.buf.step_info(t))

    def env_traffic(self, t: int) -> None:
        """safety_stats: hwy_traffic on the states step t left (LockstepRollout._steps: on the
        reference schedule the last step's launch follows the cut)."""
        if self.safety_stats and not (self.episode_schedule == "reference" and t == self.T - 1):
            traffic_after_step(self.env, self.buf, t)

    def cut_episodes(self) -> None:
        """The reference schedule's cut after the rollout's last step (LockstepRollout._steps)."""
        obs_shape = self.env.obs_buf.shape[1:]
        self.next0.copy_(self.buf.states[self.T])
        self.env.cut_episodes(self.next0.view(self.G * self.E, *obs_shape), self.cut_return,
                              self.cut_length, self.cut)
        if self.safety_stats:
            traffic_after_step(self.env, self.buf, self.T - 1, cut=self.cut)

    def finish_rollout(self) -> None:
        self.buf.finish_dones()
        if self.episode_schedule == "reference":
            self.cut_episodes()

    def _steps(self, tiles, t0: int = 0, t1: Optional[int] = None) -> None:
        t1 = self.T if t1 is None else t1
        for t in range(t0, t1):
            self.act.launch(self.act_rows(t), tiles)
            self.env_step(t)
            self.env_traffic(t)
        if t1 == self.T:
            self.finish_rollout()

    def rollout(self) -> None:
        """T steps of every experiment (LockstepRollout's order: act, then env step, per t);
        captured as one HIP graph once its launch arguments repeat (a long reference-schedule
        rollout: one graph per chunk of steps, ppo/rollout.py rollout_chunks)."""
        self._draw_noise()
        tiles = self.act.tiles()  # also syncs acting-only tile images, outside any capture
        key = (self.env._handle.value, self.env.launch_version, tuple(tiles), _flat_ptrs(self.agents))
        chunks = rollout_chunks(self.T, self.episode_schedule)
        if len(chunks) > 1:
            self._roll_chunks = _graph_run_chunks(self, self.use_graphs, key, chunks,
                                                  lambda t0, t1: self._steps(tiles, t0, t1),
                                                  self._roll_chunks)
            return
        self._roll_graph, self._roll_key, self._roll_seen = _graph_run(
            self, self.use_graphs, key, lambda: self._steps(tiles), self._roll_graph,
            self._roll_key, self._roll_seen, "rollout")

    # ------------------------------------------------------------------ update
    def bootstrap_values(self) -> torch.Tensor:
        """V(states[T]) of every experiment (PPOAgent.value: the deterministic act launch)."""
        self.act.launch(self.act_rows(0, deterministic=True))
        return self._boot[3]

    def pre_update(self, last_values: torch.Tensor) -> dict:
        """The update's inputs for every experiment, in its solo update_rollout's order on its
        generator and samples (ppo/agent.py's batched update): GAE over the [T, G*E] rollout,
        each experiment's advantage normalisation and permutation mapped into the grouped
        rollout, the learners' FusedPPO (its Adam state handed over) with its per-update
        refresh (counters, tile image).  Returns the context post_update and the step runner
        use; ctx["args"][g][i] is learner g's PpoArgs of minibatch i, rebuilt only when the
        buffers or hyper-parameters change (ctx["key"]); ctx["mb"], ctx["nmb"] and ctx["epochs"]
        are the cell's schedule (minibatch rows, minibatches per epoch, epochs)."""
        from hwy import ops

        buf, G, E, T = self.buf, self.G, self.E, self.T
        n, GE = T * E, G * E
        adv, ret = ops.gae(buf.rewards, buf.dones, buf.values, last_values,
                           self.agents[0].gamma, self.agents[0].lam)
        sizes = self.agents[0].minibatch_sizes(n)
        mb, nmb = sizes[0], len(sizes)
        if len(set(sizes)) != 1:
            raise ValueError(f"grouped update needs equal minibatches, got {sorted(set(sizes))}")
        fused = []
        for ag in self.agents:
            if not ag._fused_ok(mb):
                raise ValueError("grouped update needs the fused HIP learner (backend hip/auto)")
            F = ag._fused_for(mb, nmb, n)
            ag._adam_to("fused")
            fused.append(F)
        fkey = (tuple(id(F) for F in fused), mb, nmb)
        if self._upd is None or self._upd[0] != fkey:
            # static inputs of the captured steps (FusedPPO's _static_bufs): advantages,
            # returns and the mapped permutations are copied in every update
            self._upd = [fkey, torch.empty(T * GE, device=self.dev),
                         torch.empty(T * GE, device=self.dev),
                         torch.empty(G, n, dtype=torch.int64, device=self.dev),
                         torch.empty(G, n, dtype=torch.int64, device=self.dev), None, None]
        _, adv_grp, ret_flat, idx_all, perms, bound, args = self._upd
        adv3 = adv_grp.view(T, G, E)
        for g, ag in enumerate(self.agents):
            # contiguous, as the solo run's [T, E] advantages are: with E = 1 the slice's
            # reshape is a strided view, whose mean / std torch reduces in another order
            a = ag.normalize_advantages(adv[:, g * E:(g + 1) * E].contiguous().reshape(n))
            adv3[:, g].copy_(a.view(T, E))
            torch.randperm(n, device=self.dev, generator=ag.generator, out=perms[g])
        # sample (t, l) of experiment g sits at t*G*E + g*E + l of the grouped rollout
        offs = torch.arange(G, device=self.dev, dtype=torch.int64).mul_(E).view(G, 1)
        torch.add(torch.div(perms, E, rounding_mode="floor") * GE + offs, perms % E, out=idx_all)
        states = buf.states[:T].reshape(T * GE, -1)
        pre = buf.pre_tanh.reshape(T * GE, -1)
        old_lp = buf.log_probs.reshape(T * GE)
        ret_flat.copy_(ret.reshape(T * GE))
        key = (states.data_ptr(), pre.data_ptr(), old_lp.data_ptr(), adv_grp.data_ptr(),
               ret_flat.data_ptr(), idx_all.data_ptr()) + tuple(F._scalar_key() for F in fused)
        if bound != key:
            args = [[F._args(states, pre, old_lp, adv_grp, ret_flat,
                             idx_all[g].data_ptr() + i * mb * 8) for i in range(nmb)]
                    for g, F in enumerate(fused)]
            self._upd[5], self._upd[6] = key, args
        for F, a in zip(fused, args):
            F._last_args, F._last_inputs = a, (states, pre, old_lp, adv_grp, ret_flat, idx_all)
            F.counters[1].zero_()
            F.sync_params(a[0])  # FusedPPO.run's tile-image refresh
        return {"fused": fused, "args": args, "key": key, "sizes": sizes, "mb": mb, "nmb": nmb,
                "epochs": self.agents[0].epochs, "ret": ret}

    def post_update(self, ctx: dict, return_metrics=True):
        buf, E, T = self.buf, self.E, self.T
        n = T * E
        out = []
        for g, (ag, F) in enumerate(zip(self.agents, ctx["fused"])):
            F._tiles_version = F._param_versions()
            ag.updates += 1
            if return_metrics:
                vals = buf.values[:, g * E:(g + 1) * E].contiguous().reshape(n)
                rets = ctx["ret"][:, g * E:(g + 1) * E].contiguous().reshape(n)
                ctl = None
                if ag.controlled:  # a KL target / lr schedule: the applied rows only
                    ctl = ag._fused_ctl(F, ctx["step"], ctx.get("first", 0) + g)
                out.append(ag._finish_metrics(F.metrics, ctx["sizes"], vals, rets,
                                              deferred=return_metrics == "deferred", ctl=ctl))
        self.iterations += 1
        buf.states[0].copy_(self.next0 if self.episode_schedule == "reference" else buf.states[T])
        return out if return_metrics else None

    def update(self, return_metrics: bool = True):
        """PPOAgent.update_rollout for every experiment at once: pre_update, epochs x
        minibatches of the grouped fused step (one graph per epoch), post_update."""
        ctx = self.pre_update(self.bootstrap_values())
        self._steps_runner = _run_group_steps(self, [ctx], getattr(self, "_steps_runner", None))
        return self.post_update(ctx, return_metrics)

    def iteration(self, return_metrics=True):
        """One PPO iteration of every experiment: rollout, then update."""
        self.rollout()
        return self.update(return_metrics)

    def close(self) -> None:
        """Release the grouped env handle and the experiments' own (evaluation template) envs."""
        for e in getattr(self, "solo_envs", []) + [getattr(self, "group_env", self.env)]:
            try:
                e.close()
            except Exception:
                pass

    def episode_returns(self, g: int) -> torch.Tensor:
        """Returns of experiment g's episodes that ended in the last rollout, in (step, env)
        order (training/routine.py:_episode_ends on its [T, E] slice)."""
        E = self.E
        d = self.buf.dones[:, g * E:(g + 1) * E]
        r = self.buf.ep_return[:, g * E:(g + 1) * E]
        return r[d != 0]

    def cut_episode_returns(self, g: int):
        """(cut, partial return) of experiment g's envs after the last reference-schedule
        rollout, in env order."""
        E = self.E
        return self.cut[g * E:(g + 1) * E], self.cut_return[g * E:(g + 1) * E]


def _flat_ptrs(agents) -> tuple:
    """The agents' flat-parameter addresses: part of a rollout graph's key, as of
    LockstepRollout._launch_key -- the acting table keys on them, so a graph captured before
    flat_params rebuilt an agent's buffer would replay a table that points at the old weights."""
    from hwy.ppo_native import flat_params

    return tuple(flat_params(ag)[0].data_ptr() for ag in agents)


def update_schedule(nmbs: Sequence[int], epochs: Sequence[int]):
    """(max_steps, period) of one update of learners stepped together, learner y running
    steps[y] = epochs[y] * nmbs[y] grouped steps: the update takes max(steps) slots, and every
    learner ends on a multiple of period = gcd(steps) (hwy_ppo_sched_plan)."""
    import math

    steps = [int(e) * int(n) for n, e in zip(nmbs, epochs)]
    if not steps or min(steps) < 1:
        raise ValueError("a schedule needs nmb >= 1 and epochs >= 1 for every learner")
    return max(steps), math.gcd(*steps)


def slot_minibatch(slot: int, nmb: int, epochs: int) -> Optional[int]:
    """The minibatch a learner of `nmb` minibatches and `epochs` epochs runs in slot `slot` of
    an update (epoch-major, minibatch-minor: FusedPPO.run's order), or None once it is done."""
    return slot % nmb if 0 <= slot < nmb * epochs else None


def graph_slots(period: int, cap: int = 256) -> int:
    """Slots of the captured update graph: the schedule's period, or, past `cap` slots, its
    largest divisor below the cap (any length works -- the kernels add the table's slot base --
    and a divisor keeps every learner's end on a replay boundary)."""
    return max(d for d in range(1, min(period, cap) + 1) if period % d == 0)


def _capture_steps(owner, steps):
    """`steps()` captured as one graph on a stream of its own (FusedPPO._capture)."""
    owner.stats["update_capture"] += 1
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        with graph_capture(graph, stream=s):
            steps()
    torch.cuda.current_stream().wait_stream(s)
    return graph


def _run_group_steps(owner, ctxs, runner):
    """Every epoch's minibatch steps of the learners of `ctxs` (pre_update contexts) as grouped
    launches: one GroupStep over all of them, its tables prepared when any member's arguments
    changed.  Cells that share minibatch rows, minibatch count and epochs: one epoch captured as
    a graph and replayed `epochs` times (FusedPPO.run's schedule).  Cells whose schedules differ
    (GroupStep.sched): one table holding every learner's schedule, graph_slots(period) slots
    plus the slot-base advance captured as one graph and replayed until the longest learner is
    done; a learner that is done sits the remaining slots out.  runner = (key, GroupStep, graph)
    kept by the owner between updates."""
    from hwy.ppo_native import GroupStep

    fused = [F for c in ctxs for F in c["fused"]]
    args = [a for c in ctxs for a in c["args"]]
    sched = tuple((c["mb"], c["nmb"], c["epochs"]) for c in ctxs)
    key = (tuple(id(F) for F in fused), sched) + tuple(c["key"] for c in ctxs)
    if runner is None or runner[0] != key:
        owner.stats["update_prepare"] += 1
        step = GroupStep(fused)
        step.prepare(args)
        runner = (key, step, None)
    _, step, graph = runner
    first = 0
    for c in ctxs:  # post_update reads the KL stops of learners first .. first + G from it
        c["step"], c["first"] = step, first
        first += len(c["fused"])
    if step.sched:
        step.apply_lr()  # lr schedules: this update's rates, device to device (not captured)
        want = update_schedule([c["nmb"] for c in ctxs], [c["epochs"] for c in ctxs])
        if (step.max_steps, step.period) != want:
            raise RuntimeError(f"scheduled step: the table's schedule {step.max_steps, step.period} "
                               f"is not the cells' {want}")
        if not owner.use_graphs:
            step.begin()
            for s in range(step.max_steps):
                step.step(s)
            return runner
        P = graph_slots(step.period)
        if graph is None:
            def slots():
                for s in range(P):
                    step.step(s)
                step.advance(P)

            graph = _capture_steps(owner, slots)
            runner = (key, step, graph)
        step.begin()
        for _ in range(-(-step.max_steps // P)):
            graph.replay()
        return runner
    nmb, epochs = ctxs[0]["nmb"], ctxs[0]["epochs"]
    if not owner.use_graphs:
        for _ in range(epochs):
            for i in range(nmb):
                step.step(i)
        return runner
    if graph is None:  # one epoch's minibatch steps as one graph (FusedPPO._capture)
        graph = _capture_steps(owner, lambda: [step.step(i) for i in range(nmb)])
        runner = (key, step, graph)
    for _ in range(epochs):
        graph.replay()
    return runner


class GroupBatch:
    """Several ExperimentGroups -- a sweep's cells, which may differ in observation layout
    (state dims 60 or 120: no PE, RoPE, DistPE, RankPE), in hidden width (h128, h256, h384, ...)
    and in batch_size / num_minibatches / epochs -- stepped as ONE set of launches: per rollout step the
    acting launch for every learner of every group and one env launch for every group's handle
    (hwy_step_group); per minibatch step one grouped fused step over all their learners.  Groups
    of one hidden width take hwy_ppo_group_act / hwy_ppo_group_step (one acting launch, four per
    step); groups of different widths take hwy_ppo_mixed_act / hwy_ppo_mixed_step, which add one
    acting and one row launch when the widths span both wave-count classes (include/hwy_ppo.h).
    Groups whose minibatch rows, minibatch count or epochs differ take hwy_ppo_sched_step: the
    update runs max(epochs x minibatches) grouped steps, each learner on its own minibatch index
    and sitting the rest out once its epochs are done (_run_group_steps).  The groups still share
    envs per experiment and rollout length.  Each experiment stays bit-identical to its solo run: the same kernel bodies per
    learner, each group's own generator order, GAE and normalisation."""

    def __init__(self, groups, use_graphs: bool = True, episode_stats: Optional[bool] = None):
        from hwy.ppo_native import GroupAct

        self.groups = list(groups)
        g0 = self.groups[0]
        # the groups' steps as one hwy_step_group_info launch; the groups are built with the flag
        self.episode_stats = g0.episode_stats if episode_stats is None else bool(episode_stats)
        if any(g.episode_stats != self.episode_stats for g in self.groups):
            raise ValueError("a batch's groups share episode_stats")
        # one hwy_traffic launch per handle and step (a grouped launch does not exist)
        self.safety_stats = g0.safety_stats
        if any(g.safety_stats != self.safety_stats for g in self.groups):
            raise ValueError("a batch's groups share safety_stats")
        if any(g.E != g0.E or g.T != g0.T for g in self.groups):
            raise ValueError("a batch's groups share envs per experiment and rollout length")
        if any(g.episode_schedule != g0.episode_schedule for g in self.groups):
            raise ValueError("a batch's groups share the episode schedule")
        self.episode_schedule = g0.episode_schedule
        self.agents = [a for g in self.groups for a in g.agents]
        self.act = GroupAct(self.agents, g0.E)
        # the groups' env steps as one launch (hwy_step_group): each group's handle alone holds
        # G x E envs -- one wave each, a small part of the GPU -- so n launches in a row would
        # leave most of it idle
        from hwy.vec_env import GroupEnvStep

        self.envstep = GroupEnvStep([g.env for g in self.groups]) if len(self.groups) > 1 else None
        self.use_graphs = bool(use_graphs)
        self.T = g0.T
        self._roll = (None, None, None)
        self._roll_chunks = None
        self._runner = None
        self.stats = {"rollout_replay": 0, "rollout_eager": 0, "rollout_capture": 0,
                      "update_prepare": 0, "update_capture": 0}

    @property
    def launches_per_step(self):
        """Launches of one minibatch step over all the learners (GroupStep.launches_per_step);
        None before the first update."""
        return None if self._runner is None else self._runner[1].launches_per_step

    def _rows(self, t, deterministic=False):
        return [r for g in self.groups for r in g.act_rows(t, deterministic)]

    def _steps(self, tiles, t0=0, t1=None):
        t1 = self.T if t1 is None else t1
        for t in range(t0, t1):
            self.act.launch(self._rows(t), tiles)
            if self.envstep is not None:
                self.envstep.launch([g.env_io(t) for g in self.groups],
                                    infos=([g.buf.step_info(t) for g in self.groups]
                                           if self.episode_stats else None))
            else:
                self.groups[0].env_step(t)
            for g in self.groups:
                g.env_traffic(t)
        if t1 == self.T:
            for g in self.groups:
                g.finish_rollout()  # the reference schedule's cut: once per handle

    def rollout(self) -> None:
        for g in self.groups:
            g._draw_noise()
        tiles = self.act.tiles()
        key = (tuple((g.env._handle.value, g.env.launch_version) for g in self.groups),
               tuple(tiles), _flat_ptrs(self.agents))
        chunks = rollout_chunks(self.T, self.episode_schedule)
        if len(chunks) > 1:
            self._roll_chunks = _graph_run_chunks(self, self.use_graphs, key, chunks,
                                                  lambda t0, t1: self._steps(tiles, t0, t1),
                                                  self._roll_chunks)
            return
        self._roll = _graph_run(self, self.use_graphs, key, lambda: self._steps(tiles), *self._roll,
                                "rollout")

    def update(self, return_metrics=True):
        self.act.launch(self._rows(0, deterministic=True))  # every group's bootstrap values
        ctxs = [g.pre_update(g._boot[3]) for g in self.groups]
        self._runner = _run_group_steps(self, ctxs, self._runner)
        return [g.post_update(c, return_metrics) for g, c in zip(self.groups, ctxs)]

    def iteration(self, return_metrics=True):
        """One PPO iteration of every experiment of every group: a list per group."""
        self.rollout()
        return self.update(return_metrics)


def build_group(condition, base_config, seeds: Sequence[int], envs_per_experiment: int,
                rollout_len: int, device: torch.device, make_agent: Callable, d_embed=None,
                env_overrides: Optional[dict] = None, use_graphs: bool = True,
                episode_schedule: str = "lockstep", episode_stats: bool = False,
                safety_stats: bool = False):
    """A group of len(seeds) experiments of one condition, each constructed as
    experiments/runner.py constructs its solo run: set_random_seeds(seed), make_env (whose RankPE
    table draws from the global torch RNG), env.to(device), then ``make_agent(state_dim)`` (the
    PPOAgent, its weights drawn from the global RNG, its generator seeded from it), so every
    experiment's weights, rank table and generator are its solo run's.  The experiments' own
    E-env handles are kept as ``group.solo_envs`` (templates of their evaluation envs)."""
    import copy

    from experiments.wrappers import make_env
    from hwy.ops import PE_RANK
    from utils.reproducibility import set_random_seeds

    E = int(envs_per_experiment)
    ov = copy.deepcopy(env_overrides or {})
    if episode_schedule == "reference":
        ov.setdefault("vector_env", True)  # E = 1 too: the reference's one-env stream
    agents, tables, solos = [], [], []
    for s in seeds:
        set_random_seeds(int(s))
        solo = make_env(condition, base_config, d_embed=d_embed,
                        env_overrides=dict(copy.deepcopy(ov), num_envs=E, device=device,
                                           autoreset=True))
        if hasattr(solo, "to") and callable(solo.to):
            solo = solo.to(device)
        base = solo.unwrapped
        t = getattr(base, "_pe_table", None)
        tables.append(None if t is None else t.copy())
        agents.append(make_agent(base.obs_rows * base.obs_features))
        solos.append(solo)
    env = make_env(condition, base_config, d_embed=d_embed,
                   env_overrides=dict(copy.deepcopy(ov), num_envs=len(seeds) * E, device=device,
                                      autoreset=True))
    if hasattr(env, "to") and callable(env.to):
        env = env.to(device)
    rank = env.unwrapped.hwy_config.pe_kind == PE_RANK and tables[0] is not None
    grp = ExperimentGroup(agents, env, seeds, E, rollout_len, use_graphs=use_graphs,
                          rank_tables=tables if rank else None,
                          **options.given(episode_schedule=episode_schedule,
                                          episode_stats=episode_stats, safety_stats=safety_stats))
    grp.solo_envs = solos
    grp.group_env = env
    return grp
