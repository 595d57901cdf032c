"""PPO actor-critic for the MI355X build.

API-compatible with the reference's ppo/agent.py:
  * ActorCritic (:12-84): same module tree and parameter names (``shared.{0,2}``,
    ``actor_mean.{0,2}``, ``log_std``, ``critic.{0,2}``) so checkpoints load both ways;
    tanh-squashed Gaussian with the ``log1p(-a^2 + 1e-6)`` correction and the pre-tanh entropy.
  * PPOMemory (:87-154): list memory with store / clear / compute_advantages / get_batches /
    get_tensors; GAE runs in the HIP kernel (hwy_gae) with the reference's float64 arithmetic.
  * PPOAgent (:157-327): same constructor, select_action, update(last_value), save / load and
    the same metrics dict.

MI355X additions (the batched hot path):
  * ActorCritic.act(states) -- batched sampling on device, no host sync.
  * RolloutBuffer -- device-resident [T, E] rollout storage written by the env kernel in place.
  * PPOAgent.update_rollout(buffer, last_values) -- GAE kernel, global advantage normalisation,
    one minibatch permutation reused for every epoch (ppo/agent.py:205), per-minibatch clipped
    PPO step.  The step is captured once in a HIP graph and replayed; with a process group the
    flat gradient bucket is all-reduced (RCCL) between the two captured halves.
"""

from __future__ import annotations

import logging
import math
from typing import Any, Dict, List, Optional

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.distributions import Normal

from utils.graphs import capture as graph_capture

METRIC_KEYS = ("policy_loss", "value_loss", "entropy", "loss", "clip_fraction", "approx_kl")
_LOG_SQRT_2PI = 0.5 * math.log(2 * math.pi)


class ActorCritic(nn.Module):
    """Shared 2-layer ReLU trunk, actor mean head + state-independent log_std, critic head."""

    def __init__(self, state_dim: int, action_dim: int, hidden_dim: int = 128,
                 device: torch.device = torch.device("cpu")):
        super().__init__()
        self.device = device
        self.shared = nn.Sequential(
            nn.Linear(state_dim, hidden_dim), nn.ReLU(),
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(),
        )
        self.actor_mean = nn.Sequential(
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, action_dim)
        )
        self.log_std = nn.Parameter(torch.zeros(action_dim))
        self.critic = nn.Sequential(
            nn.Linear(hidden_dim, hidden_dim), nn.ReLU(), nn.Linear(hidden_dim, 1)
        )
        self.to(self.device)

    def forward(self, x):
        if isinstance(x, np.ndarray):
            x = torch.as_tensor(x, dtype=torch.float32, device=self.device)
        h = self.shared(x)
        return self.actor_mean(h), self.log_std.exp(), self.critic(h)

    @staticmethod
    def squashed_log_prob(dist: Normal, z: torch.Tensor) -> torch.Tensor:
        a = torch.tanh(z)
        return (dist.log_prob(z) - torch.log1p(-a.pow(2) + 1e-6)).sum(dim=-1)

    def get_action(self, state, deterministic: bool = False):
        """Reference single-state API (numpy in, numpy / Python scalars out)."""
        mean, std, value = self.forward(state)
        if deterministic:
            z = mean
            log_prob = None
        else:
            dist = Normal(mean, std, validate_args=False)
            z = dist.sample()
            log_prob = self.squashed_log_prob(dist, z)
        action = torch.tanh(z)
        return (action.detach().cpu().numpy(), z.detach().cpu().numpy(),
                None if log_prob is None else log_prob.item(),
                value.detach().cpu().numpy()[0])

    @torch.no_grad()
    def act(self, states: torch.Tensor, deterministic: bool = False,
            generator: Optional[torch.Generator] = None, noise: Optional[torch.Tensor] = None):
        """Batched device sampling: returns (action, pre_tanh, log_prob, value) tensors.
        ``noise`` (same shape as the mean) is a pre-drawn standard normal sample to use instead
        of drawing one from ``generator``."""
        mean, std, value = self.forward(states)
        if deterministic:
            z = mean
            logp = torch.zeros(mean.shape[0], device=mean.device)
        else:
            eps = noise if noise is not None else torch.randn(
                mean.shape, device=mean.device, dtype=mean.dtype, generator=generator)
            z = mean + std * eps
            logp = self.squashed_log_prob(Normal(mean, std, validate_args=False), z)
        return torch.tanh(z), z, logp, value.squeeze(-1)

    def evaluate(self, states, actions, pre_tanh_actions):
        mean, std, values = self.forward(states)
        dist = Normal(mean, std, validate_args=False)  # no host-syncing argument checks
        log_probs = self.squashed_log_prob(dist, pre_tanh_actions)
        entropy = dist.entropy().sum(dim=-1)
        return log_probs, values, entropy


class PPOMemory:
    """List-based rollout memory of the reference (one env, Python-side appends)."""

    def __init__(self, batch_size: int = 64, device: torch.device = torch.device("cpu")):
        self.batch_size = batch_size
        self.device = device
        self.clear()

    def store(self, state, action, pre_tanh_action, reward, next_state, log_prob, done, value):
        self.states.append(state)
        self.actions.append(action)
        self.pre_tanh_actions.append(pre_tanh_action)
        self.rewards.append(reward)
        self.next_states.append(next_state)
        self.log_probs.append(log_prob)
        self.dones.append(done)
        self.values.append(value)

    def clear(self):
        self.states: List[Any] = []
        self.actions: List[Any] = []
        self.pre_tanh_actions: List[Any] = []
        self.rewards: List[float] = []
        self.next_states: List[Any] = []
        self.log_probs: List[float] = []
        self.dones: List[bool] = []
        self.values: List[float] = []

    def compute_advantages(self, gamma: float, lam: float, last_value: float):
        """GAE of ppo/agent.py:126-138 on the HIP device (hwy_gae); returns numpy arrays."""
        from hwy import ops
        from hwy.native import HwyNativeError

        dev = self.device if torch.device(self.device).type == "cuda" else (
            torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None)
        if dev is None:
            raise HwyNativeError("compute_advantages runs the HIP GAE kernel; no HIP device found")
        T = len(self.rewards)
        rew = torch.as_tensor(np.asarray(self.rewards, np.float32).reshape(T, 1), device=dev)
        val = torch.as_tensor(np.asarray(self.values, np.float32).reshape(T, 1), device=dev)
        done = torch.as_tensor(np.asarray(self.dones, np.uint8).reshape(T, 1), device=dev)
        last = torch.tensor([float(last_value)], dtype=torch.float32, device=dev)
        adv, ret = ops.gae(rew, done, val, last, gamma, lam)
        return adv.view(T).cpu().numpy(), ret.view(T).cpu().numpy()

    def get_batches(self):
        n = len(self.states)
        indices = np.arange(n, dtype=np.int64)
        np.random.shuffle(indices)  # global numpy RNG, as ppo/agent.py:143
        return [indices[i:i + self.batch_size] for i in range(0, n, self.batch_size)]

    def get_tensors(self):
        dev = self.device
        f = lambda xs: torch.as_tensor(np.array(xs), dtype=torch.float32, device=dev)  # noqa: E731
        return f(self.states), f(self.actions), f(self.pre_tanh_actions), f(self.log_probs)


class RolloutBuffer:
    """Device-resident rollout of T steps x E envs (the env kernel writes rows in place).

    ``episode_stats``: also ``ep_stats`` [T, E, 8] (hwy_step_with_info's per-episode sums where an
    episode finished, 0 elsewhere) and ``acc`` [E, 8] (the running sums of the current episodes,
    carried from rollout to rollout); the rollout then issues the info variant of the step.

    ``truncation_bootstrap``: also ``final_obs`` [E, S] (the terminal observations of the envs
    that finished in the current step; one row set, reused every step) and ``boot_values`` [T, E]
    (V(final observation) at the truncated, not terminated rows, 0 elsewhere), which
    PPOAgent.update_rollout feeds to ops.gae_boot (LockstepRollout(truncation="bootstrap")).

    ``safety_stats``: also ``traffic_stats`` [T, E, 8] (hwy_traffic's per-episode reduction of the
    ego's time-to-collision, headway, gap and distance where an episode finished -- on the
    reference schedule row T - 1 also holds the rows of the episodes the cut ended -- 0
    elsewhere) and ``traffic_acc`` [E, 8] (the running reduction of the current episodes, carried
    from rollout to rollout); the rollout then issues one hwy_traffic launch per env step.

    ``shield``: also ``exec_actions`` [T, E, A] (the actions the env executed: the policy's where
    the shield let it stand, a fallback's elsewhere) and ``chosen`` [T, E] int32 (the candidate the
    shield picked, 0: the policy's own); ``actions``, ``pre_tanh``, ``log_probs`` and ``values``
    stay the policy's (LockstepRollout(shield=...))."""

    def __init__(self, T: int, E: int, state_dim: int, action_dim: int, device: torch.device,
                 episode_stats: bool = False, truncation_bootstrap: bool = False,
                 safety_stats: bool = False, shield: bool = False):
        kw = dict(device=device, dtype=torch.float32)
        self.T, self.E, self.state_dim = T, E, state_dim
        self.states = torch.zeros(T + 1, E, state_dim, **kw)  # row T = bootstrap obs
        self.pre_tanh = torch.zeros(T, E, action_dim, **kw)
        self.actions = torch.zeros(T, E, action_dim, **kw)
        self.log_probs = torch.zeros(T, E, **kw)
        self.values = torch.zeros(T, E, **kw)
        self.rewards = torch.zeros(T, E, **kw)
        self.terminated = torch.zeros(T, E, device=device, dtype=torch.uint8)
        self.truncated = torch.zeros(T, E, device=device, dtype=torch.uint8)
        self.dones = torch.zeros(T, E, device=device, dtype=torch.uint8)
        self.ep_return = torch.zeros(T, E, **kw)
        self.ep_length = torch.zeros(T, E, device=device, dtype=torch.int32)
        self.noise = torch.zeros(T, E, action_dim, **kw)  # the rollout's sampling noise
        self.ep_stats = self.acc = None
        if episode_stats:
            from hwy._abi import HWY_INFO_NACC

            self.ep_stats = torch.zeros(T, E, HWY_INFO_NACC, **kw)
            self.acc = torch.zeros(E, HWY_INFO_NACC, **kw)
        self.final_obs = self.boot_values = None
        if truncation_bootstrap:
            self.final_obs = torch.zeros(E, state_dim, **kw)
            self.boot_values = torch.zeros(T, E, **kw)
        self.traffic_stats = self.traffic_acc = None
        if safety_stats:
            from hwy._abi import HWY_TRAFFIC_NACC

            self.traffic_stats = torch.zeros(T, E, HWY_TRAFFIC_NACC, **kw)
            self.traffic_acc = torch.zeros(E, HWY_TRAFFIC_NACC, **kw)
        self.exec_actions = self.chosen = None
        if shield:
            self.exec_actions = torch.zeros(T, E, action_dim, **kw)
            self.chosen = torch.zeros(T, E, device=device, dtype=torch.int32)

    @property
    def n(self) -> int:
        return self.T * self.E

    def step_info(self, t: int):
        """step_into's ``info`` for rollout step t (None without episode_stats)."""
        if self.ep_stats is None:
            return None
        return {"acc": self.acc, "ep_stats": self.ep_stats[t]}

    def draw_noise(self, generator: Optional[torch.Generator] = None) -> None:
        """All T steps' standard normal sampling noise in one draw (one launch per rollout
        instead of one per step); step t acts with ``noise[t]``."""
        torch.randn(self.noise.shape, generator=generator, device=self.noise.device,
                    out=self.noise)

    def finish_dones(self) -> None:
        """dones = terminated | truncated for the whole rollout, once."""
        torch.bitwise_or(self.terminated, self.truncated, out=self.dones)


class _Learner:
    """Per-minibatch clipped-PPO step over a flattened device rollout, optionally graph-captured.

    Semantics per minibatch (ppo/agent.py:216-262): ratio = exp(logp - old); kl = mean(ratio - 1
    - log ratio); surrogate clipped at 1 +- eps; MSE value loss against returns; loss = pg +
    vc*vf - ec*entropy; zero grad, backward, [all-reduce mean], clip_grad_norm_, Adam step.
    Batch metrics land in a device buffer row per minibatch; nothing syncs with the host.
    """

    def __init__(self, agent: "PPOAgent", n: int, mb: int, n_steps: int, use_graph: bool,
                 group=None):
        self.agent = agent
        ac = agent.actor_critic
        dev = agent.device
        self.params = [p for p in ac.parameters()]
        numel = sum(p.numel() for p in self.params)
        self.flat_grad = torch.zeros(numel, device=dev, dtype=torch.float32)
        off = 0
        for p in self.params:
            p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
            off += p.numel()
        self.group = group
        self.world = 1 if group is None else torch.distributed.get_world_size(group)
        self.mb = mb
        self.n = n
        self.idx = torch.zeros(mb, dtype=torch.int64, device=dev)
        self.metrics = torch.zeros(max(1, n_steps), len(METRIC_KEYS), device=dev)
        self.row = torch.zeros((), dtype=torch.int64, device=dev)
        self.src: Dict[str, torch.Tensor] = {}
        self.use_graph = use_graph and dev.type == "cuda"
        self.g_fwd = self.g_opt = None

    def activate(self):
        """Point every parameter's .grad at this learner's flat buffer (another cached learner,
        or FusedPPO's flat gradient, may hold them); the same views, so captured graphs stay
        valid."""
        p0 = self.params[0]
        if p0.grad is None or p0.grad.data_ptr() != self.flat_grad.data_ptr():
            off = 0
            for p in self.params:
                p.grad = self.flat_grad[off:off + p.numel()].view_as(p)
                off += p.numel()

    def bind(self, states, pre_tanh, old_logp, adv, ret):
        same = all(self.src.get(k) is v for k, v in (("s", states), ("z", pre_tanh),
                                                      ("lp", old_logp), ("a", adv), ("r", ret)))
        if not same:
            self.src = dict(s=states, z=pre_tanh, lp=old_logp, a=adv, r=ret)
            self.g_fwd = self.g_opt = None  # new storage -> recapture

    def _fwd_bwd(self):
        ag = self.agent
        s = self.src["s"].index_select(0, self.idx)
        z = self.src["z"].index_select(0, self.idx)
        old = self.src["lp"].index_select(0, self.idx)
        a = self.src["a"].index_select(0, self.idx)
        r = self.src["r"].index_select(0, self.idx)
        new_lp, values, ent = ag.actor_critic.evaluate(s, torch.tanh(z), z)
        log_ratio = new_lp - old
        ratios = torch.exp(log_ratio)
        surr1 = ratios * a
        surr2 = torch.clamp(ratios, 1 - ag.eps_clip, 1 + ag.eps_clip) * a
        actor_loss = -torch.min(surr1, surr2).mean()
        critic_loss = F.mse_loss(values.squeeze(-1), r)
        ent_b = ent.mean()
        loss = actor_loss + ag.value_coef * critic_loss - ag.entropy_coef * ent_b
        self.flat_grad.zero_()
        loss.backward()
        with torch.no_grad():
            kl = ((ratios - 1) - log_ratio).mean()
            clip = (torch.abs(ratios - 1) > ag.eps_clip).float().sum()  # / size on the host
            vals = torch.stack([actor_loss, critic_loss, ent_b, loss, clip, kl]).detach()
            self.metrics.index_copy_(0, self.row.view(1), vals.view(1, -1))

    def _opt(self):
        ag = self.agent
        nn.utils.clip_grad_norm_(self.params, ag.max_grad_norm, foreach=True)
        ag.optimizer.step()
        self.row.add_(1)

    def _allreduce(self):
        if self.group is not None:
            torch.distributed.all_reduce(self.flat_grad, group=self.group)
            self.flat_grad.div_(self.world)

    def _capture(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):  # warm-up builds autograd / optimizer state eagerly
            for _ in range(2):
                self._fwd_bwd()
                self._allreduce()
                self._opt()
        torch.cuda.current_stream().wait_stream(s)
        self.g_fwd, self.g_opt = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with graph_capture(self.g_fwd):
            self._fwd_bwd()
        with graph_capture(self.g_opt):
            self._opt()

    def step(self, idx: torch.Tensor, kl_limit: Optional[float] = None) -> bool:
        """One minibatch step.  With ``kl_limit`` (PPOAgent.target_kl's rule, on the host): after
        the backward pass the minibatch's mean KL, the float32 the metrics row holds, is read
        back, and unless kl <= kl_limit the step is dropped -- no optimizer step, the row index
        stays on the tripping row -- and True is returned."""
        self.idx.copy_(idx)
        if self.use_graph:
            if self.g_fwd is None:
                saved = [p.detach().clone() for p in self.params]
                opt_state = {k: {kk: (vv.clone() if torch.is_tensor(vv) else vv)
                                 for kk, vv in v.items()} for k, v in self.agent.optimizer.state.items()}
                row = self.row.clone()
                self._capture()
                with torch.no_grad():  # undo the warm-up steps
                    for p, v in zip(self.params, saved):
                        p.copy_(v)
                    for k, st in self.agent.optimizer.state.items():
                        for kk, vv in st.items():
                            if not torch.is_tensor(vv):
                                continue
                            if k in opt_state:
                                vv.copy_(opt_state[k][kk])
                            else:  # state created by the warm-up: back to a fresh Adam
                                vv.zero_()
                    self.row.copy_(row)
            self.g_fwd.replay()
            if kl_limit is not None and self._trips(kl_limit):
                return True
            self._allreduce()
            self.g_opt.replay()
        else:
            self._fwd_bwd()
            if kl_limit is not None and self._trips(kl_limit):
                return True
            self._allreduce()
            self._opt()
        return False

    def _trips(self, kl_limit: float) -> bool:
        kl = float(self.metrics[int(self.row), METRIC_KEYS.index("approx_kl")])  # exact float32
        return not (kl <= kl_limit)


class _PendingMetrics:
    """An update's metrics dict whose device-to-host copy is in flight (non-blocking, pinned):
    result() waits for it, so a caller can enqueue the next rollout before reading them."""

    def __init__(self, logger, vals: torch.Tensor):
        self.logger = logger
        self._out = None
        if vals.is_cuda:
            self._host = torch.empty(vals.shape, dtype=vals.dtype, pin_memory=True)
            self._host.copy_(vals, non_blocking=True)
            self._event = torch.cuda.Event()
            self._event.record()
        else:
            self._host, self._event = vals, None

    def result(self) -> Dict[str, float]:
        if self._out is not None:
            return self._out
        if self._event is not None:
            self._event.synchronize()
        vals = self._host.tolist()
        ctl = None
        if len(vals) > len(METRIC_KEYS) + 1:  # target_kl / lr_anneal_updates: three more values
            ctl, vals = vals[len(METRIC_KEYS) + 1:], vals[:len(METRIC_KEYS) + 1]
        m = dict(zip(METRIC_KEYS, vals[:-1]))
        out = {
            "loss": m["loss"],
            "policy_loss": m["policy_loss"],
            "value_loss": m["value_loss"],
            "entropy": m["entropy"],
            "clip_fraction": m["clip_fraction"],
            "approx_kl": m["approx_kl"],
            "explained_variance": vals[-1],
        }
        self.logger.info(
            "update_complete loss=%.4f policy_loss=%.4f value_loss=%.4f entropy=%.4f "
            "clip_frac=%.3f kl=%.5f explained_var=%.3f", out["loss"], out["policy_loss"],
            out["value_loss"], out["entropy"], out["clip_fraction"], out["approx_kl"],
            out["explained_variance"])
        if ctl is not None:
            out["steps_applied"] = int(ctl[0])
            out["kl_stopped"] = bool(ctl[1])
            out["approx_kl_last"] = ctl[2]
        self._out = out
        return out


class PPOAgent:
    def __init__(self, state_dim: int, action_dim: int, lr: float = 1e-4, gamma: float = 0.99,
                 lam: float = 0.95, eps_clip: float = 0.2, value_coef: float = 0.5,
                 entropy_coef: float = 0.005, max_grad_norm: float = 0.5, epochs: int = 6,
                 batch_size: int = 64, hidden_dim: int = 128,
                 logger: Optional[logging.Logger] = None,
                 device: torch.device = torch.device("cpu"),
                 num_minibatches: Optional[int] = None, use_graphs: bool = True,
                 process_group=None, seed: Optional[int] = None, backend: str = "auto",
                 target_kl: Optional[float] = None, lr_anneal_updates: Optional[int] = None):
        """``target_kl`` = tau: the Stable-Baselines3 early stop, checked per minibatch -- a
        minibatch whose mean approx_kl is not <= float32(1.5 tau) is not applied and ends the
        update.  ``lr_anneal_updates`` = U: update u = 0, 1, ... steps with
        float32(lr max(1 - u / U, 0)).  Both default to off, work on update_rollout (the fused
        backend runs them inside the captured update, backend="torch" on the host) and are
        refused with a process group and by the one-env update()."""
        self.device = torch.device(device)
        for name, v in (("target_kl", target_kl), ("lr_anneal_updates", lr_anneal_updates)):
            if v is not None and process_group is not None:
                raise ValueError(f"{name} is not supported with a process group")
        if target_kl is not None and not float(target_kl) >= 0.0:
            raise ValueError(f"target_kl must be >= 0, got {target_kl!r}")
        if lr_anneal_updates is not None and int(lr_anneal_updates) < 1:
            raise ValueError(f"lr_anneal_updates must be >= 1, got {lr_anneal_updates!r}")
        self.target_kl = None if target_kl is None else float(target_kl)
        self.kl_limit = None if target_kl is None else float(np.float32(1.5 * float(target_kl)))
        self.lr_anneal_updates = None if lr_anneal_updates is None else int(lr_anneal_updates)
        self.lr0 = float(lr)
        self._lr_table = self._lr_cell = None
        self._ctl_runner = None
        self._last_ctl = None
        # table prepares / graph captures of the control path (ppo/group.py:_run_group_steps)
        self.stats = {"update_prepare": 0, "update_capture": 0}
        if backend not in ("auto", "hip", "torch"):
            raise ValueError(f"backend must be auto|hip|torch, got {backend!r}")
        # "hip": update_rollout runs the fused HIP minibatch step (hwy/ppo_native.py);
        # "torch": autograd + torch.optim.Adam (the reference arithmetic, also used by update())
        self.backend = backend
        self._fused = None
        self.actor_critic = ActorCritic(state_dim, action_dim, hidden_dim, device=self.device)
        self._dist = process_group
        written = False
        if process_group is not None:  # identical initial weights on every rank
            for p in self.actor_critic.parameters():
                torch.distributed.broadcast(p.data, src=0, group=process_group)
            written = True
        capturable = self.device.type == "cuda"
        self.optimizer = torch.optim.Adam(self.actor_critic.parameters(), lr=lr,
                                          capturable=capturable)
        self.gamma, self.lam, self.eps_clip = gamma, lam, eps_clip
        self.value_coef, self.entropy_coef = value_coef, entropy_coef
        self.max_grad_norm, self.epochs, self.batch_size = max_grad_norm, epochs, batch_size
        self.num_minibatches = num_minibatches
        self.use_graphs = use_graphs
        self.logger = logger or logging.getLogger(__name__)
        self.memory = PPOMemory(batch_size=batch_size, device=self.device)
        # torch-path learners, one per (rows, minibatch, steps, graph) geometry: a ragged
        # partition alternates between two sizes without reallocating
        self._learners: Dict[tuple, _Learner] = {}
        # which optimizer holds the current Adam state: "torch" (agent.optimizer) or "fused"
        # (FusedPPO's m / v / step); handed over whenever an update switches paths
        self._adam_owner = "torch"
        self._warned_ragged = False
        self.updates = 0  # completed update() / update_rollout() calls (evaluation memo key)
        # torch-path optimizer runs: a graph-replayed torch learner writes the parameters in
        # place without bumping their version counters, so the fused path's weight tile images
        # key their staleness on this count too (hwy/ppo_native.py)
        self._torch_param_writes = 0
        if written:  # the broadcast above wrote through .data
            self.params_written()
        self.generator = None
        if self.device.type == "cuda":
            self.generator = torch.Generator(device=self.device)
            self.generator.manual_seed(int(seed) if seed is not None else torch.initial_seed() % (2**63))

    # ------------------------------------------------------------------ acting
    def select_action(self, state, deterministic: bool = False, out=None, noise=None):
        """Batched (2-D tensor) or single-state acting.  For a batch, `out` may name the four
        tensors (action, pre_tanh, log_prob, value) to write, e.g. a rollout buffer's rows, and
        `noise` a pre-drawn (B, action_dim) standard normal sample (RolloutBuffer.draw_noise)."""
        if isinstance(state, torch.Tensor) and state.dim() == 2:
            if self._act_fused_ok(state):
                from hwy.ppo_native import fused_act

                return fused_act(self, state, deterministic, self.generator, out=out, noise=noise)
            res = self.actor_critic.act(state, deterministic, generator=self.generator,
                                        noise=noise)
            if out is None:
                return res
            for dst, src in zip(out, res):
                dst.copy_(src.reshape(dst.shape))
            return tuple(out)
        return self.actor_critic.get_action(state, deterministic)

    def value(self, states: torch.Tensor) -> torch.Tensor:
        """V(s) for a batch, e.g. a rollout's bootstrap row: the value output of the fused act
        launch when acting is fused, else the torch forward."""
        if self._act_fused_ok(states):
            from hwy.ppo_native import fused_act

            return fused_act(self, states.contiguous(), True)[3]
        with torch.no_grad():
            return self.actor_critic.forward(states)[2].squeeze(-1)

    def value_masked(self, states: torch.Tensor, truncated: torch.Tensor,
                     terminated: Optional[torch.Tensor] = None,
                     out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """V(s) at the rows with ``truncated & ~terminated`` and exactly 0 elsewhere (the
        bootstrap values of a time limit): hwy_ppo_value_masked when acting is fused -- tiles
        without such a row read no weight -- else the torch forward under torch.where."""
        if self._act_fused_ok(states):
            from hwy.ppo_native import fused_value_masked

            return fused_value_masked(self, states, truncated, terminated, out=out)
        with torch.no_grad():
            v = self.actor_critic.forward(states)[2].squeeze(-1)
            mark = truncated.bool()
            if terminated is not None:
                mark = mark & ~terminated.bool()
            res = torch.where(mark, v, torch.zeros_like(v))
        if out is None:
            return res
        out.copy_(res)
        return out

    _INPUT_GRAD_NAMES = ("acceleration", "steering", "value")

    def input_gradients(self, states: torch.Tensor) -> Dict[str, torch.Tensor]:
        """What the policy's outputs depend on in a batch of observations (B, S): the gradients
        of the pre-tanh actor means -- action 0, the longitudinal command ("acceleration"), and
        action 1, the lateral one ("steering"; ContinuousAction's order) -- and of the critic's
        "value" with respect to the state row, each (B, S).  One hwy_ppo_input_grad launch with
        the three one-hot cotangents where acting is fused, else (always with backend="torch" and
        on the CPU) torch autograd on the module.  Parameters, their .grad and their version
        counters are left as they are."""
        if states.dim() != 2:
            raise ValueError("input_gradients takes a (B, S) batch of states")
        B = states.shape[0]
        if self._act_fused_ok(states):
            from hwy.ppo_native import fused_input_grad

            cot = torch.eye(3, device=states.device).unsqueeze(1).expand(3, B, 3).contiguous()
            g = fused_input_grad(self, states.float().contiguous(), cot)
            return {n: g[k] for k, n in enumerate(self._INPUT_GRAD_NAMES)}
        with torch.enable_grad():
            x = states.detach().clone().requires_grad_(True)
            mean, _, value = self.actor_critic.forward(x)
            outs = (mean[:, 0].sum(), mean[:, 1].sum(), value.sum())
            # with respect to the states only: no parameter's .grad is read or written
            grads = [torch.autograd.grad(o, x, retain_graph=(k < 2))[0]
                     for k, o in enumerate(outs)]
        return {n: g.detach() for n, g in zip(self._INPUT_GRAD_NAMES, grads)}

    def _act_fused_ok(self, state: torch.Tensor) -> bool:
        """Batched acting runs through hwy_ppo_act (one launch) unless backend='torch'."""
        if self.backend == "torch" or not state.is_cuda:
            return False
        from hwy.ppo_native import act_supported

        H = self.actor_critic.shared[0].weight.shape[0]
        ok = act_supported(state.shape[1], H, self.actor_critic.log_std.numel())
        if not ok and self.backend == "hip":
            raise ValueError("backend='hip' acting needs action_dim 2, state_dim % 4 == 0 "
                             "(<= 1024) and hidden_dim in {64,128,...,512}")
        return ok

    # ------------------------------------------------------------------ metrics
    @property
    def controlled(self) -> bool:
        """A KL target or an lr schedule is set."""
        return self.kl_limit is not None or self.lr_anneal_updates is not None

    def lr_at(self, u: int) -> float:
        """The learning rate of update u: float32(lr max(1 - u / U, 0)); lr without a schedule."""
        U = self.lr_anneal_updates
        if U is None:
            return self.lr0
        return float(np.float32(self.lr0 * max(1.0 - u / U, 0.0)))

    def lr_device(self) -> Optional[torch.Tensor]:
        """This update's learning rate as one device float: element min(updates, U) of the
        schedule precomputed on the device (a view, no host round trip); None without one."""
        U = self.lr_anneal_updates
        if U is None:
            return None
        if self._lr_table is None:
            self._lr_table = torch.tensor([self.lr_at(u) for u in range(U + 1)],
                                          dtype=torch.float32, device=self.device)
        u = min(self.updates, U)
        return self._lr_table[u:u + 1]

    def _torch_lr(self) -> None:
        """backend="torch": this update's learning rate into agent.optimizer (a device scalar the
        captured optimizer step reads on cuda, a float on the CPU)."""
        if self.lr_anneal_updates is None:
            return
        g = self.optimizer.param_groups[0]
        if self.device.type != "cuda":
            g["lr"] = self.lr_at(self.updates)
            return
        if self._lr_cell is None:
            self._lr_cell = torch.zeros((), dtype=torch.float32, device=self.device)
        self._lr_cell.copy_(self.lr_device()[0])
        g["lr"] = self._lr_cell

    def _finish_metrics(self, rows: torch.Tensor, sizes: List[int], values, returns,
                        deferred: bool = False, ctl=None):
        """Aggregate per-minibatch rows like ppo/agent.py:263-287 (epoch means, then the mean
        over epochs, in float64) plus explained variance (:272-280).  Computed on the rows'
        device with one host transfer at the end (the clip count becomes a fraction by dividing
        by each minibatch's size, as the reference's per-batch clip_frac).  ``deferred``: return
        a pending result whose host copy is still in flight (see _PendingMetrics)."""
        if ctl is not None:
            return self._finish_metrics_ctl(rows, sizes, values, returns, deferred, ctl)
        nb = len(sizes)
        r = torch.as_tensor(rows).to(torch.float64)[: self.epochs * nb].view(self.epochs, nb, -1)
        ci = METRIC_KEYS.index("clip_fraction")
        inv = torch.tensor([1.0 / s for s in sizes], dtype=torch.float64, device=r.device)
        r = torch.cat([r[..., :ci], r[..., ci:ci + 1] * inv.view(1, nb, 1), r[..., ci + 1:]], -1)
        means = r.mean(dim=1).mean(dim=0)  # epoch means, then over epochs
        with torch.no_grad():
            var_y = torch.var(returns)
            ev = torch.where(var_y > 0, 1 - torch.var(returns - values) / var_y,
                             torch.zeros_like(var_y)).to(torch.float64).to(means.device)
        pending = _PendingMetrics(self.logger, torch.cat([means, ev.view(1)]))
        return pending if deferred else pending.result()

    def _finish_metrics_ctl(self, rows, sizes, values, returns, deferred, ctl):
        """_finish_metrics with a KL target or an lr schedule: ctl = (rows_written, stopped), two
        0-d tensors on the rows' device (the fused learner's counters[1] and stopped_at >= 0), so
        nothing is read back before the one transfer.  An update that applied k steps wrote k rows,
        plus the tripping row when it stopped.  The six means are float64 means over the k applied
        rows (the tripping row's alone when k = 0); three values follow the explained variance:
        steps_applied, kl_stopped, approx_kl_last (the last written row's KL)."""
        nb = len(sizes)
        steps = self.epochs * nb
        r = torch.as_tensor(rows).to(torch.float64)[:steps]
        ci, ki = METRIC_KEYS.index("clip_fraction"), METRIC_KEYS.index("approx_kl")
        inv = torch.tensor([1.0 / s for s in sizes], dtype=torch.float64,
                           device=r.device).repeat(self.epochs)
        r = torch.cat([r[:, :ci], r[:, ci:ci + 1] * inv.view(-1, 1), r[:, ci + 1:]], -1)
        written, stopped = ctl
        written = written.to(torch.int64).clamp(1, steps)
        applied = written - stopped.to(torch.int64)
        keep = torch.arange(steps, device=r.device) < applied.clamp_min(1)
        # where, not a product: rows past the last written one may hold anything
        means = torch.where(keep.view(-1, 1), r, torch.zeros_like(r)).sum(0) / keep.sum()
        kl_last = r.index_select(0, (written - 1).view(1))[0, ki]
        with torch.no_grad():
            var_y = torch.var(returns)
            ev = torch.where(var_y > 0, 1 - torch.var(returns - values) / var_y,
                             torch.zeros_like(var_y)).to(torch.float64).to(means.device)
        tail = torch.stack([applied.to(torch.float64), stopped.to(torch.float64), kl_last])
        pending = _PendingMetrics(self.logger, torch.cat([means, ev.view(1), tail]))
        return pending if deferred else pending.result()

    def _learner_for(self, n: int, mb: int, steps: int, graph: bool) -> _Learner:
        key = (n, mb, steps, graph)
        L = self._learners.get(key)
        if L is None:
            L = _Learner(self, n, mb, steps, graph, group=self._dist)
            self._learners[key] = L
        L.activate()
        return L

    def _adam_to(self, owner: str):
        """Hand the Adam state (moments, step count) to the optimizer about to step."""
        if owner == self._adam_owner:
            return
        F = self._fused
        if F is not None:
            if owner == "torch":
                F.export_torch_state()
            else:
                F._import_torch_state()
        self._adam_owner = owner

    def _run_epochs(self, states, pre_tanh, old_logp, adv, ret, batches: List[torch.Tensor]):
        self._adam_to("torch")
        self._torch_param_writes += 1  # retires every fused tile image (see __init__)
        self._torch_lr()
        lim = self.kl_limit
        self._last_ctl = None
        n = states.shape[0]
        sizes = {int(b.numel()) for b in batches}
        mb = max(sizes)
        ragged = len(sizes) > 1
        steps = self.epochs * len(batches)
        if ragged:  # short last minibatch (reference's n % batch_size != 0): eager, exact sizes
            rows = []
            for _ in range(self.epochs):
                for b in batches:
                    L = self._learner_for(n, int(b.numel()), 1, False)
                    L.bind(states, pre_tanh, old_logp, adv, ret)
                    L.row.zero_()
                    tripped = L.step(b, lim)
                    rows.append(L.metrics[0].clone())
                    if tripped:
                        break
                else:
                    continue
                break
            if self.controlled:
                self._last_ctl = self._host_ctl(len(rows), tripped, states.device)
                rows += [torch.zeros_like(rows[0])] * (steps - len(rows))
            return torch.stack(rows)
        L = self._learner_for(n, mb, steps, self.use_graphs)
        L.bind(states, pre_tanh, old_logp, adv, ret)
        L.row.zero_()
        done = tripped = 0
        for _ in range(self.epochs):
            for b in batches:
                tripped = L.step(b, lim)
                done += 1
                if tripped:
                    break
            if tripped:
                break
        if self.controlled:
            self._last_ctl = self._host_ctl(done, tripped, states.device)
        return L.metrics

    @staticmethod
    def _host_ctl(written: int, tripped, device):
        """(rows written, stopped) of a host-side update, as _finish_metrics_ctl takes them."""
        return (torch.tensor(int(written), dtype=torch.int64, device=device),
                torch.tensor(bool(tripped), device=device))

    # ------------------------------------------------------------------ reference update
    def update(self, last_value: float = 0.0):
        """Clipped-PPO update over the list memory (ppo/agent.py:196-308)."""
        for name, v in (("target_kl", self.target_kl), ("lr_anneal_updates", self.lr_anneal_updates)):
            if v is not None:
                raise ValueError(f"{name} is not supported by the one-env update(); use "
                                 "update_rollout")
        states, actions, pre_tanh, old_log_probs = self.memory.get_tensors()
        adv_np, ret_np = self.memory.compute_advantages(self.gamma, self.lam, last_value)
        advantages = torch.as_tensor(adv_np, device=self.device)
        returns = torch.as_tensor(ret_np, device=self.device)
        advantages = (advantages - advantages.mean()) / (advantages.std() + 1e-8)
        batches = [torch.as_tensor(b, device=self.device) for b in self.memory.get_batches()]
        rows = self._run_epochs(states, pre_tanh, old_log_probs, advantages, returns, batches)
        values = torch.as_tensor(np.asarray(self.memory.values, np.float32), device=self.device)
        out = self._finish_metrics(rows, [int(b.numel()) for b in batches], values,
                                   returns)
        self.memory.clear()
        self.updates += 1
        return out

    # ------------------------------------------------------------------ batched update
    def normalize_advantages(self, adv: torch.Tensor) -> torch.Tensor:
        """(adv - mean) / (unbiased std + 1e-8) over ALL ranks' samples (ppo/agent.py:204)."""
        if self._dist is None:
            return (adv - adv.mean()) / (adv.std() + 1e-8)
        a64 = adv.double()
        stats = torch.stack([torch.tensor(float(adv.numel()), device=adv.device, dtype=torch.float64),
                             a64.sum(), (a64 * a64).sum()])
        torch.distributed.all_reduce(stats, group=self._dist)
        n, s1, s2 = stats[0], stats[1], stats[2]
        mean = s1 / n
        var = (s2 - n * mean * mean) / (n - 1)
        return ((adv - mean.float()) / (var.clamp_min(0).sqrt().float() + 1e-8))

    def update_rollout(self, buf: RolloutBuffer, last_values: torch.Tensor,
                       perm: Optional[torch.Tensor] = None, return_metrics=True):
        """Batched clipped-PPO update on a device rollout (no host round trips until the end).
        return_metrics: True -> the metrics dict; "deferred" -> a pending result (metrics
        computed on the device, host copy in flight; .result() gives the dict); False -> the
        device rows only."""
        from hwy import ops

        T, E = buf.T, buf.E
        if getattr(buf, "boot_values", None) is not None:
            # bootstrap at truncation: V(final observation) instead of 0 at a time limit
            adv, ret = ops.gae_boot(buf.rewards, buf.terminated, buf.truncated, buf.values,
                                    last_values, buf.boot_values, self.gamma, self.lam)
        else:
            adv, ret = ops.gae(buf.rewards, buf.dones, buf.values, last_values, self.gamma,
                               self.lam)
        n = T * E
        states = buf.states[:T].reshape(n, -1)
        pre_tanh = buf.pre_tanh.reshape(n, -1)
        old_lp = buf.log_probs.reshape(n)
        ret = ret.reshape(n)
        adv = self.normalize_advantages(adv.reshape(n))
        if perm is None:
            perm = torch.randperm(n, device=self.device, generator=self.generator)
        sizes = self.minibatch_sizes(n)
        mb, nmb = sizes[0], len(sizes)
        if len(set(sizes)) == 1 and self._fused_ok(mb):
            F = self._fused_for(mb, nmb, n)
            self._adam_to("fused")
            F_adv, F_ret, F_perm = self._static_bufs
            F_adv.copy_(adv)
            F_ret.copy_(ret)
            F_perm.copy_(perm)
            if self.controlled:
                rows = self._run_fused_ctl(F, states, pre_tanh, old_lp, F_adv, F_ret, F_perm)
            else:
                rows = F.run(states, pre_tanh, old_lp, F_adv, F_ret, F_perm)
        else:
            # one partition for all epochs (ppo/agent.py:205); a short last minibatch takes the
            # reference's ragged path (eager torch steps at the exact sizes)
            if len(set(sizes)) > 1 and not self._warned_ragged and self._fused_ok(mb):
                self._warned_ragged = True
                self.logger.warning(
                    f"update_rollout: {n} samples split into unequal minibatches {sorted(set(sizes))}"
                    " -- the fused HIP update needs equal sizes, so these updates run the eager "
                    "torch path (choose num_minibatches / batch_size dividing T x E)")
            starts = np.cumsum([0] + sizes)
            batches = [perm[int(starts[i]):int(starts[i + 1])] for i in range(nmb)]
            rows = self._run_epochs(states, pre_tanh, old_lp, adv, ret, batches)
        self.updates += 1
        if not return_metrics:
            return rows
        return self._finish_metrics(rows, sizes, buf.values.reshape(n), ret,
                                    deferred=return_metrics == "deferred",
                                    ctl=self._last_ctl if self.controlled else None)

    def _run_fused_ctl(self, F, states, pre_tanh, old_lp, adv, ret, perm) -> torch.Tensor:
        """FusedPPO.run for a learner with a KL target or an lr schedule: the whole update as a
        one-learner scheduled GroupStep (hwy_ppo_sched_ctl_*, hwy_ppo_sched_set_lr), captured and
        replayed like a grouped update.  An applied step is the solo step bit for bit."""
        from ppo.group import _run_group_steps

        mb, nmb = F.mb, F.nmb
        self.check_control_dims(mb, nmb)
        key = (states.data_ptr(), pre_tanh.data_ptr(), old_lp.data_ptr(), adv.data_ptr(),
               ret.data_ptr(), perm.data_ptr()) + F._scalar_key() + (self.kl_limit,
                                                                    self.lr_anneal_updates)
        run = self._ctl_runner
        if run is None or run[0] != (id(F), key):
            args = [F._args(states, pre_tanh, old_lp, adv, ret, perm.data_ptr() + i * mb * 8)
                    for i in range(nmb)]
            run = [(id(F), key), args, None]
            self._ctl_runner = run
        args = run[1]
        F._last_args, F._last_inputs = args, (states, pre_tanh, old_lp, adv, ret, perm)
        F.counters[1].zero_()
        F.sync_params(args[0])
        ctx = {"fused": [F], "args": [args], "key": key, "mb": mb, "nmb": nmb,
               "epochs": self.epochs}
        run[2] = _run_group_steps(self, [ctx], run[2])
        step = run[2][1]
        F._tiles_version = F._param_versions()
        self._last_ctl = self._fused_ctl(F, step, 0)
        return F.metrics

    def check_control_dims(self, mb: int, nmb: int = 1) -> None:
        """ValueError, naming the option, unless minibatches of mb rows can run the scheduled
        step a KL target / lr schedule needs: the fused path at 16-row tiles (host-only: the
        table-size query of the C ABI, no device call)."""
        import ctypes

        from hwy.ppo_native import PpoDims, _bind, _bind_group, lib

        L = _bind_group(_bind(lib()))
        sd = self.actor_critic.shared[0].weight
        dims = (PpoDims * 1)(PpoDims(int(mb), sd.shape[1], sd.shape[0], 2))
        if L.hwy_ppo_sched_table_bytes(dims, (ctypes.c_int32 * 1)(int(nmb)), 1) < 0:
            name = "target_kl" if self.target_kl is not None else "lr_anneal_updates"
            raise ValueError(f"{name} needs the fused step at 16-row tiles (state_dim % 4 == 0 up "
                             f"to 1024, minibatches below 64 x CUs rows); got minibatches of "
                             f"{mb} rows, state_dim {sd.shape[1]}")

    @staticmethod
    def _fused_ctl(F, step, g: int):
        """(rows written, stopped) of learner g of a scheduled update, on the device."""
        stopped = (step.stopped_at[g] >= 0 if step.stopped_at is not None
                   else torch.zeros((), dtype=torch.bool, device=F.counters.device))
        return F.counters[1], stopped

    def minibatch_sizes(self, n: int) -> List[int]:
        """The minibatch partition of an n-sample update; every sample is used once per epoch.

        ``num_minibatches`` set: that many near-equal minibatches (the first n % nmb one row
        larger).  Otherwise the reference's get_batches partition (ppo/agent.py:140-146):
        ``batch_size`` rows each and a short last minibatch when batch_size does not divide n."""
        if self.num_minibatches:
            nmb = max(1, min(int(self.num_minibatches), n))
            q, r = divmod(n, nmb)
            sizes = [q + 1] * r + [q] * (nmb - r)
        else:
            bs = max(1, int(self.batch_size))
            sizes = [bs] * (n // bs) + ([n % bs] if n % bs else [])
        assert sum(sizes) == n, (sizes, n)
        return sizes

    # ------------------------------------------------------------------ fused HIP step
    def _fused_ok(self, mb: int) -> bool:
        if self.backend == "torch" or self.device.type != "cuda":
            return False
        sd = self.actor_critic.shared[0].weight
        H = sd.shape[0]
        ok = self.actor_critic.log_std.numel() == 2 and H % 64 == 0 and 64 <= H <= 512
        if not ok and self.backend == "hip":
            raise ValueError("backend='hip' needs action_dim 2 and hidden_dim in {64,128,...,512}")
        return ok

    def _optimizer_follows(self, old, new) -> None:
        """agent.optimizer steps the Parameter objects `new` (layout order) from now on, with
        the Adam state it held for `old`: a writer that replaced the module's Parameters
        (load_state_dict(assign=True), a new module) left it stepping objects nobody reads."""
        swap = {id(o): n for o, n in zip(old, new) if o is not n}
        if not swap:
            return
        opt = self.optimizer
        for o, n in zip(old, new):
            if o is not n and o in opt.state:
                opt.state[n] = opt.state.pop(o)
        for g in opt.param_groups:
            g["params"] = [swap.get(id(p), p) for p in g["params"]]

    def params_written(self) -> None:
        """Tell the agent that its parameters were written in place through ``.data``
        (``p.data.copy_()``, ``p.data.mul_()``, ``torch._foreach_*`` on ``.data`` tensors, a
        ``torch.distributed.broadcast(p.data)``): such a write bumps no version counter, so
        nothing else can see it.  Retires what was derived from the old weights -- the weight
        tile images acting and the fused step stream, the grouped acting tables and captured
        rollouts keyed on them, the torch-path learners and the evaluation memo -- exactly as a
        torch-path update does.  Every other way of writing the parameters needs no call."""
        self._torch_param_writes += 1
        self._learners = {}

    def __deepcopy__(self, memo):
        """A copy with its own weights, optimizer state and generator state and none of the
        original's device caches (flat buffer, FusedPPO, tile images, captured learners): it
        rebuilds them on first use, over its own storage."""
        import copy

        if self._fused is not None and self._adam_owner == "fused":
            self._fused.export_torch_state()  # the copy starts from agent.optimizer's state
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        fresh = {"_fused": None, "_flat": None, "_flat_guard": None, "_act_tile_image": None,
                 "_static_bufs": None, "_ctl_runner": None, "_last_ctl": None}
        for k, v in self.__dict__.items():
            if k in fresh:
                new.__dict__[k] = fresh[k]
            elif k == "_learners":
                new.__dict__[k] = {}
            elif k in ("logger", "_dist"):
                new.__dict__[k] = v
            elif k == "generator" and v is not None:
                g = torch.Generator(device=v.device)
                g.set_state(v.get_state())
                new.__dict__[k] = g
            else:
                new.__dict__[k] = copy.deepcopy(v, memo)
        new._adam_owner = "torch"
        return new

    def _fused_for(self, mb: int, nmb: int, n: int):
        from hwy.ppo_native import FusedPPO, flat_params

        F = self._fused
        # the parameters may have been rebound to other storage since F was built (p.data = ...,
        # vector_to_parameters, load_state_dict(assign=True), a .cpu()/.to(device) round trip, a
        # new module): flat_params then made a new flat buffer, and F would train the old one,
        # which nothing reads any more
        moved = F is not None and F.flat is not flat_params(self)[0]
        if (F is None or moved or F.mb != mb or F.nmb != nmb
                or F.metrics.shape[0] != self.epochs * nmb):
            if F is not None and self._adam_owner == "fused":
                F.export_torch_state()  # carry Adam's moments and step count to the new instance
            if moved:
                self._optimizer_follows(F.params, flat_params(self)[3])
            self._adam_owner = "torch"  # the new instance imports agent.optimizer's state
            F = FusedPPO(self, mb, nmb, group=self._dist, use_graphs=self.use_graphs)
            self._fused = F
            self._learners = {}
        bufs = getattr(self, "_static_bufs", None)
        if bufs is None or bufs[0].numel() != n:
            dev = self.device
            self._static_bufs = (torch.empty(n, device=dev), torch.empty(n, device=dev),
                                 torch.empty(n, device=dev, dtype=torch.int64))
        return F

    # ------------------------------------------------------------------ checkpoints
    def save(self, path: str):
        if self._fused is not None and self._adam_owner == "fused":
            self._fused.export_torch_state()
        torch.save({"model": self.actor_critic.state_dict(),
                    "optimizer": self.optimizer.state_dict()}, path)
        self.logger.info(f"model_saved path={path}")

    def load(self, path: str, load_optimizer: bool = True):
        ckpt = torch.load(path, map_location=self.device, weights_only=True)
        self.actor_critic.load_state_dict(ckpt["model"])
        if load_optimizer and "optimizer" in ckpt:
            self.optimizer.load_state_dict(ckpt["optimizer"])
            if self._fused is not None and self._adam_owner == "fused":
                self._fused._import_torch_state()
        self._learners = {}
        self.logger.info(f"model_loaded path={path}")
        return ckpt.get("config", {})
