"""Grouped PPO launches for learners whose minibatch rows, minibatch counts and epochs differ
(include/hwy_ppo.h: hwy_ppo_sched_*; hwy/ppo_native.py GroupStep; ppo/group.py GroupBatch;
ExperimentRunner.launch_batch).  The scheduled kernels run the solo kernels' bodies per learner,
on the learner's own minibatch of the slot, so every comparison here is bit equality with the
same learner run alone by the same library -- no tolerance."""

import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (H, S, B, nmb, epochs): both wave-count classes (H 128 / 256 / 384 / 512 run 8 waves, H 64 / 192
# run 4); B = 40 leaves the last 16-row tile of every minibatch partial and uses 240 of the 256
# indices.  steps = epochs * nmb = 8, 24, 12, 16, 12, 8: 24 slots, period 4.
LEARNERS = [(128, 60, 64, 4, 2), (256, 120, 32, 8, 3), (384, 60, 64, 4, 3),
            (64, 60, 32, 8, 2), (192, 120, 40, 6, 2), (512, 120, 64, 4, 2)]
N_SAMPLES, MAX_STEPS, PERIOD = 256, 24, 4


def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _stream():
    from hwy.native import stream_ptr

    return stream_ptr()


@functools.lru_cache(maxsize=None)
def _start(H, S):
    """Seeded flat weights, a 256-sample rollout and a stored permutation for one learner
    (shared, never written)."""
    from hwy.ppo_native import param_layout

    _, numel = param_layout(S, H)
    g = torch.Generator(device=DEV).manual_seed(1000 * H + S)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    return {"flat": r(numel) * 0.05, "states": r(N_SAMPLES, S), "pre": r(N_SAMPLES, 2) * 0.5,
            "old_lp": r(N_SAMPLES) * 0.1 - 2.0, "adv": r(N_SAMPLES), "ret": r(N_SAMPLES),
            "perm": torch.randperm(N_SAMPLES, device=DEV, generator=g)}


class _Learner:
    """One learner's own buffers (a fresh copy of the seeded start; Adam state zero)."""

    def __init__(self, H, S, B, nmb, epochs):
        from hwy.ppo_native import PpoDims

        L = _lib()
        st = _start(H, S)
        assert nmb * B <= N_SAMPLES
        self.st, self.B, self.nmb, self.epochs, self.steps = st, B, nmb, epochs, nmb * epochs
        self.dims = PpoDims(B, S, H, 2)
        n = st["flat"].numel()
        self.flat = st["flat"].clone()
        self.grads = torch.zeros(n, device=DEV)
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        self.counters = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.metrics = torch.zeros(self.steps, 6, device=DEV)
        ws = L.hwy_ppo_workspace_bytes(ctypes.byref(self.dims))
        assert ws > 0
        self.workspace = torch.zeros(int(ws), dtype=torch.uint8, device=DEV)
        self.sync()

    def sync(self):
        a0 = self.args(0)
        assert _lib().hwy_ppo_sync_params(ctypes.byref(a0), _stream()) == 0

    def reset(self):
        """Back to the seeded start, in place (captured graphs and tables keep pointing here)."""
        self.flat.copy_(self.st["flat"])
        for t in (self.grads, self.m, self.v, self.counters, self.metrics, self.workspace):
            t.zero_()
        self.sync()

    def args(self, i):
        """The learner's arguments for minibatch i (i = 0: idx is the whole permutation)."""
        from hwy.ppo_native import PpoArgs

        st, a = self.st, PpoArgs()
        a.dims = self.dims
        a.states, a.pre_tanh, a.old_logp = (st["states"].data_ptr(), st["pre"].data_ptr(),
                                            st["old_lp"].data_ptr())
        a.adv, a.ret = st["adv"].data_ptr(), st["ret"].data_ptr()
        a.idx = st["perm"].data_ptr() + i * self.B * 8
        a.params, a.grads = self.flat.data_ptr(), self.grads.data_ptr()
        a.adam_m, a.adam_v = self.m.data_ptr(), self.v.data_ptr()
        a.counters, a.metrics = self.counters.data_ptr(), self.metrics.data_ptr()
        a.workspace = self.workspace.data_ptr()
        a.eps_clip, a.value_coef, a.entropy_coef, a.max_grad_norm = 0.2, 0.5, 0.005, 0.5
        a.lr, a.beta1, a.beta2, a.adam_eps = 3e-4, 0.9, 0.999, 1e-8
        a.grads_modified = 0
        return a

    def state(self):
        return {"params": self.flat, "grads": self.grads, "adam_m": self.m, "adam_v": self.v,
                "counters": self.counters, "metrics": self.metrics}


@functools.lru_cache(maxsize=None)
def _solo_steps(H, S, B, nmb, epochs):
    """The learner stepped alone: hwy_ppo_forward_backward + hwy_ppo_optimizer for epochs * nmb
    steps in (epoch, minibatch) order."""
    L, lr = _lib(), _Learner(H, S, B, nmb, epochs)
    for _ in range(epochs):
        for i in range(nmb):
            a = lr.args(i)
            assert L.hwy_ppo_forward_backward(ctypes.byref(a), _stream()) == 0
            assert L.hwy_ppo_optimizer(ctypes.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in lr.state().items()}


class _Sched:
    """Learners with one prepared schedule table."""

    def __init__(self, learners):
        from hwy.ppo_native import PpoArgs, PpoDims, PpoSchedPlan

        L = self.L = _lib()
        G = self.G = len(learners)
        self.spec = list(learners)
        self.ls = [_Learner(*l) for l in learners]
        dims = (PpoDims * G)(*[l.dims for l in self.ls])
        self.nmb = (ctypes.c_int32 * G)(*[l.nmb for l in self.ls])
        self.epochs = (ctypes.c_int32 * G)(*[l.epochs for l in self.ls])
        nb = L.hwy_ppo_sched_table_bytes(dims, self.nmb, G)
        assert nb > 0
        self.arr = (PpoArgs * G)()
        for g, l in enumerate(self.ls):
            a = l.args(0)
            ctypes.memmove(ctypes.byref(self.arr[g]), ctypes.byref(a), ctypes.sizeof(PpoArgs))
        self.table = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
        self.plan = PpoSchedPlan()
        assert L.hwy_ppo_sched_prepare(self.arr, self.nmb, self.epochs, G, self.table.data_ptr(),
                                       ctypes.byref(self.plan), _stream()) == 0

    def begin(self, stream=None):
        return self.L.hwy_ppo_sched_begin(ctypes.byref(self.plan), self.table.data_ptr(),
                                          _stream() if stream is None else stream)

    def step(self, slot, stream=None):
        return self.L.hwy_ppo_sched_step(ctypes.byref(self.plan), self.table.data_ptr(), slot,
                                         _stream() if stream is None else stream)

    def advance(self, slots, stream=None):
        return self.L.hwy_ppo_sched_advance(ctypes.byref(self.plan), self.table.data_ptr(), slots,
                                            _stream() if stream is None else stream)

    def run_eager(self):
        assert self.begin() == 0
        for s in range(self.plan.max_steps):
            assert self.step(s) == 0
        torch.cuda.synchronize()

    def assert_equals_solo(self):
        for spec, l in zip(self.spec, self.ls):
            want = _solo_steps(*spec)
            assert int(l.counters[0]) == int(l.counters[1]) == l.steps, spec
            for k, v in l.state().items():
                assert torch.equal(v, want[k]), (spec, k)
            assert bool(torch.isfinite(l.metrics).all()) and bool((l.flat != l.st["flat"]).any())

    def snapshot(self):
        return [{**{k: v.clone() for k, v in l.state().items()}, "workspace": l.workspace.clone()}
                for l in self.ls]


def _hip():
    """The HIP runtime this process already uses (the one torch and libhwy.so loaded)."""
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipStreamBeginCapture.argtypes = [ctypes.c_void_p, ctypes.c_int]
    hip.hipStreamEndCapture.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_void_p)]
    hip.hipGraphGetNodes.argtypes = [ctypes.c_void_p, ctypes.c_void_p,
                                     ctypes.POINTER(ctypes.c_size_t)]
    hip.hipGraphDestroy.argtypes = [ctypes.c_void_p]
    return hip


def _launches_issued(call, want_rc=0) -> int:
    """How many launches `call(stream)` issues: it is captured into a HIP graph on a stream of
    its own (nothing runs) and the graph's nodes are counted."""
    hip = _hip()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipStreamBeginCapture(s.cuda_stream, 1) == 0  # thread-local mode
    rc = call(s.cuda_stream)
    assert hip.hipStreamEndCapture(s.cuda_stream, ctypes.byref(graph)) == 0
    assert rc == want_rc
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    hip.hipGraphDestroy(graph)
    return int(n.value)


@pytest.fixture(scope="module")
def eager():
    """The six learners stepped through the whole update, slot by slot (shared by the tests
    below; they leave it as it is)."""
    sc = _Sched(LEARNERS)
    sc.run_eager()
    return sc


def test_sched_steps_equal_each_learners_solo_update(eager):
    p = eager.plan
    assert p.max_steps == MAX_STEPS and p.period == PERIOD and p.G == len(LEARNERS)
    assert p.present[0] == 4 and p.present[1] == 2 and p.launches == 5
    # each class's row grid covers its learner with the most rows per minibatch
    assert p.grid_rows[0] == 4 and p.grid_rows[1] == 3
    eager.assert_equals_solo()
    assert [int(l.counters[1]) for l in eager.ls] == [8, 24, 12, 16, 12, 8]
    assert _launches_issued(lambda st: eager.step(0, st)) == 5


def test_slots_past_the_schedule_touch_nothing(eager):
    before = eager.snapshot()
    assert eager.step(MAX_STEPS) == 0 and eager.step(MAX_STEPS + 1) == 0
    torch.cuda.synchronize()
    for l, b, a in zip(LEARNERS, before, eager.snapshot()):
        for k in b:
            assert torch.equal(b[k], a[k]), (l, k)
    eager.assert_equals_solo()


def test_sched_graph_of_one_period_replayed(eager):
    """step(0..3) + advance(4) captured once; begin + 6 replays is the update, a 7th replay does
    nothing, and begin restarts the schedule for the next update."""
    from utils.graphs import capture

    sc = _Sched(LEARNERS)

    def period(stream=None):
        rc = 0
        for s in range(PERIOD):
            rc |= sc.step(s, stream)
        return rc | sc.advance(PERIOD, stream)

    assert _launches_issued(period) == PERIOD * 5 + 1
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with capture(graph, stream=side):
            assert period() == 0
    torch.cuda.current_stream().wait_stream(side)
    assert sc.begin() == 0
    for _ in range(MAX_STEPS // PERIOD):
        graph.replay()
    torch.cuda.synchronize()
    sc.assert_equals_solo()
    for l, e in zip(sc.ls, eager.ls):
        for k, v in l.state().items():
            assert torch.equal(v, e.state()[k]), k
    # the next update of fresh learners: the slot base starts over; one replay too many is inert
    for l in sc.ls:
        l.reset()
    assert sc.begin() == 0
    for _ in range(MAX_STEPS // PERIOD + 1):
        graph.replay()
    torch.cuda.synchronize()
    sc.assert_equals_solo()


def test_sched_step_of_one_wave_count_class_issues_four_launches():
    even = [l for l in LEARNERS if (l[0] // 64) % 2 == 0]
    sc = _Sched(even)
    assert sc.plan.launches == 4 and sc.plan.present[0] == 4 and sc.plan.present[1] == 0
    assert sc.plan.max_steps == 24 and sc.plan.period == 4
    assert _launches_issued(lambda st: sc.step(0, st)) == 4
    sc.run_eager()
    sc.assert_equals_solo()


def test_sched_calls_refuse_bad_arguments():
    from hwy.ppo_native import PpoSchedPlan

    sc = _Sched(LEARNERS[:3])
    L, G = sc.L, sc.G
    before = sc.snapshot()

    def prepare(arr=sc.arr, nmb=sc.nmb, epochs=sc.epochs):
        plan = PpoSchedPlan()
        rc = L.hwy_ppo_sched_prepare(arr, nmb, epochs, G, sc.table.data_ptr(), ctypes.byref(plan),
                                     _stream())
        assert rc == 0 or plan.G == 0  # a refused prepare leaves the plan alone
        return rc

    assert prepare() == 0
    assert prepare(nmb=(ctypes.c_int32 * G)(4, 0, 4)) == -1
    assert prepare(nmb=(ctypes.c_int32 * G)(4, 8, -1)) == -1
    assert prepare(epochs=(ctypes.c_int32 * G)(2, 3, 0)) == -1
    assert prepare(epochs=(ctypes.c_int32 * G)(-2, 3, 3)) == -1
    bad = type(sc.arr)()
    ctypes.memmove(bad, sc.arr, ctypes.sizeof(bad))
    bad[1].dims.A = 3
    assert prepare(arr=bad) == -1
    bad[1].dims.A = 2
    bad[2].grads_modified = 1
    assert prepare(arr=bad) == -1
    bad[2].grads_modified = 0
    assert prepare(arr=bad) == 0
    # a negative slot (or a negative advance) is refused before any launch
    assert _launches_issued(lambda st: sc.step(-1, st), want_rc=-1) == 0
    assert _launches_issued(lambda st: sc.advance(-1, st), want_rc=-1) == 0
    torch.cuda.synchronize()
    for b, a in zip(before, sc.snapshot()):
        for k in b:
            assert torch.equal(b[k], a[k]), k


# ---------------------------------------------------------------- GroupBatch and the runner
def _solo(cond, d, seed, E, T, iters, hp):
    """One experiment alone: the runner's construction and _train_vector's loop
    (LockstepRollout + update_rollout), as tests/test_group_gpu.py runs it."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.wrappers import make_env
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout
    from utils.reproducibility import set_random_seeds

    set_random_seeds(seed)
    env = make_env(cond, HIGHWAY_CONFIG, d_embed=d,
                   env_overrides=dict(num_envs=E, device=DEV, autoreset=True))
    if hasattr(env, "to"):
        env = env.to(DEV)
    base = env.unwrapped
    sd = base.obs_rows * base.obs_features
    agent = PPOAgent(sd, 2, device=DEV, **hp)
    base.set_seed_schedule(seed)
    obs, _ = env.reset()
    buf = RolloutBuffer(T, E, sd, 2, DEV)
    buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, base, buf)
    hist = []
    for _ in range(iters):
        roll.run()
        hist.append({k: getattr(buf, k).clone() for k in ("states", "rewards", "log_probs")})
        agent.update_rollout(buf, agent.value(buf.states[T]))
        buf.states[0].copy_(buf.states[T])
    torch.cuda.synchronize()
    return agent, hist, env


def test_group_batch_across_batch_sizes_and_epochs_matches_solo_runs():
    """GroupBatch over an h128 cell (batch_size 64, 2 epochs), an h256 cell (32, 3) and an h384
    cell (64, 3) on 256-sample rollouts: 8, 24 and 12 steps per update in 24 slots, inside
    captured graphs, each experiment its solo run."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from ppo.agent import PPOAgent
    from ppo.group import GroupBatch, build_group

    E, T, iters = 16, 16, 3
    hp = lambda H, bs, ep: dict(lr=3e-4, epochs=ep, batch_size=bs, hidden_dim=H)
    cells = [(Condition.SORTED, None, hp(128, 64, 2), [42, 1042]),
             (Condition.SHUFFLED_RANKPE, 4, hp(256, 32, 3), [7, 2042]),
             (Condition.SHUFFLED_ROPE, 4, hp(384, 64, 3), [99])]
    groups = [build_group(c, HIGHWAY_CONFIG, seeds, E, T, DEV,
                          lambda sd, h=h: PPOAgent(sd, 2, device=DEV, **h), d_embed=d)
              for c, d, h, seeds in cells]
    batch = GroupBatch(groups)
    hist = []
    for _ in range(iters):
        batch.rollout()
        hist.append([{k: getattr(g.buf, k).clone() for k in ("states", "rewards", "log_probs")}
                     for g in groups])
        batch.update()
    torch.cuda.synchronize()
    step = batch._runner[1]
    assert step.sched and (step.max_steps, step.period) == (24, 4)
    for gi, (c, d, h, seeds) in enumerate(cells):
        for j, s in enumerate(seeds):
            agent, shist, env = _solo(c, d, s, E, T, iters, h)
            sl = slice(j * E, (j + 1) * E)
            for it in range(iters):
                for k, v in hist[it][gi].items():
                    assert torch.equal(v[:, sl], shist[it][k]), (gi, j, it, k)
            for (k, va), (_, vb) in zip(agent.actor_critic.state_dict().items(),
                                        groups[gi].agents[j].actor_critic.state_dict().items()):
                assert torch.equal(va, vb), (gi, j, k)
            env.close()
    # one table for the whole batch and one captured graph of one period
    assert batch.stats["update_prepare"] == 1 and batch.stats["update_capture"] == 1
    assert batch.launches_per_step == 4
    for g in groups:
        g.close()


def _comparable(mh):
    """metrics_history without its two wall-clock fields: `timestamps` (seconds since the run
    began, per evaluation) and each policy update's `time` (seconds the update took)."""
    out = {k: v for k, v in mh.items() if k != "timestamps"}
    out["policy_updates"] = [{k: v for k, v in u.items() if k != "time"}
                             for u in mh["policy_updates"]]
    return out


def test_runner_launch_batch_across_batch_sizes_and_epochs_equals_launch_group(tmp_path,
                                                                              monkeypatch):
    """ExperimentRunner.launch_batch over two cells that differ in epochs and batch_size returns,
    per experiment, exactly what launch_group returns for its cell alone."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)

    def exp(cond, d, H, bs, epochs, seed):
        hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=epochs, batch_size=bs, hidden_dim=H,
                         d_embed=d)
        hp.entropy_coef = 0.005
        hp.steps_per_update = 16 * 32
        return Experiment(name=f"s_{cond.name}_h{H}_b{bs}_e{epochs}_{seed}", condition=cond, hp=hp,
                          seed=seed, max_episodes=24, target_reward=1e9,
                          extra={"num_envs": 16, "eval_interval": 8, "log_interval": 50},
                          env_config_overrides={})

    cells = [[exp(Condition.SORTED, None, 256, 64, 2, s) for s in (42, 1042)],
             [exp(Condition.SHUFFLED_RANKPE, 4, 384, 32, 3, s) for s in (7, 2042)]]
    batched = ExperimentRunner(HIGHWAY_CONFIG).launch_batch(cells)
    for cell, got in zip(cells, batched):
        alone = ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
        for a, b in zip(alone, got):
            assert a["status"] == b["status"] == "COMPLETED", (a.get("error_message"),
                                                               b.get("error_message"))
            assert a["rewards"] == b["rewards"] and a["avg_rewards"] == b["avg_rewards"]
            assert _comparable(a["metrics_history"]) == _comparable(b["metrics_history"])
            assert len(a["metrics_history"]["policy_updates"]) > 0
