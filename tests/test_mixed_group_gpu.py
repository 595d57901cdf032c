"""Grouped PPO launches for learners of different hidden widths (include/hwy_ppo.h:
hwy_ppo_mixed_*; hwy/ppo_native.py GroupStep / GroupAct; ppo/group.py GroupBatch;
ExperimentRunner.launch_batch; training/routine.py evaluate_many).  The mixed kernels run the
solo kernels' bodies per learner, so every comparison here is bit equality with the same
learner run alone by the same library -- no tolerance."""

import ctypes
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

# (H, S): both wave-count classes (H 128 / 256 / 384 / 512 run 8 waves, H 64 / 192 run 4)
LEARNERS = [(128, 60), (256, 120), (384, 60), (512, 120), (64, 60), (192, 120)]
N_SAMPLES, STEPS = 256, 3


def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _stream():
    from hwy.native import stream_ptr

    return stream_ptr()


@functools.lru_cache(maxsize=None)
def _start(H, S):
    """Seeded flat weights and a 256-sample rollout for one learner (shared, never written)."""
    from hwy.ppo_native import param_layout

    _, numel = param_layout(S, H)
    g = torch.Generator(device=DEV).manual_seed(1000 * H + S)
    r = lambda *shape: torch.randn(*shape, device=DEV, generator=g)
    return {"flat": r(numel) * 0.05, "states": r(N_SAMPLES, S), "pre": r(N_SAMPLES, 2) * 0.5,
            "old_lp": r(N_SAMPLES) * 0.1 - 2.0, "adv": r(N_SAMPLES), "ret": r(N_SAMPLES),
            "perm": torch.randperm(N_SAMPLES, device=DEV, generator=g)}


class _Learner:
    """One learner's own buffers (a fresh copy of the seeded start; Adam state zero)."""

    def __init__(self, H, S, B):
        from hwy.ppo_native import PpoDims

        L = _lib()
        st = _start(H, S)
        self.st, self.B = st, B
        self.dims = PpoDims(B, S, H, 2)
        n = st["flat"].numel()
        self.flat = st["flat"].clone()
        self.grads = torch.zeros(n, device=DEV)
        self.m = torch.zeros(n, device=DEV)
        self.v = torch.zeros(n, device=DEV)
        self.counters = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.metrics = torch.zeros(STEPS, 6, device=DEV)
        ws = L.hwy_ppo_workspace_bytes(ctypes.byref(self.dims))
        assert ws > 0
        self.workspace = torch.zeros(int(ws), dtype=torch.uint8, device=DEV)

    def args(self, step):
        from hwy.ppo_native import PpoArgs

        st, a = self.st, PpoArgs()
        a.dims = self.dims
        a.states, a.pre_tanh, a.old_logp = (st["states"].data_ptr(), st["pre"].data_ptr(),
                                            st["old_lp"].data_ptr())
        a.adv, a.ret = st["adv"].data_ptr(), st["ret"].data_ptr()
        a.idx = st["perm"].data_ptr() + step * self.B * 8
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
def _solo_steps(H, S, B):
    """The learner stepped alone: hwy_ppo_forward_backward + hwy_ppo_optimizer, STEPS times."""
    L, lr = _lib(), _Learner(H, S, B)
    a0 = lr.args(0)
    assert L.hwy_ppo_sync_params(ctypes.byref(a0), _stream()) == 0
    for i in range(STEPS):
        a = lr.args(i)
        assert L.hwy_ppo_forward_backward(ctypes.byref(a), _stream()) == 0
        assert L.hwy_ppo_optimizer(ctypes.byref(a), _stream()) == 0
    torch.cuda.synchronize()
    return {k: v.clone() for k, v in lr.state().items()}


def _mixed_steps(learners, B):
    from hwy.ppo_native import PpoArgs, PpoDims, PpoMixedPlan

    L = _lib()
    G = len(learners)
    ls = [_Learner(H, S, B) for H, S in learners]
    dims = (PpoDims * G)(*[l.dims for l in ls])
    nb = L.hwy_ppo_mixed_table_bytes(dims, G)
    assert nb > 0
    for l in ls:
        a0 = l.args(0)
        assert L.hwy_ppo_sync_params(ctypes.byref(a0), _stream()) == 0
    tables, plans = [], []
    for i in range(STEPS):
        arr = (PpoArgs * G)()
        for g, l in enumerate(ls):
            a = l.args(i)
            ctypes.memmove(ctypes.byref(arr[g]), ctypes.byref(a), ctypes.sizeof(PpoArgs))
        t = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
        plan = PpoMixedPlan()
        assert L.hwy_ppo_mixed_prepare(arr, G, t.data_ptr(), ctypes.byref(plan), _stream()) == 0
        tables.append(t)
        plans.append(plan)
    for t, plan in zip(tables, plans):
        assert L.hwy_ppo_mixed_step(ctypes.byref(plan), t.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    return ls, plans, tables


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


def _launches_issued(call) -> int:
    """How many launches `call(stream)` issues: it is captured into a HIP graph on a stream of
    its own (nothing runs) and the graph's nodes are counted."""
    hip = _hip()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    graph, n = ctypes.c_void_p(), ctypes.c_size_t()
    assert hip.hipStreamBeginCapture(s.cuda_stream, 1) == 0  # thread-local mode
    rc = call(s.cuda_stream)
    assert hip.hipStreamEndCapture(s.cuda_stream, ctypes.byref(graph)) == 0
    assert rc == 0
    assert hip.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
    hip.hipGraphDestroy(graph)
    return int(n.value)


@pytest.mark.parametrize("B", [64, 40])  # 40: the last 16-row tile of every learner is partial
def test_mixed_step_equals_each_learners_solo_steps(B):
    ls, plans, tables = _mixed_steps(LEARNERS, B)
    # two row launches (one per wave-count class) + weight gradients, slice sums, Adam
    assert all(p.launches == 5 and p.present[0] == 4 and p.present[1] == 2 for p in plans)
    assert plans[0].grid_rows[0] == plans[0].grid_rows[1] == (B + 15) // 16
    for (H, S), l in zip(LEARNERS, ls):
        want = _solo_steps(H, S, B)
        assert int(l.counters[0]) == int(l.counters[1]) == STEPS
        for k, v in l.state().items():
            assert torch.equal(v, want[k]), (H, S, k)
        assert bool(torch.isfinite(l.metrics).all()) and bool((l.flat != l.st["flat"]).any())
    # the launches the call really issues, counted as the nodes of a capture of it
    L = _lib()
    assert _launches_issued(lambda st: L.hwy_ppo_mixed_step(
        ctypes.byref(plans[0]), tables[0].data_ptr(), st)) == 5


def test_mixed_step_of_one_wave_count_class_issues_four_launches():
    even = [hs for hs in LEARNERS if (hs[0] // 64) % 2 == 0]
    ls, plans, tables = _mixed_steps(even, 64)
    assert all(p.launches == 4 and p.present[0] == 4 and p.present[1] == 0 for p in plans)
    L = _lib()
    assert _launches_issued(lambda st: L.hwy_ppo_mixed_step(
        ctypes.byref(plans[0]), tables[0].data_ptr(), st)) == 4
    for (H, S), l in zip(even, ls):
        want = _solo_steps(H, S, 64)
        for k, v in l.state().items():
            assert torch.equal(v, want[k]), (H, S, k)


def _tile_image(H, S, flat):
    """A weight tile image of `flat` (hwy_ppo_sync_params on a workspace of its own)."""
    from hwy.ppo_native import PpoArgs, PpoDims

    L = _lib()
    d = PpoDims(64, S, H, 2)
    ws = torch.zeros(int(L.hwy_ppo_workspace_bytes(ctypes.byref(d))), dtype=torch.uint8,
                     device=DEV)
    a = PpoArgs()
    a.dims = d
    a.params, a.workspace = flat.data_ptr(), ws.data_ptr()
    assert L.hwy_ppo_sync_params(ctypes.byref(a), _stream()) == 0
    return ws, ws.data_ptr() + int(L.hwy_ppo_tile_image_offset(ctypes.byref(d)))


@pytest.mark.parametrize("rows", [16, 5])          # 5: the evaluation's shape, a partial tile
@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("with_tiles", [True, False])
def test_mixed_act_equals_each_agents_solo_act(rows, stochastic, with_tiles):
    """hwy_ppo_mixed_act against hwy_ppo_act (what fused_act calls) per agent, the same weights,
    rows, noise and tile images: with tile images the H = 256 learner runs the compact body
    beside the others' row-image bodies in one launch."""
    from hwy.ppo_native import PpoActArgs, PpoDims, PpoMixedActPlan

    L = _lib()
    G = len(LEARNERS)
    keep, arr, solo_out, mix_out = [], (PpoActArgs * G)(), [], []
    for g, (H, S) in enumerate(LEARNERS):
        st = _start(H, S)
        states = st["states"][:rows].contiguous()
        noise = st["pre"][:rows].contiguous() if stochastic else None
        ws, tiles = _tile_image(H, S, st["flat"]) if with_tiles else (None, None)
        outs = [[torch.full((rows, 2), 7.0, device=DEV), torch.full((rows, 2), 7.0, device=DEV),
                 torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)]
                for _ in range(2)]
        keep.append((states, noise, ws))
        for a, o in ((PpoActArgs(), outs[0]), (arr[g], outs[1])):
            a.dims = PpoDims(rows, S, H, 2)
            a.states, a.params = states.data_ptr(), st["flat"].data_ptr()
            a.noise = None if noise is None else noise.data_ptr()
            a.action, a.pre_tanh, a.logp, a.value = (t.data_ptr() for t in o)
            a.tiles = tiles
            if o is outs[0]:
                assert L.hwy_ppo_act(ctypes.byref(a), _stream()) == 0
        solo_out.append(outs[0])
        mix_out.append(outs[1])
    table = torch.empty(int(L.hwy_ppo_mixed_act_table_bytes(G)), dtype=torch.uint8, device=DEV)
    plan = PpoMixedActPlan()
    assert L.hwy_ppo_mixed_act_prepare(arr, G, table.data_ptr(), ctypes.byref(plan),
                                       _stream()) == 0
    assert plan.launches == 2 and plan.tiles == int(with_tiles)
    assert L.hwy_ppo_mixed_act(ctypes.byref(plan), table.data_ptr(), _stream()) == 0
    torch.cuda.synchronize()
    assert _launches_issued(lambda st: L.hwy_ppo_mixed_act(
        ctypes.byref(plan), table.data_ptr(), st)) == 2
    for (H, S), so, mo in zip(LEARNERS, solo_out, mix_out):
        for name, a, b in zip(("action", "pre_tanh", "logp", "value"), so, mo):
            assert torch.equal(a, b), (H, S, name)
        assert bool((so[3] != 7.0).all())


@pytest.mark.parametrize("H", [64, 128, 192, 320, 384, 448, 512])
def test_act_from_a_tile_image_equals_act_from_the_params_rows(H):
    """A mixed acting group streams tile images for every learner or for none, so GroupAct gives
    a learner that has none an acting-only image where its solo call reads the params rows.
    hwy_ppo_act's two weight paths (act_body's TL true / false) must then give the same bits at
    every width that keeps both (H = 256 with an image takes the compact kernel, solo and
    grouped alike): state dims 60 (a partial last 16-block) and 120, 16 and 5 rows, with and
    without noise."""
    from hwy.ppo_native import PpoActArgs, PpoDims

    L = _lib()
    for S in (60, 120):
        st = _start(H, S)
        ws, tiles = _tile_image(H, S, st["flat"])
        for rows in (16, 5):
            states = st["states"][:rows].contiguous()
            for noise in (st["pre"][:rows].contiguous(), None):
                outs = []
                for tl in (tiles, None):
                    o = [torch.full((rows, 2), 7.0, device=DEV), torch.full((rows, 2), 7.0, device=DEV),
                         torch.full((rows,), 7.0, device=DEV), torch.full((rows,), 7.0, device=DEV)]
                    a = PpoActArgs()
                    a.dims = PpoDims(rows, S, H, 2)
                    a.states, a.params = states.data_ptr(), st["flat"].data_ptr()
                    a.noise = None if noise is None else noise.data_ptr()
                    a.action, a.pre_tanh, a.logp, a.value = (t.data_ptr() for t in o)
                    a.tiles = tl
                    assert L.hwy_ppo_act(ctypes.byref(a), _stream()) == 0
                    outs.append(o)
                torch.cuda.synchronize()
                for name, x, y in zip(("action", "pre_tanh", "logp", "value"), *outs):
                    assert torch.equal(x, y), (H, S, rows, noise is not None, name)
                assert bool((outs[0][3] != 7.0).all())
        del ws


def _hp(H, epochs=2):
    return dict(lr=3e-4, epochs=epochs, batch_size=64, hidden_dim=H)


def _solo(cond, d, seed, E, T, iters, H, overrides):
    """One experiment alone: the runner's construction and _train_vector's loop
    (LockstepRollout + update_rollout), as tests/test_group_gpu.py runs it."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.wrappers import make_env
    from ppo.agent import PPOAgent, RolloutBuffer
    from ppo.rollout import LockstepRollout
    from utils.reproducibility import set_random_seeds

    set_random_seeds(seed)
    env = make_env(cond, HIGHWAY_CONFIG, d_embed=d,
                   env_overrides=dict(overrides, num_envs=E, device=DEV, autoreset=True))
    if hasattr(env, "to"):
        env = env.to(DEV)
    base = env.unwrapped
    sd = base.obs_rows * base.obs_features
    agent = PPOAgent(sd, 2, device=DEV, **_hp(H))
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


def test_group_batch_across_hidden_widths_matches_solo_runs():
    """GroupBatch over an h128, an h256 and an h384 cell (state dims 60, 120, 120): one set of
    launches for all five learners, inside captured graphs, each experiment its solo run."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from ppo.agent import PPOAgent
    from ppo.group import GroupBatch, build_group

    E, T, iters = 16, 16, 3
    cells = [(Condition.SORTED, None, 128, [42, 1042]),
             (Condition.SHUFFLED_RANKPE, 4, 256, [7, 2042]),
             (Condition.SHUFFLED_ROPE, 4, 384, [99])]
    groups = [build_group(c, HIGHWAY_CONFIG, seeds, E, T, DEV,
                          lambda sd, H=H: PPOAgent(sd, 2, device=DEV, **_hp(H)), d_embed=d)
              for c, d, H, seeds in cells]
    batch = GroupBatch(groups)
    assert batch.act.mixed and batch.act.launches_per_act == 1
    hist = []
    for _ in range(iters):
        batch.rollout()
        hist.append([{k: getattr(g.buf, k).clone() for k in ("states", "rewards", "log_probs")}
                     for g in groups])
        batch.update()
    torch.cuda.synchronize()
    for gi, (c, d, H, seeds) in enumerate(cells):
        for j, s in enumerate(seeds):
            agent, shist, env = _solo(c, d, s, E, T, iters, H, {})
            sl = slice(j * E, (j + 1) * E)
            for it in range(iters):
                for k, v in hist[it][gi].items():
                    assert torch.equal(v[:, sl], shist[it][k]), (gi, j, it, k)
            for (k, va), (_, vb) in zip(agent.actor_critic.state_dict().items(),
                                        groups[gi].agents[j].actor_critic.state_dict().items()):
                assert torch.equal(va, vb), (gi, j, k)
            env.close()
    # one table preparation for the whole batch, the rollout captured as a graph: the mixed
    # launches ran inside captured graphs; the three even widths share one row launch
    assert batch.stats["update_prepare"] == 1 and batch.stats["rollout_capture"] == 1
    assert batch.stats["update_capture"] == 1
    assert batch.launches_per_step == 4
    for g in groups:
        g.close()


def test_runner_launch_batch_across_hidden_widths_equals_launch_group(tmp_path, monkeypatch):
    """ExperimentRunner.launch_batch over an h256 and an h384 cell returns, per experiment,
    exactly what launch_group returns for its cell alone."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    monkeypatch.chdir(tmp_path)

    def exp(cond, d, H, seed):
        hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=64, hidden_dim=H, d_embed=d)
        hp.entropy_coef = 0.005
        hp.steps_per_update = 16 * 32
        return Experiment(name=f"m_{cond.name}_h{H}_{seed}", condition=cond, hp=hp, seed=seed,
                          max_episodes=24, target_reward=1e9,
                          extra={"num_envs": 16, "num_minibatches": 8, "eval_interval": 8,
                                 "log_interval": 50}, env_config_overrides={})

    cells = [[exp(Condition.SORTED, None, 256, s) for s in (42, 1042)],
             [exp(Condition.SHUFFLED_RANKPE, 4, 384, s) for s in (7, 2042)]]
    batched = ExperimentRunner(HIGHWAY_CONFIG).launch_batch(cells)
    for cell, got in zip(cells, batched):
        alone = ExperimentRunner(HIGHWAY_CONFIG).launch_group(cell)
        for a, b in zip(alone, got):
            assert a["status"] == b["status"] == "COMPLETED", (a.get("error_message"),
                                                               b.get("error_message"))
            assert a["rewards"] == b["rewards"] and a["avg_rewards"] == b["avg_rewards"]
            assert _comparable(a["metrics_history"]) == _comparable(b["metrics_history"])
            assert len(a["metrics_history"]["policy_updates"]) > 0


def _comparable(mh):
    """metrics_history without its two wall-clock fields: `timestamps` (seconds since the run
    began, per evaluation) and each policy update's `time` (seconds the update took)."""
    out = {k: v for k, v in mh.items() if k != "timestamps"}
    out["policy_updates"] = [{k: v for k, v in u.items() if k != "time"}
                             for u in mh["policy_updates"]]
    return out


def test_evaluate_many_groups_agents_of_different_hidden_widths(monkeypatch):
    """evaluate_many over three agents of widths 128, 256 and 384 runs as ONE group (the mixed
    acting launch) and returns what evaluate returns for each alone; a repeat is a memo hit."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from experiments.wrappers import make_env
    from hwy import ppo_native
    from ppo.agent import PPOAgent
    from training import routine
    from utils.reproducibility import set_random_seeds

    items = []
    for H, seed in ((128, 42), (256, 1042), (384, 7)):
        set_random_seeds(seed)
        env = make_env(Condition.SORTED, HIGHWAY_CONFIG,
                       env_overrides=dict(num_envs=16, device=DEV, autoreset=True))
        if hasattr(env, "to"):
            env = env.to(DEV)
        base = env.unwrapped
        items.append((env, PPOAgent(base.obs_rows * base.obs_features, 2, device=DEV, **_hp(H)),
                      seed))
    calls = {"launch": [], "vector": 0}
    launch, vector = ppo_native.GroupAct.launch, routine._run_eval_vector

    def counted_launch(self, rows, tiles=None):
        calls["launch"].append((id(self), self.G, self.mixed))
        return launch(self, rows, tiles)

    def counted_vector(*a, **k):
        calls["vector"] += 1
        return vector(*a, **k)

    monkeypatch.setattr(ppo_native.GroupAct, "launch", counted_launch)
    monkeypatch.setattr(routine, "_run_eval_vector", counted_vector)
    many = routine.evaluate_many(items, num_episodes=5)
    assert calls["vector"] == 0 and calls["launch"], calls
    assert len({c[0] for c in calls["launch"]}) == 1                   # one GroupAct ...
    assert all(c[1:] == (3, True) for c in calls["launch"])            # ... of all three, mixed
    n = len(calls["launch"])
    again = routine.evaluate_many(items, num_episodes=5)               # memo hit: nothing runs
    assert again == many and len(calls["launch"]) == n and calls["vector"] == 0
    for (env, agent, seed), r in zip(items, many):
        env.unwrapped._eval_memo = None
        assert routine.evaluate(env, agent, num_episodes=5, exp_seed=seed) == r, seed
    assert calls["vector"] == 3
    for env, _, _ in items:
        env.close()
