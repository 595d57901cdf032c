"""Grouped PPO launches with learners whose state rows are wider than 256 floats (S <= 1,024):
hwy_ppo_group_*, hwy_ppo_mixed_*, hwy_ppo_sched_* and their acting calls with wide learners,
alone and beside narrow ones, and a RankPE d_embed 16 cell (S 300) through build_group.  A table
that holds a wide learner runs the chunked kernels for every learner of the launch; they are the
solo kernels' bodies, so every comparison here is bit equality with the learner run alone by the
same library -- no tolerance."""

import ctypes

import pytest
import torch

import test_sched_group_gpu as sg  # the seeded learners of the grouped-step tests

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
UPDATES = 2  # whole updates (epochs x minibatches each) before anything is compared


class _Learner(sg._Learner):
    """sg._Learner with metrics rows for UPDATES updates (counters[1] runs on across them)."""

    def __init__(self, H, S, B, nmb, epochs):
        super().__init__(H, S, B, nmb, epochs)
        self.metrics = torch.zeros(UPDATES * self.steps, 6, device=DEV)
        d = self.dims
        self.tile_off = int(sg._lib().hwy_ppo_tile_image_offset(ctypes.byref(d)))
        assert self.tile_off >= 0

    def snapshot(self):
        out = {k: v.clone() for k, v in self.state().items()}
        out["tile_image"] = self.workspace[self.tile_off:].clone()
        return out


def _solo(spec):
    L, lr = sg._lib(), _Learner(*spec)
    for _ in range(UPDATES * lr.epochs):
        for i in range(lr.nmb):
            a = lr.args(i)
            assert L.hwy_ppo_forward_backward(ctypes.byref(a), sg._stream()) == 0
            assert L.hwy_ppo_optimizer(ctypes.byref(a), sg._stream()) == 0
    torch.cuda.synchronize()
    return lr.snapshot()


def _assert_equal_solo(specs, learners):
    for spec, l in zip(specs, learners):
        want, got = _solo(spec), l.snapshot()
        assert int(l.counters[0]) == int(l.counters[1]) == UPDATES * l.steps, spec
        for k in want:
            assert torch.equal(got[k], want[k]), (spec, k)
        assert bool(torch.isfinite(l.metrics).all()) and bool((l.flat != l.st["flat"]).any())
        assert bool((l.metrics[-1] != 0).any())


def _arr(ls, i):
    from hwy.ppo_native import PpoArgs

    arr = (PpoArgs * len(ls))()
    for g, l in enumerate(ls):
        a = l.args(i)
        ctypes.memmove(ctypes.byref(arr[g]), ctypes.byref(a), ctypes.sizeof(PpoArgs))
    return arr


def test_group_step_with_a_narrow_and_a_wide_learner_equals_solo_steps():
    """hwy_ppo_group_*: S 60 and S 360 at H 256 in one table; the row launch runs the chunked
    kernel for both (HWY_PPO_PLAN_WIDE in grid_rows), the narrow learner at one chunk."""
    from hwy.ppo_native import PpoGroupPlan

    L = sg._lib()
    B, nmb, epochs = 40, 2, 1
    specs = [(256, 60, B, nmb, epochs), (256, 360, B, nmb, epochs)]
    ls = [_Learner(*s) for s in specs]
    nb = L.hwy_ppo_group_table_bytes(ctypes.byref(ls[1].dims), len(ls))
    assert nb > 0
    tables, plans = [], []
    for i in range(nmb):
        t = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
        plan = PpoGroupPlan()
        assert L.hwy_ppo_group_prepare(_arr(ls, i), len(ls), t.data_ptr(), ctypes.byref(plan),
                                       sg._stream()) == 0
        assert plan.grid_rows == (1 << 30) | ((B + 15) // 16)
        tables.append(t)
        plans.append(plan)
    for _ in range(UPDATES * epochs):
        for t, plan in zip(tables, plans):
            assert L.hwy_ppo_group_step(ctypes.byref(plan), t.data_ptr(), sg._stream()) == 0
    torch.cuda.synchronize()
    assert sg._launches_issued(lambda st: L.hwy_ppo_group_step(
        ctypes.byref(plans[0]), tables[0].data_ptr(), st)) == 4
    _assert_equal_solo(specs, ls)


def test_mixed_step_with_wide_learners_equals_solo_steps():
    """hwy_ppo_mixed_*: (S, H) (300, 128), (600, 256), (120, 320) -- two wide learners of the
    8-wave class and a narrow one of the 4-wave class, whose launch stays the narrow kernel."""
    from hwy.ppo_native import PpoDims, PpoMixedPlan

    L = sg._lib()
    B, nmb, epochs = 40, 2, 1
    specs = [(128, 300, B, nmb, epochs), (256, 600, B, nmb, epochs), (320, 120, B, nmb, epochs)]
    ls = [_Learner(*s) for s in specs]
    G = len(ls)
    nb = L.hwy_ppo_mixed_table_bytes((PpoDims * G)(*[l.dims for l in ls]), G)
    assert nb > 0
    tables, plans = [], []
    for i in range(nmb):
        t = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
        plan = PpoMixedPlan()
        assert L.hwy_ppo_mixed_prepare(_arr(ls, i), G, t.data_ptr(), ctypes.byref(plan),
                                       sg._stream()) == 0
        assert plan.launches == 5 and plan.present[0] == 2 and plan.present[1] == 1
        assert plan.grid_rows[0] == (1 << 30) | 3 and plan.grid_rows[1] == 3
        tables.append(t)
        plans.append(plan)
    for _ in range(UPDATES * epochs):
        for t, plan in zip(tables, plans):
            assert L.hwy_ppo_mixed_step(ctypes.byref(plan), t.data_ptr(), sg._stream()) == 0
    torch.cuda.synchronize()
    assert sg._launches_issued(lambda st: L.hwy_ppo_mixed_step(
        ctypes.byref(plans[0]), tables[0].data_ptr(), st)) == 5
    _assert_equal_solo(specs, ls)


def test_sched_steps_with_wide_learners_equal_solo_updates():
    """hwy_ppo_sched_*: two wide learners that differ in B and epochs (and in H and S)."""
    from hwy.ppo_native import PpoDims, PpoSchedPlan

    L = sg._lib()
    specs = [(256, 300, 32, 2, 2), (128, 600, 40, 3, 1)]
    ls = [_Learner(*s) for s in specs]
    G = len(ls)
    nmb = (ctypes.c_int32 * G)(*[l.nmb for l in ls])
    epochs = (ctypes.c_int32 * G)(*[l.epochs for l in ls])
    nb = L.hwy_ppo_sched_table_bytes((PpoDims * G)(*[l.dims for l in ls]), nmb, G)
    assert nb > 0
    table = torch.empty(int(nb), dtype=torch.uint8, device=DEV)
    p = PpoSchedPlan()
    assert L.hwy_ppo_sched_prepare(_arr(ls, 0), nmb, epochs, G, table.data_ptr(), ctypes.byref(p),
                                   sg._stream()) == 0
    assert p.max_steps == 4 and p.present[0] == 2 and p.present[1] == 0 and p.launches == 4
    assert p.grid_rows[0] == (1 << 30) | 3
    for _ in range(UPDATES):
        assert L.hwy_ppo_sched_begin(ctypes.byref(p), table.data_ptr(), sg._stream()) == 0
        for slot in range(p.max_steps):
            assert L.hwy_ppo_sched_step(ctypes.byref(p), table.data_ptr(), slot,
                                        sg._stream()) == 0
    torch.cuda.synchronize()
    assert sg._launches_issued(lambda st: L.hwy_ppo_sched_step(
        ctypes.byref(p), table.data_ptr(), 0, st)) == 4
    _assert_equal_solo(specs, ls)


@pytest.mark.parametrize("stochastic", [True, False])
@pytest.mark.parametrize("with_tiles", [True, False])
def test_grouped_and_mixed_act_with_wide_learners_equal_solo_act(stochastic, with_tiles):
    """hwy_ppo_group_act (S 60 and 360 at H 256) and hwy_ppo_mixed_act ((300, 128), (600, 256),
    (120, 320)) against hwy_ppo_act per learner: 5 rows, a partial tile."""
    from hwy.ppo_native import PpoActArgs, PpoDims, PpoMixedActPlan
    from test_mixed_group_gpu import _tile_image

    L = sg._lib()
    rows = 5

    def build(learners):
        G = len(learners)
        keep, arr, solo_out, grp_out = [], (PpoActArgs * G)(), [], []
        for g, (H, S) in enumerate(learners):
            st = sg._start(H, S)
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
                    assert L.hwy_ppo_act(ctypes.byref(a), sg._stream()) == 0
            solo_out.append(outs[0])
            grp_out.append(outs[1])
        return keep, arr, solo_out, grp_out

    def compare(learners, solo_out, grp_out):
        torch.cuda.synchronize()
        for (H, S), so, mo in zip(learners, solo_out, grp_out):
            for name, a, b in zip(("action", "pre_tanh", "logp", "value"), so, mo):
                assert torch.equal(a, b), (H, S, name)
            assert bool((so[3] != 7.0).all())

    same_h = [(256, 60), (256, 360)]
    keep, arr, solo_out, grp_out = build(same_h)
    table = torch.empty(int(L.hwy_ppo_group_act_table_bytes(2)), dtype=torch.uint8, device=DEV)
    assert L.hwy_ppo_group_act_prepare(arr, 2, table.data_ptr(), sg._stream()) == 0
    d = PpoDims(rows, 360, 256, 2)  # the shared B and H, the widest learner's S
    assert L.hwy_ppo_group_act(ctypes.byref(d), 2, int(with_tiles), table.data_ptr(),
                               sg._stream()) == 0
    compare(same_h, solo_out, grp_out)

    mixed = [(128, 300), (256, 600), (320, 120)]
    keep2, arr, solo_out, grp_out = build(mixed)
    table = torch.empty(int(L.hwy_ppo_mixed_act_table_bytes(3)), dtype=torch.uint8, device=DEV)
    plan = PpoMixedActPlan()
    assert L.hwy_ppo_mixed_act_prepare(arr, 3, table.data_ptr(), ctypes.byref(plan),
                                       sg._stream()) == 0
    assert plan.launches == 2 and plan.lds_bytes[0] & (1 << 30) and not plan.lds_bytes[1] & (1 << 30)
    assert L.hwy_ppo_mixed_act(ctypes.byref(plan), table.data_ptr(), sg._stream()) == 0
    compare(mixed, solo_out, grp_out)


def _hp(H):
    return dict(lr=3e-4, epochs=2, batch_size=16, hidden_dim=H)


def _solo_experiment(cond, d, seed, E, T, iters, H):
    """One experiment alone: the runner's construction and _train_vector's loop, as
    tests/test_group_gpu.py runs it (here with 16-row minibatches of the 32-row rollout)."""
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
    agent = PPOAgent(sd, 2, device=DEV, **_hp(H))
    base.set_seed_schedule(seed)
    obs, _ = env.reset()
    buf = RolloutBuffer(T, E, sd, 2, DEV)
    buf.states[0].copy_(obs.reshape(E, sd))
    roll = LockstepRollout(agent, base, buf)
    hist, metrics = [], []
    for _ in range(iters):
        roll.run()
        hist.append({k: getattr(buf, k).clone() for k in ("states", "actions", "rewards", "dones",
                                                          "log_probs", "values")})
        metrics.append(agent.update_rollout(buf, agent.value(buf.states[T])))
        buf.states[0].copy_(buf.states[T])
    torch.cuda.synchronize()
    return agent, hist, metrics, env


def test_rankpe_d16_group_matches_solo_runs_bit_for_bit():
    """build_group(SHUFFLED_RANKPE, d_embed=16): S = 15 x (4 + 16) = 300.  Two iterations of the
    grouped rollout (GroupAct) and update (GroupStep) equal two solo runs: rollout buffers,
    weights, Adam moments, metrics."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from ppo.agent import PPOAgent
    from ppo.group import build_group

    cond, d, H = Condition.SHUFFLED_RANKPE, 16, 256
    seeds, E, T, iters = [42, 1042], 4, 8, 2
    grp = build_group(cond, HIGHWAY_CONFIG, seeds, E, T, DEV,
                      lambda sd: PPOAgent(sd, 2, device=DEV, **_hp(H)), d_embed=d)
    assert grp.sd == 300
    ghist, gmet = [], []
    for _ in range(iters):
        grp.rollout()
        b = grp.buf
        ghist.append({k: getattr(b, k).clone() for k in ("states", "actions", "rewards", "dones",
                                                         "log_probs", "values")})
        gmet.append(grp.update())
    torch.cuda.synchronize()
    F0 = grp.agents[0]._fused
    assert F0 is not None and F0.mb == 16 and F0._tile_off is not None
    for g, s in enumerate(seeds):
        agent, hist, metrics, env = _solo_experiment(cond, d, s, E, T, iters, H)
        assert agent._fused is not None and agent._fused._tile_off is not None
        sl = slice(g * E, (g + 1) * E)
        for it in range(iters):
            for k, v in hist[it].items():
                assert torch.equal(ghist[it][k][:, sl], v), (g, it, k)
            assert gmet[it][g] == metrics[it], (g, it)
        for (k, va), (_, vb) in zip(agent.actor_critic.state_dict().items(),
                                    grp.agents[g].actor_critic.state_dict().items()):
            assert torch.equal(va, vb), (g, k)
        Fs, Fg = agent._fused, grp.agents[g]._fused
        assert torch.equal(Fs.m, Fg.m) and torch.equal(Fs.v, Fg.v), g
        assert int(Fs.counters[0]) == int(Fg.counters[0]) == iters * 2 * (T * E // 16)
        env.close()
    grp.close()


def test_runner_launch_group_trains_a_rankpe_d16_cell(tmp_path, monkeypatch):
    """ExperimentRunner.launch_group on a RankPE d_embed 16 cell (S 300): it completes on the
    fused paths and returns, per experiment, what launch() returns for it alone."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner
    from hwy import ppo_native

    monkeypatch.chdir(tmp_path)
    seen = {"group_act": 0, "group_step": 0}
    launch, step = ppo_native.GroupAct.launch, ppo_native.GroupStep.step

    def counted_launch(self, rows, tiles=None):
        seen["group_act"] += int(max(self.S) == 300)
        return launch(self, rows, tiles)

    def counted_step(self, i):
        seen["group_step"] += int(all(F.S == 300 and F._tile_off is not None for F in self.fused))
        return step(self, i)

    monkeypatch.setattr(ppo_native.GroupAct, "launch", counted_launch)
    monkeypatch.setattr(ppo_native.GroupStep, "step", counted_step)

    def exp(seed):
        hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=64, hidden_dim=256,
                         d_embed=16)
        hp.entropy_coef = 0.005
        hp.steps_per_update = 16 * 32
        return Experiment(name=f"wide_rank_seed{seed}", condition=Condition.SHUFFLED_RANKPE,
                          hp=hp, seed=seed, max_episodes=24, target_reward=1e9,
                          extra={"num_envs": 16, "num_minibatches": 8, "eval_interval": 8,
                                 "log_interval": 50}, env_config_overrides={})

    seeds = [42, 1042]
    grouped = ExperimentRunner(HIGHWAY_CONFIG).launch_group([exp(s) for s in seeds])
    assert seen["group_act"] > 0 and seen["group_step"] > 0, seen
    for s, g in zip(seeds, grouped):
        solo = ExperimentRunner(HIGHWAY_CONFIG).launch(exp(s))
        assert solo["status"] == g["status"] == "COMPLETED", (solo.get("error_message"),
                                                              g.get("error_message"))
        assert g["rewards"] == solo["rewards"] and g["avg_rewards"] == solo["avg_rewards"], s
        mg, ms = g["metrics_history"], solo["metrics_history"]
        assert mg["episode_rewards"] == ms["episode_rewards"]
        assert [u["loss"] for u in mg["policy_updates"]] == [u["loss"] for u in ms["policy_updates"]]
        assert len(mg["policy_updates"]) > 0
