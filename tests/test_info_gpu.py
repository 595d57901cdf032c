"""hwy_step_with_info / hwy_step_group_info (include/hwy.h) on the GPU: the info variant of the
step computes the plain step, its per-step outputs are the oracle's ego state and the four terms
of HighwayEnv._rewards exactly as they enter the reward, the per-episode sums equal a float32
host mirror through autoresets and a cut, the grouped launch equals each handle's own, and the
Python envs, the rollout and the training loops carry them up to the artifacts.

Shapes: 5 envs (a full workgroup of 4 and a partial one), 12-step episodes, 48 steps of
parity_util.policy_actions: with autoreset 20 crashes, 10 pure truncations and 46 steps that change
the ego's lane; with this file's masked re-resets (seeds 7000 + 100 t + e) 20 / 12 / 56.  Each
test that leans on these events asserts >= 5 of each."""

import ctypes
import functools
import os

import numpy as np
import pytest
import torch

from hwy import _abi
from hwy.native import check, lib, ptr
from oracle.oracle import OracleEnv
from parity_util import diff_state, make_cfg, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, STEPS, HORIZON = 5, 48, 12
f32 = np.float32


@functools.lru_cache(maxsize=None)
def _actions():
    rng = np.random.default_rng(0)
    return [policy_actions(rng, E, t) for t in range(STEPS)]


def _cfg(autoreset=True):
    return make_cfg(E=E, seed_base=42, max_episode_steps=HORIZON, autoreset=autoreset)


class _Hip:
    """The C ABI driven directly: hwy_step or hwy_step_with_info on one handle."""

    STEP_KEYS = ("obs", "rew", "term", "trunc", "er", "el")
    INFO_KEYS = ("speed", "crashed", "lane", "rewards", "acc", "ep_stats")

    def __init__(self, cfg):
        self.cfg, self.E = cfg, cfg.num_envs
        self.h = ctypes.c_void_p()
        check(lib().hwy_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "hwy_create")
        n = self.E
        self.obs = torch.zeros(n, cfg.obs_vehicles, cfg.obs_features(), device=DEV)
        self.rew = torch.zeros(n, device=DEV)
        self.term = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.trunc = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.er = torch.zeros(n, device=DEV)
        self.el = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.speed = torch.zeros(n, device=DEV)
        self.crashed = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.lane = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.rewards = torch.zeros(n, 4, device=DEV)
        # the sums must start from zero at a new episode whatever the buffer holds
        self.acc = torch.full((n, _abi.HWY_INFO_NACC), float("nan"), device=DEV)
        self.ep_stats = torch.full((n, _abi.HWY_INFO_NACC), float("nan"), device=DEV)
        self.cut = torch.zeros(n, dtype=torch.uint8, device=DEV)

    def reset(self, seeds=None, mask=None):
        s = None if seeds is None else torch.as_tensor(np.asarray(seeds, np.int64), device=DEV)
        m = None if mask is None else torch.as_tensor(np.asarray(mask, np.uint8), device=DEV)
        check(lib().hwy_reset(self.h, ptr(s), ptr(m), ptr(self.obs), None), "hwy_reset")
        torch.cuda.synchronize()

    def _out(self, keys):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in keys}

    def step(self, a):
        at = torch.as_tensor(a, device=DEV).contiguous()
        check(lib().hwy_step(self.h, ptr(at), ptr(self.obs), ptr(self.rew), ptr(self.term),
                             ptr(self.trunc), ptr(self.er), ptr(self.el), None), "hwy_step")
        return self._out(self.STEP_KEYS)

    def step_info(self, a):
        at = torch.as_tensor(a, device=DEV).contiguous()
        info = _abi.HwyStepInfo(*[ptr(getattr(self, k)) for k in self.INFO_KEYS])
        check(lib().hwy_step_with_info(self.h, ptr(at), ptr(self.obs), ptr(self.rew),
                                       ptr(self.term), ptr(self.trunc), ptr(self.er),
                                       ptr(self.el), ctypes.byref(info), None),
              "hwy_step_with_info")
        return self._out(self.STEP_KEYS + self.INFO_KEYS)

    def cut_episodes(self):
        check(lib().hwy_cut_episodes(self.h, ptr(self.obs), ptr(self.er), ptr(self.el),
                                     ptr(self.cut), None), "hwy_cut_episodes")
        return self._out(("cut", "acc"))

    def state(self):
        out = torch.zeros(_abi.NFIELDS, self.E, 64, dtype=torch.int32, device=DEV)
        check(lib().hwy_export_state(self.h, ptr(out), None), "export")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def ego_lane(self):
        return self.state()[_abi.F_LANE, :, 0].astype(np.int32)

    def close(self):
        lib().hwy_destroy(self.h)


def _values(out, lane_before):
    """One step's six accumulated values per env, [E, 6] float32."""
    changed = (out["lane"] != lane_before).astype(f32)
    return np.concatenate([out["speed"][:, None], out["rewards"], changed[:, None]],
                          axis=1).astype(f32)


def test_info_step_is_the_step():
    plain, info = _Hip(_cfg()), _Hip(_cfg())
    V = plain.cfg.vehicles_count + 1
    try:
        plain.reset()
        info.reset()
        dones = 0
        for t, a in enumerate(_actions()):
            p, i = plain.step(a), info.step_info(a)
            for k in _Hip.STEP_KEYS:
                np.testing.assert_array_equal(p[k], i[k], err_msg=f"{k} at step {t}")
            d = diff_state(info.state(), plain.state(), V)
            assert d is None, f"step {t}: {d}"
            dones += int((p["term"] | p["trunc"]).sum())
        assert dones >= 10  # autoresets happened on both sides
    finally:
        plain.close()
        info.close()


def test_per_step_values_against_the_oracle():
    cfg = _cfg(autoreset=False)
    hip, ora = _Hip(cfg), OracleEnv(cfg)
    cr, rl = f32(cfg.collision_reward), f32(cfg.right_lane_reward)
    hs, onr = f32(cfg.high_speed_reward), f32(cfg.on_road_reward)
    lo, hi = float(cfg.reward_speed_range[0]), float(cfg.reward_speed_range[1])
    assert cfg.lanes_count == 4 and (lo, hi) == (20.0, 30.0)
    crashes = truncs = changes = 0
    worst = 0.0
    try:
        hip.reset()
        ora.reset()
        for t, a in enumerate(_actions()):
            lane0 = ora.field(_abi.F_LANE)[:, 0].astype(np.int32)
            out = hip.step_info(a)
            _, rew, term, trunc, _, _ = ora.step(a)
            np.testing.assert_array_equal(out["rew"], rew, err_msg=f"reward at step {t}")
            speed = ora.ffield(_abi.F_SPEED)[:, 0]
            np.testing.assert_array_equal(out["speed"].view(np.uint32), speed.view(np.uint32),
                                          err_msg=f"speed at step {t}")
            flags = ora.field(_abi.F_FLAGS)[:, 0]
            np.testing.assert_array_equal(out["crashed"], (flags & 1).astype(np.uint8))
            lane = ora.field(_abi.F_LANE)[:, 0].astype(np.int32)
            np.testing.assert_array_equal(out["lane"], lane)
            r = out["rewards"]
            np.testing.assert_array_equal(r[:, 0], out["crashed"].astype(f32))
            np.testing.assert_array_equal(r[:, 1], lane.astype(f32) / f32(3))
            assert np.isin(r[:, 3], (0.0, 1.0)).all()
            # the reward recomposed from the reported terms, in the kernel's operation order
            rec = np.zeros(E, f32)
            rec = rec + cr * r[:, 0]
            rec = rec + rl * r[:, 1]
            rec = rec + hs * r[:, 2]
            rec = rec + onr * r[:, 3]
            if cfg.normalize_reward:  # hm_lmap(rew, collision, high_speed + right_lane, 0, 1)
                x0, x1, y0, y1 = cr, f32(hs + rl), f32(0), f32(1)
                rec = y0 + (rec - x0) * (y1 - y0) / (x1 - x0)
            rec = rec * r[:, 3]
            assert rec.dtype == f32
            np.testing.assert_array_equal(rec, out["rew"], err_msg=f"recomposed at step {t}")
            heading = ora.ffield(_abi.F_HEADING)[:, 0].astype(np.float64)
            want = np.clip((speed.astype(np.float64) * np.cos(heading) - lo) / (hi - lo), 0, 1)
            err = float(np.abs(r[:, 2].astype(np.float64) - want).max())
            worst = max(worst, err)
            # device cos within 1e-7 absolute at |speed| <= 40 -> 4e-6, one float32 rounding at 40
            # -> 2.4e-6; both / 10, rounded up
            assert err <= 2e-6, (t, err)
            crashes += int(term.sum())
            truncs += int((trunc & ~term).sum())
            changes += int((lane != lane0).sum())
            done = term | trunc
            if done.any():  # masked re-reset with explicit seeds, both sides
                seeds = (7000 + 100 * t + np.arange(E)).astype(np.uint64)
                hip.reset(seeds=seeds, mask=done)
                ora.reset(seeds=seeds, mask=done.astype(np.uint8))
        print(f"crashes {crashes} truncations {truncs} lane changes {changes} "
              f"high_speed worst error {worst:.3g}")
        assert crashes >= 5 and truncs >= 5 and changes >= 5
    finally:
        hip.close()


def test_episode_sums_equal_a_float32_host_mirror():
    hip = _Hip(_cfg())
    mirror = np.zeros((E, 6), f32)
    crashes = truncs = changes = 0
    try:
        hip.reset()
        for t, a in enumerate(_actions()):
            lane0 = hip.ego_lane()
            out = hip.step_info(a)
            vals = _values(out, lane0)
            mirror = mirror + vals
            assert mirror.dtype == f32
            done = (out["term"] | out["trunc"]).astype(bool)
            acc, es = out["acc"], out["ep_stats"]
            np.testing.assert_array_equal(acc[:, :6], mirror, err_msg=f"acc at step {t}")
            assert (acc[:, 6:] == 0).all()
            want = np.zeros((E, _abi.HWY_INFO_NACC), f32)
            want[done, :6] = mirror[done]
            want[done, 6] = out["crashed"][done]
            np.testing.assert_array_equal(es, want, err_msg=f"ep_stats at step {t}")
            np.testing.assert_array_equal(es[:, 6], out["term"].astype(f32))
            # the lane-change count is a count: the sum of the 0 / 1 flags, exactly
            assert (es[done, 5] == np.round(es[done, 5])).all()
            crashes += int(out["term"].sum())
            truncs += int((out["trunc"] & ~out["term"]).sum())
            changes += int(vals[:, 5].sum())
            mirror[done] = 0
        print(f"crashes {crashes} truncations {truncs} lane changes {changes}")
        assert crashes >= 5 and truncs >= 5 and changes >= 5
    finally:
        hip.close()


def test_cut_leaves_the_partial_sums_and_the_next_step_starts_from_zero():
    hip = _Hip(_cfg())
    mirror = np.zeros((E, 6), f32)
    try:
        hip.reset()
        for t in range(7):
            lane0 = hip.ego_lane()
            out = hip.step_info(_actions()[t])
            mirror = mirror + _values(out, lane0)
            mirror[(out["term"] | out["trunc"]).astype(bool)] = 0
        steps = hip.state()[_abi.F_ENV, :, _abi.E_STEP].astype(np.int32)
        c = hip.cut_episodes()
        cut = c["cut"].astype(bool)
        np.testing.assert_array_equal(cut, steps >= 1)
        assert cut.sum() >= 3
        np.testing.assert_array_equal(c["acc"][cut, :6], mirror[cut])
        assert (hip.state()[_abi.F_ENV, :, _abi.E_STEP] == 0).all()
        lane0 = hip.ego_lane()
        out = hip.step_info(_actions()[7])
        np.testing.assert_array_equal(out["acc"][:, :6], _values(out, lane0))
        assert (out["acc"][:, 6:] == 0).all()
    finally:
        hip.close()


def test_grouped_info_step_equals_each_handles_own_and_replays_from_a_graph():
    """Three handles (3 envs sorted; 5 envs shuffled RoPE; 6 envs RankPE in two seed groups) in
    one hwy_step_group_info launch against each handle's own hwy_step_with_info."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition
    from experiments.wrappers import make_env
    from hwy.vec_env import GroupEnvStep, alloc_step_info
    from utils.graphs import capture
    from utils.reproducibility import set_random_seeds

    specs = [(Condition.SORTED, None, 3, {}, None),
             (Condition.SHUFFLED_ROPE, 4, 5, {"observation": {"order": "shuffled"}}, None),
             (Condition.SHUFFLED_RANKPE, 4, 6, {}, [5, 900])]

    def make_set():
        envs = []
        for i, (cond, d, n, ov, groups) in enumerate(specs):
            set_random_seeds(1000 + i)  # RankPE draws its table from the global RNG
            env = make_env(cond, HIGHWAY_CONFIG, d_embed=d,
                           env_overrides=dict(ov, num_envs=n, device=DEV, autoreset=True,
                                              max_episode_steps=HORIZON))
            if hasattr(env, "to"):
                env = env.to(DEV)
            base = env.unwrapped
            if groups:
                base.set_seed_groups(groups, n // len(groups))
            else:
                base.set_seed_schedule(31 + i)
            env.reset()
            envs.append(base)
        return envs

    def bufs(env):
        n = env.num_envs
        io = (torch.zeros(n, 2, device=DEV), torch.zeros_like(env.obs_buf),
              torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
              torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, device=DEV),
              torch.zeros(n, dtype=torch.int32, device=DEV))
        return io, alloc_step_info(n, DEV)

    solo, grouped = make_set(), make_set()
    try:
        gstep = GroupEnvStep(grouped)
        bs, bg = [bufs(e) for e in solo], [bufs(e) for e in grouped]
        rng = np.random.default_rng(0)
        dones = 0

        def set_actions(t):
            for (a, _), (b, _) in zip(bs, bg):
                x = torch.as_tensor(policy_actions(rng, a[0].shape[0], t), device=DEV)
                a[0].copy_(x)
                b[0].copy_(x)

        def compare(what):
            n = 0
            torch.cuda.synchronize()
            for i, ((a, ai), (b, bi)) in enumerate(zip(bs, bg)):
                for k in range(1, 7):
                    assert torch.equal(a[k], b[k]), (what, i, k)
                for k in ai:
                    assert torch.equal(ai[k], bi[k]), (what, i, k)
                n += int((a[3] | a[4]).sum())
            return n

        for t in range(24):
            set_actions(t)
            for env, (a, ai) in zip(solo, bs):
                env.step_into(*a, info=ai)
            gstep.launch([b for b, _ in bg], infos=[bi for _, bi in bg])
            dones += compare(f"step {t}")
        assert dones >= 5
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                gstep.launch([b for b, _ in bg], infos=[bi for _, bi in bg])
        torch.cuda.current_stream().wait_stream(s)
        for t in range(24, 28):
            set_actions(t)
            for env, (a, ai) in zip(solo, bs):
                env.step_into(*a, info=ai)
            g.replay()
            compare(f"replay {t}")
        for x, y in zip(solo, grouped):
            assert torch.equal(x.export_state(), y.export_state())
    finally:
        for env in solo + grouped:
            env.close()


def test_python_envs_report_the_info():
    from config.base_config import HIGHWAY_CONFIG
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv

    cfg = dict(HIGHWAY_CONFIG, max_episode_steps=HORIZON)
    on = HighwayVecEnv(cfg, num_envs=E, device=DEV, seed_base=42, info=True)
    off = HighwayVecEnv(cfg, num_envs=E, device=DEV, seed_base=42)
    one = HighwayVecEnv(cfg, num_envs=1, device=DEV, autoreset=False, info=True)
    single = HighwayEnv(cfg, device=DEV, info=True)
    plain_single = HighwayEnv(cfg, device=DEV)
    try:
        on.reset()
        off.reset()
        a = torch.as_tensor(_actions()[0], device=DEV)
        o1, r1, te1, tr1, i1 = on.step(a)
        o0, r0, te0, tr0, i0 = off.step(a)
        assert sorted(i0) == ["episode_length", "episode_return"]
        assert sorted(i1) == ["crashed", "episode_length", "episode_return", "episode_stats",
                              "lane", "rewards", "speed"]
        assert torch.equal(o1, o0) and torch.equal(r1, r0)
        assert i1["speed"].shape == (E,) and i1["speed"].dtype == torch.float32
        assert i1["crashed"].shape == (E,) and i1["crashed"].dtype == torch.uint8
        assert i1["lane"].shape == (E,) and i1["lane"].dtype == torch.int32
        assert list(i1["rewards"]) == ["collision_reward", "right_lane_reward",
                                       "high_speed_reward", "on_road_reward"]
        assert all(v.shape == (E,) for v in i1["rewards"].values())
        assert i1["episode_stats"].shape == (E, 8)
        assert bool((i1["speed"] > 0).all())

        single.reset(seed=77)
        plain_single.reset(seed=77)
        one.reset(seeds=torch.tensor([77]))
        for t in range(HORIZON):
            act = _actions()[t][0]
            _, r, te, tr, info = single.step(act)
            assert plain_single.step(act)[4] == {}
            _, vr, _, _, vi = one.step(torch.as_tensor(act.reshape(1, 2), device=DEV))
            assert sorted(info) == ["action", "crashed", "rewards", "speed"]
            assert type(info["speed"]) is float and type(info["crashed"]) is bool
            assert isinstance(info["action"], np.ndarray) and info["action"].shape == (2,)
            np.testing.assert_array_equal(info["action"], act)
            assert sorted(info["rewards"]) == sorted(i1["rewards"])
            assert all(type(v) is float for v in info["rewards"].values())
            assert info["speed"] == float(vi["speed"][0]) and r == float(vr[0])
            assert info["crashed"] == bool(vi["crashed"][0]) == te
            for k, v in info["rewards"].items():
                assert v == float(vi["rewards"][k][0]), k
            if te or tr:
                break
    finally:
        for env in (on, off, one, single, plain_single):
            env.close()


# ------------------------------------------------------------------------------- training
def _exp(seed, schedule, stats, name):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps
    extra = {"num_envs": 4, "eval_interval": 4, "log_interval": 50}
    if schedule != "lockstep":
        extra["episode_schedule"] = schedule
    if stats:
        extra["episode_stats"] = True
    return Experiment(name=f"{name}_{schedule}_{seed}", condition=Condition.SORTED, hp=hp,
                      seed=seed, max_episodes=12, target_reward=1e9, extra=extra,
                      env_config_overrides={"max_episode_steps": HORIZON})


_RUNS = {}


def _run(tmp, schedule, seeds, stats):
    """launch (one seed) or launch_group (several) once per key; the status dicts, each with the
    final weights of its agent."""
    from config.base_config import HIGHWAY_CONFIG
    from experiments.runner import ExperimentRunner

    key = (schedule, tuple(seeds), stats)
    if key in _RUNS:
        return _RUNS[key]
    agents = []

    class Runner(ExperimentRunner):
        def _create_agent(self, *a, **kw):
            agents.append(super()._create_agent(*a, **kw))
            return agents[-1]

    name = f"{'g' if len(seeds) > 1 else 's'}{int(stats)}"
    exps = [_exp(s, schedule, stats, name) for s in seeds]
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        r = Runner(HIGHWAY_CONFIG)
        res = r.launch_group(exps) if len(seeds) > 1 else [r.launch(exps[0])]
    finally:
        os.chdir(cwd)
    torch.cuda.synchronize()
    for x, ag, e in zip(res, agents, exps):
        assert x["status"] == "COMPLETED", x.get("error_message")
        x["weights"] = [p.detach().clone() for p in ag.actor_critic.parameters()]
        x["summary"] = open(os.path.join(tmp, "artifacts", "highway-ppo",
                                         f"summary_{e.name}.csv")).read().splitlines()
    _RUNS[key] = res
    return res


STATS = ("episode_lengths", "episode_crashed", "episode_mean_speed", "episode_lane_changes")


@pytest.fixture(scope="module")
def run_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("info_runs"))


@pytest.mark.parametrize("schedule", ["lockstep", "reference"])
def test_training_with_episode_stats_is_the_same_training(run_dir, schedule):
    from training.routine import crash_rate

    on = _run(run_dir, schedule, [42], True)[0]
    off = _run(run_dir, schedule, [42], False)[0]
    mh, m0 = on["metrics_history"], off["metrics_history"]
    assert not any(k in m0 for k in STATS)
    assert off["summary"][0] == "experiment,final_reward,max_reward,steps,best_model,plot"
    assert mh["episode_rewards"] == m0["episode_rewards"] and len(mh["episode_rewards"]) == 12
    assert on["rewards"] == off["rewards"] and on["avg_rewards"] == off["avg_rewards"]
    assert mh["eval_rewards"] == m0["eval_rewards"]
    assert [u["loss"] for u in mh["policy_updates"]] == [u["loss"] for u in m0["policy_updates"]]
    assert all(torch.equal(a, b) for a, b in zip(on["weights"], off["weights"]))
    n = len(mh["episode_rewards"])
    assert all(len(mh[k]) == n for k in STATS)
    cut = 0
    for r, length, crashed, speed, changes in zip(mh["episode_rewards"], *(mh[k] for k in STATS)):
        assert type(length) is int and type(crashed) is bool and type(changes) is int
        assert type(speed) is float and 0.0 < speed <= 41.0
        assert 1 <= length <= HORIZON and 0 <= changes <= length
        assert 0.0 <= r <= length  # a normalised step reward lies in [0, 1]
        if not crashed and length < HORIZON:
            cut += 1  # neither crashed nor truncated: cut at the update boundary
    if schedule == "reference":
        assert cut >= 1
    else:
        assert cut == 0
    assert on["summary"][0].endswith(",plot,crash_rate")
    assert float(on["summary"][1].rsplit(",", 1)[1]) == pytest.approx(
        crash_rate(mh["episode_crashed"]), abs=5e-5)


@pytest.mark.parametrize("schedule", ["lockstep", "reference"])
def test_launch_group_books_each_seeds_solo_stats(run_dir, schedule):
    seeds = [42, 1042]
    grouped = _run(run_dir, schedule, seeds, True)
    for s, g in zip(seeds, grouped):
        solo = _run(run_dir, schedule, [s], True)[0]
        ms, mg = solo["metrics_history"], g["metrics_history"]
        for k in ("episode_rewards", "eval_rewards") + STATS:
            assert ms[k] == mg[k], (s, k)
        assert all(torch.equal(a, b) for a, b in zip(solo["weights"], g["weights"])), s
        assert solo["summary"][1].rsplit(",", 1)[1] == g["summary"][1].rsplit(",", 1)[1]
