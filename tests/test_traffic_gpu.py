"""hwy_traffic on the device: natural runs and crafted states against tests/traffic_model.py, the
deliberate mistakes, the structural guarantees (state untouched, outputs not given not written,
every refusal, graph capture), the per-episode reduction against a numpy fold of the kernel's own
per-state outputs, and the Python surface.

Every launch of the kernel-level tests writes into ONE allocation that holds all the outputs side
by side between guard words: an output that was not asked for has to keep its fill."""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest
import torch

import traffic_model as tm
import traffic_util as tu
from config.base_config import HIGHWAY_CONFIG
from env_util import HipEnv
from hwy import _abi
from parity_util import make_cfg, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64
CANARY = 0x5A5AA5A5
FILL = 0x7FC12345          # a NaN pattern no output holds
VEH = _abi.TRAFFIC_VEHICLE_OUTPUTS
ALL = VEH + ("ego", "acc", "ep_stats")
WIDTH = dict({k: 64 for k in VEH}, ego=16, acc=8, ep_stats=8)


class Arena:
    """all of hwy_traffic's outputs for E envs in one allocation, guard words between them"""

    def __init__(self, E):
        self.E = E
        self.off, n = {}, GUARD
        for k in ALL:
            self.off[k] = n
            n += E * WIDTH[k] + GUARD
        self.buf = torch.full((n,), CANARY, dtype=torch.int32, device=DEV)
        for k in ALL:
            self.words(k).fill_(FILL)
        self.words("acc").zero_()

    def words(self, k):
        return self.buf[self.off[k]:self.off[k] + self.E * WIDTH[k]]

    def numpy(self, k):
        w = self.words(k).cpu().numpy().reshape(self.E, WIDTH[k])
        return w if k in ("front", "rear") else w.view(np.float32)

    def check(self, given):
        b = self.buf.cpu().numpy()
        inside = np.zeros(len(b), bool)
        for k in ALL:
            lo, hi = self.off[k], self.off[k] + self.E * WIDTH[k]
            inside[lo:hi] = True
            if k not in given and k != "acc":
                assert (b[lo:hi] == FILL).all(), f"{k} was not given and was written"
            elif k in given:
                assert not (b[lo:hi] == FILL).any(), f"{k}: an entry was left unwritten"
        assert (b[~inside] == CANARY).all(), "a word outside the outputs was written"


def traffic(hip, outs=ALL[:8], arena=None, restart=(), **thresholds):
    """one hwy_traffic launch on a HipEnv's handle through the C ABI; numpy results by name"""
    from hwy.native import check, lib

    arena = arena or Arena(hip.E)
    a = _abi.TrafficArgs()
    for k in outs:
        setattr(a, k, arena.words(k).data_ptr())
    masks = [torch.as_tensor(np.asarray(m, np.uint8), device=DEV) for m in restart]
    for k, m in enumerate(masks):
        a.restart[k] = m.data_ptr()
    for k, v in dict(_abi.TRAFFIC_DEFAULTS, **thresholds).items():
        setattr(a, k, v)
    check(lib().hwy_traffic(hip.h, ctypes.byref(a), None), "hwy_traffic")
    torch.cuda.synchronize()
    arena.check(outs)
    return {k: arena.numpy(k) for k in outs}


def check_against_model(cfg, state, got, what, **thresholds):
    m = tm.traffic_model(cfg, state, **thresholds)
    bad = tm.compare(m, got, what + ": ")
    assert not bad, "\n".join(bad)
    return m


# ------------------------------------------------------------------- 1. natural runs
@pytest.mark.parametrize("name", list(tu.NATURAL))
def test_natural_run_matches_the_model_at_every_step(name):
    cfg = tu.natural_cfg(name)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        und = present = resets = 0
        for t, a in enumerate([None] + tu.actions(name)):
            if a is not None:
                out = hip.step(a)
                resets += int((out[2] | out[3]).sum())
            before = hip.state()
            got = traffic(hip)
            assert np.array_equal(before, hip.state()), f"step {t}: the call changed the state"
            m = check_against_model(cfg, before, got, f"{name} step {t}")
            und += int(((m["und"]["ttc"] | m["und"]["thw"] | m["und"]["risk"]) & m["present"]).sum())
            present += int(m["present"].sum())
        assert resets > 0, "no autoreset happened"
        assert und <= 0.01 * present, f"{und} of {present} entries undecided"
    finally:
        hip.close()


# ------------------------------------------------------------------- 2. crafted states
@pytest.fixture(scope="module")
def crafted():
    cfg = tu.craft_cfg()
    st = tu.craft(cfg)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(st)
        got = traffic(hip)
        assert np.array_equal(hip.state(), st)
    finally:
        hip.close()
    return cfg, st, got


def test_crafted_states(crafted):
    cfg, st, got = crafted
    tu.check_crafted(got["front"], got["rear"], got["gap"], got["ego"])
    m = check_against_model(cfg, st, got, "crafted")
    assert not any(m["und"][k].any() for k in ("ttc", "thw", "risk"))
    # absent slots and lanes past the vehicles hold the "none" values
    gone = ~m["present"]
    assert (got["front"][gone] == -1).all() and (got["rear"][gone] == -1).all()
    assert (got["gap"][gone] == np.inf).all() and (got["ttc"][gone] == np.inf).all()
    assert (got["thw"][gone] == np.inf).all()
    assert not got["closing"][gone].any() and not got["risk"][gone].any()
    assert ((got["risk"] >= 0) & (got["risk"] <= 1)).all()


@pytest.fixture(scope="module")
def sampled():
    """(name, cfg, state, outputs) of the crafted states and of a few natural ones"""
    out = []
    for name in ("E16-default", "E16-1lane", "E5-8lanes-63cars"):
        cfg = tu.natural_cfg(name)
        hip = HipEnv(cfg)
        try:
            hip.reset()
            for t, a in enumerate(tu.actions(name)[:17]):
                hip.step(a)
                if t % 4 == 0:
                    out.append((name, cfg, hip.state(), traffic(hip)))
        finally:
            hip.close()
    return out


@pytest.mark.parametrize("mistake", list(tu.MISTAKES))
def test_each_deliberate_mistake_in_the_model_fails_a_case(crafted, sampled, mistake):
    kw = tu.MISTAKES[mistake]
    thresholds = {k: v for k, v in kw.items() if k != "consts"}
    failed = []
    for name, cfg, st, got in [("crafted",) + crafted] + sampled:
        assert not tm.compare(tm.traffic_model(cfg, st), got), name
        if tm.compare(tm.traffic_model(cfg, st, kw.get("consts"), **thresholds), got):
            failed.append(name)
    assert failed, f"'{mistake}' in the model agrees with the kernel on every case"


def test_thresholds_reach_the_kernel():
    cfg = tu.natural_cfg("E16-default")
    hip = HipEnv(cfg)
    try:
        hip.reset()
        for a in tu.actions("E16-default")[:6]:
            hip.step(a)
        st = hip.state()
        for th in (dict(risk_horizon=9.5, near_range=17.0), dict(risk_horizon=0.75, near_range=140.0)):
            check_against_model(cfg, st, traffic(hip, **th), str(th), **th)
    finally:
        hip.close()


# ------------------------------------------------------------------- 3. structure
def test_an_output_not_given_is_not_written():
    cfg = tu.natural_cfg("E5-dt5")
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.step(policy_actions(np.random.default_rng(2), 5, 0))
        full = traffic(hip, ALL[:8])
        n = 0
        for k in ALL[:9]:                               # each output alone (acc alone included)
            part = traffic(hip, (k,))
            n += 1
            if k != "acc":
                assert np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)), k
        for outs in (("front", "risk"), ("gap", "ego"), ("ego", "acc"), ("ego", "acc", "ep_stats"),
                     ("rear", "closing", "ttc", "thw"), ALL):
            part = traffic(hip, outs)
            n += 1
            for k in outs:
                if k in full:
                    assert np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)), (outs, k)
        assert n == 15
    finally:
        hip.close()


def test_refusals_come_before_any_device_call():
    from hwy.native import HWY_EINVAL, last_error, lib

    cfg = make_cfg(E=3)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        before = hip.state()
        arena = Arena(3)
        ok = dict(_abi.TRAFFIC_DEFAULTS)
        cases = [({}, ok, (), "no output"), ({"ep_stats"}, ok, (), "no output"),
                 ({"ego", "ep_stats"}, ok, (), "ep_stats needs acc"),
                 ({"ego"}, ok, (0,), "restart[0] needs acc"), ({"gap"}, ok, (2,), "restart[2] needs acc")]
        for name in ok:
            for bad in (0.0, -1.0, float("inf"), float("nan")):
                cases.append(({"ego"}, dict(ok, **{name: bad}), (), name))
        mask = torch.ones(3, dtype=torch.uint8, device=DEV)
        for outs, th, rs, word in cases:
            a = _abi.TrafficArgs()
            for k in outs:
                setattr(a, k, arena.words(k).data_ptr())
            for k in rs:
                a.restart[k] = mask.data_ptr()
            for k, v in th.items():
                setattr(a, k, v)
            assert lib().hwy_traffic(hip.h, ctypes.byref(a), None) == HWY_EINVAL, word
            assert word in last_error()
        assert lib().hwy_traffic(hip.h, None, None) == HWY_EINVAL
        torch.cuda.synchronize()
        arena.check(())
        assert np.array_equal(before, hip.state())
    finally:
        hip.close()


def _vec(E, autoreset=True, **kw):
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(kw)
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=autoreset, seed_base=5)


def test_python_argument_errors_are_value_errors():
    from hwy.vec_env import alloc_traffic

    env = _vec(3)
    try:
        env.reset()
        t = alloc_traffic(3, DEV)
        env.traffic_into(**t)
        with pytest.raises(ValueError, match="at least one output"):
            env.traffic_into()
        with pytest.raises(ValueError, match="ep_stats needs acc"):
            env.traffic_into(ego=t["ego"], ep_stats=t["ep_stats"])
        with pytest.raises(ValueError, match="restart masks need acc"):
            env.traffic_into(ego=t["ego"], restart=(torch.zeros(3, dtype=torch.uint8, device=DEV),))
        with pytest.raises(ValueError, match=r"^restart\[0\] must be"):
            env.traffic_into(acc=t["acc"], restart=(torch.zeros(3, dtype=torch.uint8),))
        with pytest.raises(ValueError, match="^gap must be"):
            env.traffic_into(gap=torch.zeros(3, 64))
        with pytest.raises(ValueError, match="^front must be"):
            env.traffic_into(front=torch.zeros(3, 64, device=DEV))
        with pytest.raises(ValueError, match="^ego must be"):
            env.traffic_into(ego=torch.zeros(3, 15, device=DEV))
        with pytest.raises(ValueError, match="unknown traffic outputs"):
            env.traffic_into(headway=t["thw"])
        for name in _abi.TRAFFIC_DEFAULTS:
            with pytest.raises(ValueError, match=f"^{name} must be finite"):
                env.traffic(**{name: 0.0})
    finally:
        env.close()


def test_captured_step_and_traffic_replays_as_the_eager_run():
    from hwy.vec_env import alloc_traffic
    from utils.graphs import capture

    E = 6
    envs = [_vec(E, max_episode_steps=3), _vec(E, max_episode_steps=3)]
    try:
        bufs = []
        for env in envs:
            env.reset()
            b = dict(act=torch.zeros(E, 2, device=DEV), obs=torch.zeros_like(env.obs_buf),
                     rew=torch.zeros(E, device=DEV), term=torch.zeros(E, dtype=torch.uint8, device=DEV),
                     trunc=torch.zeros(E, dtype=torch.uint8, device=DEV), t=alloc_traffic(E, DEV))
            env.traffic_into(**b["t"])       # the reset state (and the code object loads here)
            bufs.append(b)

        def both(env, b):
            env.step_into(b["act"], b["obs"], b["rew"], b["term"], b["trunc"])
            env.traffic_into(restart=(b["term"], b["trunc"]), **b["t"])

        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                both(envs[0], bufs[0])
        torch.cuda.current_stream().wait_stream(s)
        rng = np.random.default_rng(8)
        flushed = 0
        for t in range(3):
            a = torch.as_tensor(policy_actions(rng, E, t), device=DEV)
            for b in bufs:
                b["act"].copy_(a)
            g.replay()
            both(envs[1], bufs[1])
            torch.cuda.synchronize()
            for k in ALL:
                assert torch.equal(bufs[0]["t"][k].view(torch.int32), bufs[1]["t"][k].view(torch.int32)), (t, k)
            assert torch.equal(envs[0].export_state(), envs[1].export_state())
            flushed += int((bufs[0]["t"]["ep_stats"][:, 0] > 0).sum())
        assert flushed >= E, "no episode ended under the capture"
    finally:
        for env in envs:
            env.close()


# ------------------------------------------------------------------- 4. the reduction
@pytest.mark.parametrize("with_cut", [False, True])
def test_running_reduction_is_the_fold_of_the_per_state_outputs(with_cut):
    E = 9
    cfg = make_cfg(E=E, max_episode_steps=7, vehicles_density=2)
    hip = HipEnv(cfg)
    try:
        arena = Arena(E)
        outs = ("front", "ego", "acc", "ep_stats")
        hip.reset()
        got = traffic(hip, outs, arena)
        acc = np.zeros((E, 8), np.float32)
        acc, ep = tm.fold(acc, tm.state_row(got["ego"], got["front"][:, 0] >= 0), np.zeros(E, bool))
        assert np.array_equal(got["acc"].view(np.uint32), acc.view(np.uint32))
        assert not got["ep_stats"].any()
        rng = np.random.default_rng(21)
        flushed, lengths = 0, []
        for t in range(40):
            term, trunc = hip.step(policy_actions(rng, E, t))[2:4]
            masks = [term, trunc]
            if with_cut and t == 17:
                cut = hip.cut_episodes()[3]
                assert cut.any()
                masks.append(cut)
            got = traffic(hip, outs, arena, restart=masks)
            restart = np.logical_or.reduce([m != 0 for m in masks])
            acc, ep = tm.fold(acc, tm.state_row(got["ego"], got["front"][:, 0] >= 0), restart)
            assert np.array_equal(got["acc"].view(np.uint32), acc.view(np.uint32)), f"acc, step {t}"
            assert np.array_equal(got["ep_stats"].view(np.uint32), ep.view(np.uint32)), f"ep, step {t}"
            flushed += int(restart.sum())
            lengths += ep[restart, 0].tolist()
            # (the least gap may be negative: cars overlap before a crash ends the episode)
            assert (ep[restart, 0] >= 1).all() and (ep[restart][:, [1, 2, 4]] >= 0).all()
        assert flushed >= 4 * E and max(lengths) == 7, "no episode of the full 7 states was flushed"
        if with_cut:
            assert any(n < 7 for n in lengths), "the cut flushed no running episode"
    finally:
        hip.close()


# ------------------------------------------------------------------- 5. the Python surface
def test_conveniences_and_the_one_env_facade():
    from hwy.single_env import HighwayEnv

    env = _vec(4)
    try:
        env.reset()
        env.step(torch.full((4, 2), 0.1, device=DEV))
        st = env.export_state().cpu().numpy().view(np.uint32)
        out = env.traffic()
        assert tuple(out) == VEH + ("ego",)
        assert all(out[k].shape == (4, 64) for k in VEH) and out["ego"].shape == (4, 16)
        assert out["front"].dtype == torch.int32 and out["risk"].dtype == torch.float32
        got = {k: v.cpu().numpy() for k, v in out.items()}
        check_against_model(env.hwy_config, st, got, "traffic()")
        th = dict(ttc_thresh=3.0, thw_thresh=2.0, risk_horizon=8.0, near_range=20.0)
        got = {k: v.cpu().numpy() for k, v in env.traffic(**th).items()}
        check_against_model(env.hwy_config, st, got, "traffic(thresholds)", **th)
        frame = env.render(shade=env.traffic(risk_horizon=60.0)["risk"])   # the layout render takes
        assert not torch.equal(frame, env.render())
    finally:
        env.close()
    one = HighwayEnv(HIGHWAY_CONFIG)
    try:
        one.reset(seed=5)
        one.step(np.array([0.1, 0.0], np.float32))
        t = one.traffic()
        assert all(isinstance(v, np.ndarray) for v in t.values())
        assert t["ego"].shape == (16,) and t["front"].shape == (64,) and t["front"].dtype == np.int32
        st = one.vec_env.export_state().cpu().numpy().view(np.uint32)
        check_against_model(one.vec_env.hwy_config, st, {k: v[None] for k, v in t.items()}, "one env")
    finally:
        one.close()
