"""hwy_cut_episodes (include/hwy.h): ending every running episode and starting the schedule's
next one must leave, bit for bit, what an autoreset at a truncation leaves -- checked against
the CPU oracle's reset, with seed groups against solo handles, and captured in a HIP graph."""

import ctypes

import numpy as np
import pytest
import torch

from hwy import _abi
from hwy.native import check, lib, ptr
from oracle.oracle import OracleEnv
from parity_util import diff_state, make_cfg, pe_table_for, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SENTINEL = -777.25


class _Hip:
    """The C ABI driven directly (tests/test_env_parity_gpu.py's HipEnv, plus the cut)."""

    def __init__(self, cfg, table=None):
        self.cfg, self.E = cfg, cfg.num_envs
        self.h = ctypes.c_void_p()
        check(lib().hwy_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "hwy_create")
        if table is not None:
            t = np.ascontiguousarray(table, np.float32)
            check(lib().hwy_set_pe_table(self.h, t.ctypes.data_as(ctypes.c_void_p), t.size),
                  "hwy_set_pe_table")
        E = self.E
        self.obs = torch.zeros(E, cfg.obs_vehicles, cfg.obs_features(), device=DEV)
        self.rew = torch.zeros(E, device=DEV)
        self.term = torch.zeros(E, dtype=torch.uint8, device=DEV)
        self.trunc = torch.zeros(E, dtype=torch.uint8, device=DEV)
        self.er = torch.zeros(E, device=DEV)
        self.el = torch.zeros(E, dtype=torch.int32, device=DEV)
        self.cut = torch.zeros(E, dtype=torch.uint8, device=DEV)

    def reset(self):
        check(lib().hwy_reset(self.h, None, None, ptr(self.obs), None), "hwy_reset")
        torch.cuda.synchronize()
        return self.obs.cpu().numpy()

    def step(self, a):
        at = torch.as_tensor(a, device=DEV).contiguous()
        check(lib().hwy_step(self.h, ptr(at), ptr(self.obs), ptr(self.rew), ptr(self.term),
                             ptr(self.trunc), ptr(self.er), ptr(self.el), None), "hwy_step")
        torch.cuda.synchronize()
        return (self.obs.cpu().numpy(), self.rew.cpu().numpy(), self.term.cpu().numpy().astype(bool),
                self.trunc.cpu().numpy().astype(bool), self.er.cpu().numpy(), self.el.cpu().numpy())

    def cut_episodes(self):
        check(lib().hwy_cut_episodes(self.h, ptr(self.obs), ptr(self.er), ptr(self.el),
                                     ptr(self.cut), None), "hwy_cut_episodes")
        torch.cuda.synchronize()
        return (self.obs.cpu().numpy(), self.er.cpu().numpy(), self.el.cpu().numpy(),
                self.cut.cpu().numpy())

    def state(self):
        out = torch.zeros(_abi.NFIELDS, self.E, 64, dtype=torch.int32, device=DEV)
        check(lib().hwy_export_state(self.h, ptr(out), None), "export")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def set_state(self, st):
        t = torch.as_tensor(np.ascontiguousarray(st).view(np.int32), device=DEV)
        check(lib().hwy_import_state(self.h, ptr(t), None), "import")
        torch.cuda.synchronize()

    def close(self):
        lib().hwy_destroy(self.h)


def _both_step(hip, ora, a, V, what):
    rh, ro = hip.step(a), ora.step(a)
    d = diff_state(hip.state(), ora.state, V)
    assert d is None, f"{what}: {d}"
    for k, name in enumerate(("obs", "reward", "terminated", "truncated", "ep_return", "ep_length")):
        np.testing.assert_array_equal(rh[k], ro[k], err_msg=f"{name} at {what}")
    return ro


@pytest.mark.parametrize("order,pe,d", [("sorted", _abi.PE_NONE, 0),
                                        ("shuffled", _abi.PE_RANK, 4)])
def test_cut_equals_the_oracles_reset_of_the_next_episode(order, pe, d):
    E, skip = 5, (1, 4)  # 5 envs: a full workgroup of 4 and a partial one
    cfg = make_cfg(E=E, order=order, pe=pe, d=d, seed_base=11, max_episode_steps=3)
    table = pe_table_for(pe, d, cfg.obs_vehicles, seed=3)
    hip, ora = _Hip(cfg, table), OracleEnv(cfg, table)
    V = cfg.vehicles_count + 1
    try:
        np.testing.assert_array_equal(hip.reset(), ora.reset())
        rng = np.random.default_rng(7)  # no ego crashes in the first 5 steps: all at step 2
        resets = np.zeros(E, int)
        for t in range(5):
            ro = _both_step(hip, ora, policy_actions(rng, E, t), V, f"step {t}")
            resets += ro[2] | ro[3]
        assert (resets >= 1).all()  # every env went through an autoreset (truncation at 3)
        st = ora.state.copy()
        st[_abi.F_ENV, list(skip), _abi.E_STEP] = 0  # "just reset": the cut must leave them
        ora.state[...] = st
        hip.set_state(st)
        steps = st[_abi.F_ENV, :, _abi.E_STEP].astype(np.int32)
        rets = st[_abi.F_ENV, :, _abi.E_RETURN].copy().view(np.float32)
        k = st[_abi.F_ENV, :, _abi.E_EPISODE].astype(np.int64)
        cutting = np.array([e not in skip for e in range(E)])
        assert (steps[cutting] >= 1).all()

        hip.obs.fill_(SENTINEL)
        obs, er, el, cut = hip.cut_episodes()

        # the oracle's side: reset the cut envs with the schedule's seed of episode k + 1
        seeds = np.array([_abi.schedule_seed(cfg, e, int(k[e]) + 1) for e in range(E)], np.uint64)
        want_obs = ora.reset(seeds=seeds, mask=cutting.astype(np.uint8))
        ora.state[_abi.F_ENV, cutting, _abi.E_EPISODE] = (k[cutting] + 1).astype(np.uint32)
        np.testing.assert_array_equal(cut, cutting.astype(np.uint8))
        np.testing.assert_array_equal(er, np.where(cutting, rets, np.float32(0)))
        np.testing.assert_array_equal(el, np.where(cutting, steps, 0))
        got = hip.state()
        d_ = diff_state(got, ora.state, V)
        assert d_ is None, f"after the cut: {d_}"
        for e in skip:  # untouched: every word as imported, the obs rows still the sentinel
            assert np.array_equal(got[:, e], st[:, e])
            assert (obs[e] == np.float32(SENTINEL)).all()
        np.testing.assert_array_equal(obs[cutting], want_obs[cutting])
        assert (obs[cutting] != np.float32(SENTINEL)).any()

        # the schedule goes on: 4 more steps take the cut envs through an autoreset from
        # episode k + 1 to k + 2 (and the two others from k to k + 1)
        for t in range(4):
            _both_step(hip, ora, policy_actions(rng, E, 5 + t), V, f"step {5 + t} after the cut")
        k2 = hip.state()[_abi.F_ENV, :, _abi.E_EPISODE].astype(np.int64)
        assert (k2 >= np.where(cutting, k + 2, k + 1)).all(), (k, k2)
    finally:
        hip.close()


def _vec(E, table, order="shuffled"):
    import copy

    from config.base_config import HIGHWAY_CONFIG
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["order"] = order
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, pe_kind=_abi.PE_RANK, d_embed=4,
                         pe_table=table)


def _cut_bufs(env):
    E = env.num_envs
    return (torch.full_like(env.obs_buf, SENTINEL), torch.full((E,), SENTINEL, device=DEV),
            torch.full((E,), -5, dtype=torch.int32, device=DEV),
            torch.full((E,), 9, dtype=torch.uint8, device=DEV))


def test_cut_with_seed_groups_equals_solo_handles():
    from config.base_config import HIGHWAY_CONFIG

    G, E, seeds = 2, 3, [5, 900]
    N = HIGHWAY_CONFIG["observation"]["vehicles_count"]
    tables = [pe_table_for(_abi.PE_RANK, 4, N, seed=s) for s in (1, 2)]
    grp = _vec(G * E, tables[0])
    grp.set_seed_groups(seeds, E)
    grp.set_pe_table(np.concatenate([t.reshape(-1) for t in tables]))
    solos = []
    for s, t in zip(seeds, tables):
        solo = _vec(E, t)
        solo.set_seed_schedule(s)
        solos.append(solo)
    gen = torch.Generator(device=DEV).manual_seed(3)
    acts = [torch.rand(G * E, 2, device=DEV, generator=gen) * 2 - 1 for _ in range(3)]
    try:
        for env in [grp] + solos:
            env.reset()
        for a in acts[:2]:
            grp.step(a)
            for g, solo in enumerate(solos):
                solo.step(a[g * E:(g + 1) * E].contiguous())
        gb = _cut_bufs(grp)
        grp.cut_episodes(*gb)
        gstate = grp.export_state()
        gnext = [x.clone() for x in grp.step(acts[2])[:4]]
        torch.cuda.synchronize()
        assert bool((gb[3] == 1).all())
        for g, solo in enumerate(solos):
            sl = slice(g * E, (g + 1) * E)
            sb = _cut_bufs(solo)
            solo.cut_episodes(*sb)
            for k in range(4):
                assert torch.equal(gb[k][sl], sb[k]), (g, k)
            assert torch.equal(gstate[:, sl], solo.export_state()), g
            # ... and the next step of the new episodes
            for x, y in zip(gnext, solo.step(acts[2][sl].contiguous())[:4]):
                assert torch.equal(x[sl], y), g
        # the two groups really differ (their own seeds and rank tables)
        assert not torch.equal(gb[0][:E], gb[0][E:])
    finally:
        for env in [grp] + solos:
            env.close()


def test_cut_captured_in_a_graph_replays_the_eager_result():
    from utils.graphs import capture

    from config.base_config import HIGHWAY_CONFIG

    E = 5
    table = pe_table_for(_abi.PE_RANK, 4, HIGHWAY_CONFIG["observation"]["vehicles_count"], seed=1)
    a, b = _vec(E, table), _vec(E, table)
    gen = torch.Generator(device=DEV).manual_seed(7)
    acts = [torch.rand(E, 2, device=DEV, generator=gen) * 2 - 1 for _ in range(2)]
    try:
        for env in (a, b):
            env.set_seed_schedule(21)
            env.reset()
            for x in acts:
                env.step(x)
        start = b.export_state().clone()
        # env 3 is "just reset" on both sides: the captured launch must skip it as well
        start[_abi.F_ENV, 3, _abi.E_STEP] = 0
        a.import_state(start)
        ab, bb = _cut_bufs(a), _cut_bufs(b)
        a.cut_episodes(*ab)  # eager (also loads the kernel before anything is captured)
        b.import_state(start)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                b.cut_episodes(*bb)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        # capturing ran nothing: the state is still the imported one
        assert torch.equal(b.export_state(), start)
        g.replay()
        torch.cuda.synchronize()
        for k in range(4):
            assert torch.equal(ab[k], bb[k]), k
        assert torch.equal(a.export_state(), b.export_state())
        assert ab[3].tolist() == [1, 1, 1, 0, 1]
        assert bool((bb[0][3] == SENTINEL).all())
    finally:
        a.close()
        b.close()
