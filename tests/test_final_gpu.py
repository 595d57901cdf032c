"""hwy_step_with_final / hwy_step_group_final (include/hwy.h) on the GPU: the final variant of the
step computes the plain step, and where an episode finishes it writes that episode's last
observation -- bit for bit what the CPU oracle observes from the same pre-step state with
autoreset off -- and nothing anywhere else.

Shapes: 6 envs (a full workgroup of 4 and a partial one), 50 vehicles, 15 observed rows,
3-step episodes, 8 steps of hard steering at density 3.  Seed 0 was picked with the oracle on the
CPU: it gives 2 terminated-only and 12 truncated-only rows (the same for every observation
setting, which does not feed back into the dynamics); the tests assert that both kinds occurred."""

import copy
import ctypes
import functools

import numpy as np
import pytest
import torch

from hwy import _abi
from hwy.native import check, lib, ptr
from oracle.oracle import OracleEnv
from parity_util import diff_state, make_cfg, pe_table_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E, STEPS, HORIZON, N = 6, 8, 3, 15
SENTINEL = 0x7FC0DEAD  # a NaN payload no observation produces

CASES = [("sorted", _abi.PE_NONE, 0), ("shuffled", _abi.PE_NONE, 0),
         ("shuffled", _abi.PE_RANK, 4), ("shuffled", _abi.PE_ROPE, 4),
         ("shuffled", _abi.PE_DIST, 4)]
IDS = ["sorted", "shuffled", "shuffled-rankpe4", "shuffled-rope4", "shuffled-distpe4"]


@functools.lru_cache(maxsize=None)
def _actions(n=E):
    """Hard steering (test_step_parity_dense_crashes' actions): crashes within 3 steps."""
    rng = np.random.default_rng(0)
    return [np.tanh(rng.normal(size=(n, 2)) * 2.0).astype(np.float32) for _ in range(STEPS)]


def _cfg(order, pe, d, autoreset=True, n=E):
    return make_cfg(E=n, order=order, pe=pe, d=d, N=N, autoreset=autoreset, seed_base=42,
                    max_episode_steps=HORIZON, vehicles_density=3)


class _Hip:
    """The C ABI driven directly: hwy_step, hwy_step_with_info or hwy_step_with_final."""

    STEP_KEYS = ("obs", "rew", "term", "trunc", "er", "el")
    INFO_KEYS = ("speed", "crashed", "lane", "rewards", "acc", "ep_stats")

    def __init__(self, cfg, table=None):
        self.cfg, self.E = cfg, cfg.num_envs
        self.h = ctypes.c_void_p()
        check(lib().hwy_create(ctypes.byref(cfg), 0, ctypes.byref(self.h)), "hwy_create")
        if table is not None:
            t = np.ascontiguousarray(table, np.float32)
            check(lib().hwy_set_pe_table(self.h, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
                  "hwy_set_pe_table")
        n = self.E
        self.obs = torch.zeros(n, cfg.obs_vehicles, cfg.obs_features(), device=DEV)
        self.final = torch.zeros_like(self.obs)
        self.rew = torch.zeros(n, device=DEV)
        self.term = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.trunc = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.er = torch.zeros(n, device=DEV)
        self.el = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.speed = torch.zeros(n, device=DEV)
        self.crashed = torch.zeros(n, dtype=torch.uint8, device=DEV)
        self.lane = torch.zeros(n, dtype=torch.int32, device=DEV)
        self.rewards = torch.zeros(n, 4, device=DEV)
        self.acc = torch.zeros(n, _abi.HWY_INFO_NACC, device=DEV)
        self.ep_stats = torch.zeros(n, _abi.HWY_INFO_NACC, device=DEV)

    def reset(self, seeds=None, mask=None):
        s = None if seeds is None else torch.as_tensor(np.asarray(seeds, np.int64), device=DEV)
        m = None if mask is None else torch.as_tensor(np.asarray(mask, np.uint8), device=DEV)
        check(lib().hwy_reset(self.h, ptr(s), ptr(m), ptr(self.obs), None), "hwy_reset")
        torch.cuda.synchronize()

    def _out(self, keys):
        torch.cuda.synchronize()
        return {k: getattr(self, k).cpu().numpy() for k in keys}

    def _io(self, a):
        self._a = torch.as_tensor(a, device=DEV).contiguous()
        return (self.h, ptr(self._a), ptr(self.obs), ptr(self.rew), ptr(self.term),
                ptr(self.trunc), ptr(self.er), ptr(self.el))

    def _info(self):
        return _abi.HwyStepInfo(*[ptr(getattr(self, k)) for k in self.INFO_KEYS])

    def step(self, a):
        check(lib().hwy_step(*self._io(a), None), "hwy_step")
        return self._out(self.STEP_KEYS)

    def step_info(self, a):
        info = self._info()
        check(lib().hwy_step_with_info(*self._io(a), ctypes.byref(info), None),
              "hwy_step_with_info")
        return self._out(self.STEP_KEYS + self.INFO_KEYS)

    def step_final(self, a, info=False):
        """The final buffer is filled with the sentinel first; returns it as uint32 words."""
        self.final.view(torch.int32).fill_(SENTINEL)
        si = self._info() if info else None
        check(lib().hwy_step_with_final(*self._io(a), None if si is None else ctypes.byref(si),
                                        ptr(self.final), None), "hwy_step_with_final")
        out = self._out(self.STEP_KEYS + (self.INFO_KEYS if info else ()))
        out["final"] = self.final.cpu().numpy().view(np.uint32)
        return out

    def state(self):
        out = torch.zeros(_abi.NFIELDS, self.E, 64, dtype=torch.int32, device=DEV)
        check(lib().hwy_export_state(self.h, ptr(out), None), "export")
        torch.cuda.synchronize()
        return out.cpu().numpy().view(np.uint32)

    def close(self):
        lib().hwy_destroy(self.h)


def _check_final_rows(out, want_obs, done, what):
    """final rows of done envs = want_obs' rows bit for bit; the others keep the sentinel."""
    fin = out["final"]
    want = np.ascontiguousarray(want_obs, np.float32).view(np.uint32)
    for e in range(fin.shape[0]):
        if done[e]:
            np.testing.assert_array_equal(fin[e], want[e], err_msg=f"{what}: final row of env {e}")
        else:
            assert (fin[e] == SENTINEL).all(), f"{what}: env {e} is not done but was written"


@pytest.mark.parametrize("order,pe,d", CASES, ids=IDS)
def test_final_step_is_the_step_and_final_obs_is_the_oracles(order, pe, d):
    table = pe_table_for(pe, d, N)
    cfg = _cfg(order, pe, d)
    fin, twin, inf = _Hip(cfg, table), _Hip(cfg, table), _Hip(cfg, table)
    ora = OracleEnv(_cfg(order, pe, d, autoreset=False), table)
    V = cfg.vehicles_count + 1
    term_only = trunc_only = 0
    try:
        for h in (fin, twin, inf):
            h.reset()
        for t, a in enumerate(_actions()):
            before = fin.state()
            assert diff_state(before, twin.state(), V) is None
            ora.state[...] = before  # the oracle, autoreset off, takes the same step
            o_obs, o_rew, o_term, o_trunc, _, _ = ora.step(a)
            f, p, i = fin.step_final(a, info=True), twin.step(a), inf.step_info(a)
            for k in _Hip.STEP_KEYS:
                np.testing.assert_array_equal(
                    f[k].view(np.uint32) if f[k].dtype == np.float32 else f[k],
                    p[k].view(np.uint32) if p[k].dtype == np.float32 else p[k],
                    err_msg=f"{k} at step {t}")
            for k in _Hip.INFO_KEYS:  # with info pointers: hwy_step_with_info's outputs
                np.testing.assert_array_equal(f[k], i[k], err_msg=f"info {k} at step {t}")
            d_ = diff_state(fin.state(), twin.state(), V)
            assert d_ is None, f"step {t}: {d_}"
            np.testing.assert_array_equal(f["term"].astype(bool), o_term)
            np.testing.assert_array_equal(f["trunc"].astype(bool), o_trunc)
            np.testing.assert_array_equal(f["rew"], o_rew)
            done = (f["term"] | f["trunc"]).astype(bool)
            _check_final_rows(f, o_obs, done, f"step {t}")
            # where the env goes on, the oracle's obs is the step's obs too
            np.testing.assert_array_equal(f["obs"][~done].view(np.uint32),
                                          o_obs[~done].view(np.uint32))
            term_only += int((f["term"] & ~f["trunc"] & 1).sum())
            trunc_only += int((f["trunc"] & ~f["term"] & 1).sum())
        print(f"terminated-only {term_only} truncated-only {trunc_only}")
        assert term_only >= 1 and trunc_only >= 1
    finally:
        for h in (fin, twin, inf):
            h.close()


def test_final_without_info_pointers_and_episode_stats_only():
    """info NULL, and info with only acc / ep_stats (what the rollout passes): the same step."""
    cfg = _cfg("shuffled", _abi.PE_NONE, 0)
    a_, b_, ref = _Hip(cfg), _Hip(cfg), _Hip(cfg)
    dones = 0
    try:
        for h in (a_, b_, ref):
            h.reset()
        for t, a in enumerate(_actions()):
            fa = a_.step_final(a, info=False)
            b_.final.view(torch.int32).fill_(SENTINEL)
            si = _abi.HwyStepInfo(acc=ptr(b_.acc), ep_stats=ptr(b_.ep_stats))
            check(lib().hwy_step_with_final(*b_._io(a), ctypes.byref(si), ptr(b_.final), None),
                  "hwy_step_with_final")
            fb = b_._out(_Hip.STEP_KEYS + ("acc", "ep_stats"))
            fb["final"] = b_.final.cpu().numpy().view(np.uint32)
            r = ref.step_info(a)
            for k in _Hip.STEP_KEYS:
                np.testing.assert_array_equal(fa[k], r[k], err_msg=f"{k} at step {t}")
                np.testing.assert_array_equal(fb[k], r[k], err_msg=f"{k} at step {t}")
            np.testing.assert_array_equal(fa["final"], fb["final"])
            np.testing.assert_array_equal(fb["acc"], r["acc"])
            np.testing.assert_array_equal(fb["ep_stats"], r["ep_stats"])
            dones += int((r["term"] | r["trunc"]).sum())
        assert dones >= 5
    finally:
        for h in (a_, b_, ref):
            h.close()


def test_autoreset_off_final_rows_equal_the_obs_rows():
    cfg = _cfg("shuffled", _abi.PE_ROPE, 4, autoreset=False)
    hip = _Hip(cfg, pe_table_for(_abi.PE_ROPE, 4, N))
    dones = 0
    try:
        hip.reset()
        for t, a in enumerate(_actions()):
            f = hip.step_final(a)
            done = (f["term"] | f["trunc"]).astype(bool)
            _check_final_rows(f, f["obs"], done, f"step {t}")
            dones += int(done.sum())
            if done.any():  # masked re-reset with explicit seeds
                hip.reset(seeds=(7000 + 100 * t + np.arange(E)).astype(np.uint64), mask=done)
        assert dones >= 5
    finally:
        hip.close()


def _vec_env(n, pe, d, seed, **kw):
    from config.base_config import HIGHWAY_CONFIG
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["order"] = "shuffled"
    cfg.update(max_episode_steps=HORIZON, vehicles_density=3)
    return HighwayVecEnv(cfg, num_envs=n, device=DEV, seed_base=seed, pe_kind=pe, d_embed=d,
                         pe_table=pe_table_for(pe, d, N), **kw)


def test_grouped_final_step_equals_each_handles_own_and_replays_from_a_graph():
    """Two handles (6 envs, F_out 4; 5 envs RankPE d 4, F_out 8) through one GroupEnvStep final
    launch against each handle's own hwy_step_with_final; then the launch captured in a (linear)
    graph and replayed 3 times against the eager solo calls."""
    from hwy.vec_env import GroupEnvStep, alloc_step_info
    from utils.graphs import capture

    specs = [(6, _abi.PE_NONE, 0, 42), (5, _abi.PE_RANK, 4, 77)]

    def make_set():
        envs = [_vec_env(*s) for s in specs]
        for e in envs:
            e.reset()
        return envs

    def bufs(env):
        n = env.num_envs
        io = (torch.zeros(n, 2, device=DEV), torch.zeros_like(env.obs_buf),
              torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.uint8, device=DEV),
              torch.zeros(n, dtype=torch.uint8, device=DEV), torch.zeros(n, device=DEV),
              torch.zeros(n, dtype=torch.int32, device=DEV))
        info = alloc_step_info(n, DEV)
        return io, {"acc": info["acc"], "ep_stats": info["ep_stats"]}, torch.zeros_like(env.obs_buf)

    solo, grouped = make_set(), make_set()
    assert [e.obs_features for e in solo] == [4, 8]
    try:
        gstep = GroupEnvStep(grouped)
        bs, bg = [bufs(e) for e in solo], [bufs(e) for e in grouped]
        rng = np.random.default_rng(0)
        dones = 0

        def set_actions():
            for (a, _, fa), (b, _, fb) in zip(bs, bg):
                x = torch.as_tensor(np.tanh(rng.normal(size=(a[0].shape[0], 2)) * 2.0)
                                    .astype(np.float32), device=DEV)
                a[0].copy_(x)
                b[0].copy_(x)
                fa.view(torch.int32).fill_(SENTINEL)
                fb.view(torch.int32).fill_(SENTINEL)

        def solo_step():
            for env, (a, ai, fa) in zip(solo, bs):
                env.step_into(*a, info=ai, final_obs=fa)

        def launch():
            gstep.launch([b for b, _, _ in bg], infos=[bi for _, bi, _ in bg],
                         final_obs=[fb for _, _, fb in bg])

        def compare(what):
            n = 0
            torch.cuda.synchronize()
            for i, ((a, ai, fa), (b, bi, fb)) in enumerate(zip(bs, bg)):
                for k in range(1, 7):
                    assert torch.equal(a[k], b[k]), (what, i, k)
                for k in ai:
                    assert torch.equal(ai[k], bi[k]), (what, i, k)
                assert torch.equal(fa.view(torch.int32), fb.view(torch.int32)), (what, i, "final")
                done = (a[3] | a[4]).bool()
                sent = (fa.view(torch.int32) == SENTINEL).flatten(1).all(1)
                assert torch.equal(sent, ~done), (what, i, "sentinel rows")
                n += int(done.sum())
            return n

        for t in range(STEPS):
            set_actions()
            solo_step()
            launch()
            dones += compare(f"step {t}")
        assert dones >= 5
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                launch()
        torch.cuda.current_stream().wait_stream(s)
        # the capture ran nothing: both sides are still in step
        replay_dones = 0
        for t in range(3):
            set_actions()
            solo_step()
            g.replay()
            replay_dones += compare(f"replay {t}")
        assert replay_dones >= 1
        for x, y in zip(solo, grouped):
            assert torch.equal(x.export_state(), y.export_state())
        # without info dicts the launch is the same step
        set_actions()
        for env, (a, _, fa) in zip(solo, bs):
            env.step_into(*a, final_obs=fa)
        gstep.launch([b for b, _, _ in bg], final_obs=[fb for _, _, fb in bg])
        torch.cuda.synchronize()
        for (a, _, fa), (b, _, fb) in zip(bs, bg):
            assert torch.equal(a[1], b[1])
            assert torch.equal(fa.view(torch.int32), fb.view(torch.int32))
    finally:
        for env in solo + grouped:
            env.close()


def test_python_env_reports_final_observation():
    on = _vec_env(E, _abi.PE_NONE, 0, 42, final_obs=True)
    both = _vec_env(E, _abi.PE_NONE, 0, 42, final_obs=True, info=True)
    off = _vec_env(E, _abi.PE_NONE, 0, 42)
    dones = 0
    try:
        assert off.final_obs_buf is None
        assert on.final_obs_buf.shape == on.obs_buf.shape == (E, N, 4)
        for env in (on, both, off):
            env.reset()
        for t, a in enumerate(_actions()):
            at = torch.as_tensor(a, device=DEV)
            prev = on.final_obs_buf.clone()
            o1, r1, te1, tr1, i1 = on.step(at)
            o2, r2, te2, tr2, i2 = both.step(at)
            o0, r0, te0, tr0, i0 = off.step(at)
            assert sorted(i0) == ["episode_length", "episode_return"]
            assert sorted(i1) == ["_final_observation", "episode_length", "episode_return",
                                  "final_observation"]
            assert sorted(i2) == sorted(list(i1) + ["crashed", "episode_stats", "lane", "rewards",
                                                    "speed"])
            for x, y, z in ((o1, o2, o0), (r1, r2, r0), (te1, te2, te0), (tr1, tr2, tr0)):
                assert torch.equal(x, z) and torch.equal(y, z)
            mask = i1["_final_observation"]
            assert mask.dtype == torch.bool and torch.equal(mask, (te0 | tr0).bool())
            assert i1["final_observation"] is on.final_obs_buf
            assert torch.equal(i1["final_observation"], i2["final_observation"])
            # rows of envs that go on keep what they held
            assert torch.equal(on.final_obs_buf[~mask], prev[~mask])
            # a finished env's obs row is the next episode's first observation, not the final one
            if bool(mask.any()):
                assert not torch.equal(on.final_obs_buf[mask], o1[mask])
            dones += int(mask.sum())
        assert dones >= 5
        with pytest.raises(ValueError, match="final_obs"):
            on.step_into(at, on.obs_buf, on.reward_buf, on.term_buf, on.trunc_buf,
                         final_obs=torch.zeros(3, device=DEV))
        with pytest.raises(ValueError, match="obs buffer"):
            on.step_into(at, on.obs_buf, on.reward_buf, on.term_buf, on.trunc_buf,
                         final_obs=on.obs_buf)
    finally:
        for env in (on, both, off):
            env.close()
