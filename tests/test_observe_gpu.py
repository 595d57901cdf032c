"""hwy_observe on the device: the handle's own order against the step's bits, the other order
against the oracle's, the row -> vehicle map against tests/observe_model.py and by identification,
the scatter, bounds, graph capture, the Python surface, and what training/routine.py and
experiments/runner.py build on it (evaluate(order=...), the attribution overlay, eval_orders).

Every observe call of the kernel-level tests runs between guard words: each output (and the
row_values input) sits inside a larger buffer whose other words must come back untouched."""

from __future__ import annotations

import copy
import ctypes
import os

import numpy as np
import pytest
import torch

import env_model as em
import observe_model as om
import observe_util as ou
from config.base_config import HIGHWAY_CONFIG
from env_util import HipEnv
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import dist_freqs, make_cfg, pe_table_for, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 64            # words on either side of every buffer
CANARY = 0x5A5AA5A5

PE = {"none": (_abi.PE_NONE, 0), "rank": (_abi.PE_RANK, 8), "dist": (_abi.PE_DIST, 8),
      "dist1": (_abi.PE_DIST1, 8), "rope": (_abi.PE_ROPE, 4)}
ALL_FEATURES = ["presence", "x", "y", "vx", "vy", "cos_h", "sin_h", "heading"]


def table_for(kind, d, N, seed=0):
    return dist_freqs(d) if kind == _abi.PE_DIST1 else pe_table_for(kind, d, N, seed)


class Guarded:
    """n 32-bit words between two runs of canaries"""

    def __init__(self, n, dtype, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.mid = self.buf[GUARD:GUARD + n]
        self.mid.fill_(0x7FC12345 if fill is None else fill)   # a NaN pattern no output holds
        self.view = self.mid.view(dtype)

    def ptr(self):
        return self.mid.data_ptr()

    def check(self, name):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == CANARY).all() and (b[GUARD + self.n:] == CANARY).all(), \
            f"{name}: a word outside the output was written"


def observe(hip, order=-1, obs=True, rv=True, row_values=None):
    """one hwy_observe launch on a HipEnv's handle; numpy results by name"""
    from hwy.native import check, lib

    E, N, Fo = hip.E, hip.N, hip.Fo
    bufs = {}
    if obs:
        bufs["obs"] = Guarded(E * N * Fo, torch.float32)
    if rv:
        bufs["row_vehicle"] = Guarded(E * N, torch.int32)
    if row_values is not None:
        bufs["row_values"] = Guarded(E * N, torch.float32)
        bufs["row_values"].view.copy_(torch.as_tensor(np.ascontiguousarray(row_values, np.float32)
                                                      .reshape(-1), device=DEV))
        bufs["veh_values"] = Guarded(E * 64, torch.float32)
    a = _abi.ObserveArgs(int(order), *[bufs[k].ptr() if k in bufs else None
                                       for k in ("obs", "row_vehicle", "row_values", "veh_values")])
    check(lib().hwy_observe(hip.h, ctypes.byref(a), None), "hwy_observe")
    torch.cuda.synchronize()
    for k, b in bufs.items():
        b.check(k)
    out = {}
    if obs:
        out["obs"] = bufs["obs"].view.cpu().numpy().reshape(E, N, Fo)
    if rv:
        out["row_vehicle"] = bufs["row_vehicle"].view.cpu().numpy().reshape(E, N)
    if row_values is not None:
        out["veh_bits"] = bufs["veh_values"].mid.cpu().numpy().view(np.uint32).reshape(E, 64)
        given = np.ascontiguousarray(row_values, np.float32).reshape(-1).view(np.uint32)
        assert (bufs["row_values"].mid.cpu().numpy().view(np.uint32) == given).all(), \
            "row_values was written"
    return out


def same_bits(a, b, msg):
    a, b = (np.ascontiguousarray(x, np.float32).view(np.uint32) for x in (a, b))
    assert a.shape == b.shape, msg
    bad = np.argwhere(a != b)
    assert not len(bad), f"{msg}: {len(bad)} words differ, first at {bad[0].tolist()}"


# ------------------------------------------------------------------- 1. the handle's own order
def drive_and_compare(cfg, table, steps=16, groups=None, group_tables=None):
    """reset, `steps` steps, a masked seeded reset and a cut on a handle that observes after
    each, against the buffer the call wrote and against a twin handle that never observes"""
    from hwy.native import check, lib

    hips = [HipEnv(cfg, table), HipEnv(cfg, table)]
    try:
        for h in hips:
            if groups is not None:
                h.set_seed_groups(*groups)
                t = np.ascontiguousarray(group_tables, np.float32)
                check(lib().hwy_set_pe_table(h.h, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
                      "hwy_set_pe_table")
        hip, twin = hips
        E = cfg.num_envs

        def agree(what):
            before = hip.state()
            for order in (-1, int(cfg.order)):
                same_bits(observe(hip, order)["obs"], hip.obs.cpu().numpy(), f"{what}, order {order}")
            assert np.array_equal(before, hip.state()), f"{what}: the observe changed the state"

        hip.reset()
        twin.reset()
        agree("after reset")
        rng = np.random.default_rng(5)
        resets = 0
        for t in range(steps):
            a = policy_actions(rng, E, t)
            out = hip.step(a)
            twin.step(a)
            resets += int((out[2] | out[3]).sum())
            agree(f"after step {t}")
        assert resets > 0, "no autoreset happened"
        mask = (np.arange(E) % 3 == 1).astype(np.uint8)
        seeds = 9000 + 7 * np.arange(E)
        hip.reset(seeds, mask)
        twin.reset(seeds, mask)
        agree("after a masked seeded reset")
        a = policy_actions(rng, E, steps)
        out = hip.step(a)
        twin.step(a)
        cut = hip.cut_episodes()[3]
        twin.cut_episodes()
        # every env that did not just finish (and restart at step 0) is cut
        assert np.array_equal(cut != 0, (out[2] | out[3]) == 0)
        agree("after cut_episodes")
        a = policy_actions(rng, E, steps + 1)
        hip.step(a)
        twin.step(a)
        assert np.array_equal(hip.state(), twin.state()), "step-observe-step is not step-step"
        same_bits(hip.obs.cpu().numpy(), twin.obs.cpu().numpy(), "obs of step-observe-step")
    finally:
        for h in hips:
            h.close()


@pytest.mark.parametrize("stored", ou.VIEWS)
@pytest.mark.parametrize("pe", list(PE))
def test_own_order_gives_the_steps_bits(pe, stored):
    kind, d = PE[pe]
    cfg = make_cfg(E=18, order=stored, pe=kind, d=d, max_episode_steps=5)
    drive_and_compare(cfg, table_for(kind, d, cfg.obs_vehicles))


def test_own_order_one_env():
    kind, d = PE["rope"]
    cfg = make_cfg(E=1, order="shuffled", pe=kind, d=d, max_episode_steps=3)
    drive_and_compare(cfg, table_for(kind, d, cfg.obs_vehicles))


@pytest.mark.parametrize("stored", ou.VIEWS)
def test_own_order_seed_groups_with_their_own_rank_tables(stored):
    kind, d = PE["rank"]
    cfg = make_cfg(E=18, order=stored, pe=kind, d=d, max_episode_steps=5)
    cfg.seed_stride = 6
    tables = np.stack([table_for(kind, d, cfg.obs_vehicles, seed=s) for s in (1, 2, 3)])
    assert not np.array_equal(tables[0], tables[1])
    drive_and_compare(cfg, tables[0], groups=([100, 2000, 30000], 6), group_tables=tables)


def test_own_order_widest_row():
    cfg = make_cfg(E=6, order="shuffled", pe=_abi.PE_RANK, d=56, max_episode_steps=4,
                   observation={"features": ALL_FEATURES})
    assert cfg.obs_features() == _abi.HWY_MAX_FOUT
    drive_and_compare(cfg, table_for(_abi.PE_RANK, 56, cfg.obs_vehicles), steps=8)


# ------------------------------------------------------------------- 2. the other order
SUBSET = {
    "default": {},
    "N1": dict(N=1), "N2": dict(N=2), "N3": dict(N=3), "N64": dict(N=64),
    "1car": dict(vehicles_count=1), "63cars": dict(vehicles_count=63),
    "see_behind": dict(observation={"see_behind": True}),
    "absolute": dict(observation={"absolute": True}),
    "raw": dict(observation={"normalize": False}),
    "ego_idx2": dict(ego_idx=2),
}


@pytest.mark.parametrize("pe", list(PE))
@pytest.mark.parametrize("name", list(SUBSET))
def test_either_order_gives_the_oracles_bits(name, pe):
    kind, d = PE[pe]
    stored = ou.VIEWS[(list(SUBSET).index(name) + list(PE).index(pe)) % 2]
    cfg = make_cfg(E=6, order=stored, pe=kind, d=d, max_episode_steps=4, **SUBSET[name])
    table = table_for(kind, d, cfg.obs_vehicles)
    hip = HipEnv(cfg, table)
    try:
        hip.reset()
        rng = np.random.default_rng(11)
        for t in range(6):
            if t:
                hip.step(policy_actions(rng, cfg.num_envs, t))
            st = hip.state()
            for view in ou.VIEWS:
                got = observe(hip, om.ORDERS[view], rv=False)["obs"]
                want = ou.oracle_observe(om.with_order(cfg, view), st, table)
                same_bits(got, want, f"{name}/{pe} stored {stored} viewed {view} at step {t}")
            if name == "default" and t == 5:   # the two views are two observations
                assert not np.array_equal(got, observe(hip, om.ORDERS["sorted"], rv=False)["obs"])
    finally:
        hip.close()


# ------------------------------------------------------------------- 3. the map, 4. the scatter
def identity_obs(cfg, state, view):
    """the kernel's observation of `state` under the identity config (a handle of its own)"""
    ic = om.identity_cfg(cfg, view)
    h = HipEnv(ic)
    try:
        h.set_state(state)
        return ic, observe(h, rv=False)["obs"]
    finally:
        h.close()


def check_map_and_scatter(cfg, hip, state, rng, tally):
    keep = ~em.uncertain(cfg, state)
    tally["cases"] += 2 * len(keep)
    tally["left_out"] += 2 * int((~keep).sum())
    E, N = cfg.num_envs, cfg.obs_vehicles
    for view in ou.VIEWS:
        vals = rng.normal(size=(E, N)).astype(np.float32)
        vals[:, ::4] = -0.0
        vals[0, 0] = np.float32(-1.5)
        out = observe(hip, om.ORDERS[view], row_values=vals)
        rv = out["row_vehicle"]
        want = om.row_vehicles(cfg, state, view)
        assert np.array_equal(rv[keep], want[keep]), f"row_vehicle, view {view}"
        assert (rv[:, 0] == 0).all(), "row 0 is the ego"
        assert ((rv >= -1) & (rv < 64)).all()
        for e in range(E):
            full = rv[e][rv[e] >= 0]
            assert len(set(full.tolist())) == len(full), f"env {e}: a vehicle in two rows"
        ic, obs_abs = identity_obs(cfg, state, view)
        seen, empty, bad = om.identify(ic, state, rv, obs_abs)
        assert not bad, bad[:5]
        zero_row = ~obs_abs.view(np.uint32).any(axis=2)
        assert np.array_equal(zero_row, rv < 0), "-1 exactly where the row is all zero"
        tally["rows"] += seen
        tally["empty"] += empty
        assert np.array_equal(out["veh_bits"][keep], om.scatter(want, vals)[keep]), "veh_values"
        assert np.array_equal(out["veh_bits"], om.scatter(rv, vals)), \
            "veh_values against the kernel's own map: an entry no row shows must be +0.0"


@pytest.mark.parametrize("stored", ou.VIEWS)
@pytest.mark.parametrize("name", list(ou.CONFIGS))
def test_map_and_scatter_on_natural_states(name, stored):
    cfg = make_cfg(E=16, order=stored, max_episode_steps=6, **ou.CONFIGS[name])
    hip = HipEnv(cfg)
    tally = dict(cases=0, left_out=0, rows=0, empty=0)
    try:
        hip.reset()
        rng = np.random.default_rng(3)
        for t in range(8):
            hip.step(policy_actions(rng, cfg.num_envs, t))
            if t % 2:
                check_map_and_scatter(cfg, hip, hip.state(), rng, tally)
        print(f"{name}/{stored}: {tally}")
        assert tally["left_out"] <= 0.01 * tally["cases"]
        assert 0 < tally["empty"] < tally["rows"]
    finally:
        hip.close()


@pytest.mark.parametrize("behind", [False, True])
@pytest.mark.parametrize("stored", ou.VIEWS)
def test_map_and_scatter_on_crafted_states(stored, behind):
    cfg = ou.craft_cfg(stored, **(dict(observation={"see_behind": True}) if behind else {}))
    st = ou.craft(cfg)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(st)
        tally = dict(cases=0, left_out=0, rows=0, empty=0)
        check_map_and_scatter(cfg, hip, st, np.random.default_rng(1), tally)
        assert tally["left_out"] == 0
        rows = observe(hip, om.ORDERS["sorted"], obs=False)["row_vehicle"]
        if not behind:
            ou.check_crafted_map(rows)   # the tie to the lower index, the NaN, the absent slots
            assert list(rows[4]) == [0, 8, 5, 2, 10]
        else:
            assert list(rows[3]) == [0, 9, 2, 1, -1]
        sh = observe(hip, om.ORDERS["shuffled"], obs=False)["row_vehicle"]
        assert len({tuple(sh[e]) for e in (4, 5, 6, 7)}) > 1, "the shuffle ignores the step word"
        for e in (4, 5, 6, 7):
            assert sorted(sh[e, 1:]) == [1, 2, 3, 4]
    finally:
        hip.close()


# ------------------------------------------------------------------- 5. NULL outputs
def test_every_combination_of_outputs():
    kind, d = PE["dist"]
    cfg = make_cfg(E=7, order="shuffled", pe=kind, d=d)
    hip = HipEnv(cfg, table_for(kind, d, cfg.obs_vehicles))
    try:
        hip.reset()
        hip.step(policy_actions(np.random.default_rng(2), 7, 0))
        vals = np.random.default_rng(4).normal(size=(7, cfg.obs_vehicles)).astype(np.float32)
        for order in (-1, 0, 1):
            full = observe(hip, order, row_values=vals)
            n = 0
            for o in (False, True):
                for r in (False, True):
                    for v in (None, vals):
                        if not (o or r or v is not None):
                            continue
                        part = observe(hip, order, obs=o, rv=r, row_values=v)
                        n += 1
                        assert part and all(np.array_equal(part[k].view(np.uint32),
                                                           full[k].view(np.uint32)) for k in part)
            assert n == 7
    finally:
        hip.close()


# ------------------------------------------------------------------- 6. capture
def _vec(E, order="sorted", autoreset=False, **kw):
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["order"] = order
    cfg.update(kw)
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=autoreset)


def test_captured_observe_replays_on_the_later_state():
    from utils.graphs import capture

    env = _vec(5)
    try:
        env.reset(seed=3)
        E, N, Fo = 5, env.obs_rows, env.obs_features
        obs = torch.zeros(E, N, Fo, device=DEV)
        rv = torch.zeros(E, N, dtype=torch.int32, device=DEV)
        vals = torch.rand(E, N, device=DEV)
        veh = torch.zeros(E, 64, device=DEV)
        kw = dict(obs=obs, row_vehicle=rv, row_values=vals, veh_values=veh)
        env.observe_into("shuffled", **kw)  # eager first: the code object loads outside the capture
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                env.observe_into("shuffled", **kw)
        torch.cuda.current_stream().wait_stream(s)
        first = [t.clone() for t in (obs, rv, veh)]
        for _ in range(3):
            env.step(torch.full((E, 2), 0.3, device=DEV))
        for t in (obs, rv, veh):
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(obs, env.observe("shuffled"))
        assert torch.equal(rv, env.row_vehicles("shuffled"))
        assert torch.equal(veh, env.rows_to_vehicles(vals, "shuffled"))
        assert not torch.equal(obs, first[0]) and not torch.equal(veh, first[2])
    finally:
        env.close()


# ------------------------------------------------------------------- 7. the Python surface
def test_conveniences_and_the_one_env_facade():
    from hwy.single_env import HighwayEnv

    env = _vec(4, order="shuffled", autoreset=True)
    try:
        step_obs, _ = env.reset(seed=11)
        env.step(torch.full((4, 2), 0.1, device=DEV))
        E, N, Fo = 4, env.obs_rows, env.obs_features
        o = env.observe()
        assert o.shape == (E, N, Fo) and o.dtype == torch.float32 and torch.equal(o, step_obs)
        assert o.data_ptr() != env.obs_buf.data_ptr()
        buf = torch.empty(E * N * Fo, device=DEV)
        assert env.observe("sorted", out=buf).data_ptr() == buf.data_ptr()
        assert not torch.equal(buf.view(E, N, Fo), o)
        rv = env.row_vehicles()
        assert rv.shape == (E, N) and rv.dtype == torch.int32 and (rv[:, 0] == 0).all()
        want = om.row_vehicles(env.hwy_config, env.export_state().cpu().numpy().view(np.uint32))
        assert np.array_equal(rv.cpu().numpy(), want)
        rbuf = torch.empty(E, N, dtype=torch.int32, device=DEV)
        assert env.row_vehicles("sorted", out=rbuf).data_ptr() == rbuf.data_ptr()
        vals = torch.rand(E, N, device=DEV) + 0.5
        veh = env.rows_to_vehicles(vals)
        assert veh.shape == (E, 64) and veh.dtype == torch.float32
        assert np.array_equal(veh.cpu().numpy().view(np.uint32), om.scatter(want, vals.cpu().numpy()))
        vbuf = torch.empty(E, 64, device=DEV)
        assert env.rows_to_vehicles(vals, out=vbuf).data_ptr() == vbuf.data_ptr()
        assert torch.equal(vbuf, veh)
        frame = env.render(shade=veh)   # the layout render takes
        assert not torch.equal(frame, env.render())
    finally:
        env.close()
    one = HighwayEnv(HIGHWAY_CONFIG)
    try:
        one.reset(seed=5)
        one.step(np.array([0.1, 0.0], np.float32))
        rows = one.row_vehicles()
        assert isinstance(rows, np.ndarray) and rows.shape == (15,) and rows.dtype == np.int32
        st = one.vec_env.export_state().cpu().numpy().view(np.uint32)
        assert np.array_equal(rows, om.row_vehicles(one.vec_env.hwy_config, st)[0])
    finally:
        one.close()


def test_bad_observe_arguments_raise_value_error():
    env = _vec(3)
    try:
        env.reset(seed=1)
        E, N, Fo = 3, env.obs_rows, env.obs_features
        ok = dict(obs=torch.zeros(E, N, Fo, device=DEV),
                  row_vehicle=torch.zeros(E, N, dtype=torch.int32, device=DEV),
                  row_values=torch.zeros(E, N, device=DEV), veh_values=torch.zeros(E, 64, device=DEV))
        env.observe_into(**ok)
        bad = dict(obs=[torch.zeros(E, N, Fo), torch.zeros(E, N, Fo + 1, device=DEV),
                        torch.zeros(E, N, Fo, dtype=torch.float64, device=DEV),
                        torch.zeros(E, Fo, N, device=DEV).transpose(1, 2)],
                   row_vehicle=[torch.zeros(E, N, dtype=torch.int64, device=DEV),
                                torch.zeros(E, N, dtype=torch.int32)],
                   row_values=[torch.zeros(E, N + 1, device=DEV), torch.zeros(E, N)],
                   veh_values=[torch.zeros(E, 63, device=DEV),
                               torch.zeros(E, 64, dtype=torch.float16, device=DEV)])
        for name, tensors in bad.items():
            for t in tensors:
                with pytest.raises(ValueError, match=f"^{name} must be"):
                    env.observe_into(**{**ok, name: t})
        with pytest.raises(ValueError, match="at least one"):
            env.observe_into()
        with pytest.raises(ValueError, match="go together"):
            env.observe_into(obs=ok["obs"], veh_values=ok["veh_values"])
        with pytest.raises(ValueError, match="go together"):
            env.observe_into(row_vehicle=ok["row_vehicle"], row_values=ok["row_values"])
        for call in (env.observe, env.row_vehicles, lambda o: env.rows_to_vehicles(ok["row_values"], o)):
            with pytest.raises(ValueError, match="order must be"):
                call("reversed")
        with pytest.raises(ValueError):
            env.observe(out=torch.zeros(5, device=DEV))
        with pytest.raises(ValueError):
            env.rows_to_vehicles(torch.zeros(E, N + 2, device=DEV))
    finally:
        env.close()


def test_tables_without_meaning_are_refused():
    from hwy.vec_env import HighwayVecEnv

    kind, d = PE["rank"]
    N = HIGHWAY_CONFIG["observation"]["vehicles_count"]
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=4, device=DEV, pe_kind=kind, d_embed=d,
                        pe_table=table_for(kind, d, N))
    try:
        env.set_seed_groups([10, 20], 2)
        env.set_pe_table(np.stack([table_for(kind, d, N, s) for s in (1, 2)]))
        env.reset()
        assert torch.equal(env.observe(), env.obs_buf)
        env.set_seed_groups(None)
        with pytest.raises(ValueError, match="hwy_observe"):
            env.observe()
        env.set_pe_table(table_for(kind, d, N))
        env.observe()
    finally:
        env.close()


# ------------------------------------------------------------------- 8. evaluation
def test_evaluate_in_either_order(monkeypatch):
    from test_eval_gpu import HORIZON, REL, _agent, _config, tape_select_action
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    n, seed = 5, 7
    env = HighwayVecEnv(_config(), num_envs=4, device=DEV, autoreset=True)   # stored `sorted`
    agent = _agent(64, seed=64)
    try:
        base = routine.evaluate(env, agent, n, exp_seed=seed)
        # once more: the first fused acting moved the weights into their flat buffer, which is
        # part of the memo's key; from here on the key is stable
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base
        memo = env._eval_memo
        assert routine.evaluate(env, agent, n, exp_seed=seed, order="sorted") == base
        tape = tape_select_action(agent, monkeypatch)
        value = routine.evaluate(env, agent, n, exp_seed=seed, order="shuffled")
        assert env._eval_memo is memo, "the order=None memo was touched"
        assert len(tape) in (8, HORIZON + 1)   # the host's "all done" check at k = 7, or the end

        ev = env._eval_envs[n]
        c = _abi.HwyConfig.from_buffer_copy(ev.hwy_config)
        c.num_envs, c.autoreset = n, 0
        flipped = om.with_order(c, "shuffled")
        ora = OracleEnv(c)
        ora.reset(seeds=(seed + 1000 + np.arange(n)).astype(np.uint64))
        total, alive, differs = np.zeros(n), np.ones(n, bool), False
        for k, (o, a) in enumerate(tape[:HORIZON]):
            want = ou.oracle_observe(flipped, ora.state).reshape(n, -1)
            same_bits(np.asarray(o).reshape(n, -1)[alive], want[alive], f"fed observation {k}")
            differs |= not np.array_equal(want[alive], ora.observe().reshape(n, -1)[alive])
            _, r, te, tr, _, _ = ora.step(np.asarray(a, np.float32).reshape(n, 2))
            total += np.where(alive, r.astype(np.float64), 0.0)
            alive &= ~(te | tr)
        assert not alive.any() and differs
        want = float(np.mean(total))
        print(f"shuffled view: {value!r}, replay {want!r}; own order {base!r}")
        assert abs(value - want) <= REL * abs(want)

        # a memo hit runs nothing and returns the same value; the order=None memo stays
        monkeypatch.setattr(routine, "_run_eval_vector",
                            lambda *a, **k: pytest.fail("the memo missed"))
        assert routine.evaluate(env, agent, n, exp_seed=seed, order="shuffled") == value
        assert routine.evaluate(env, agent, n, exp_seed=seed, order="sorted") == base
        assert routine.evaluate(env, agent, n, exp_seed=seed) == base
        assert env._eval_memo is memo
    finally:
        for e in getattr(env, "_eval_envs", {}).values():
            e.close()
        env.close()


# ------------------------------------------------------------------- 9. the overlay
def test_visualize_agent_attribution_overlay(tmp_path):
    from hwy.vec_env import HighwayVecEnv
    from ppo.agent import PPOAgent
    from training.routine import attribution_shade, visualize_agent

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=5, screen_width=96, screen_height=32)
    torch.manual_seed(0)
    agent = PPOAgent(60, 2, hidden_dim=64, device=DEV)
    n = 3
    env = HighwayVecEnv(cfg, num_envs=2, device=DEV)
    twin = HighwayVecEnv(cfg, num_envs=n, device=DEV, autoreset=False)
    try:
        recs = {}
        for name in (None, "value"):
            tape, out_dir = [], str(tmp_path / str(name))
            rewards = visualize_agent(env, agent, num_episodes=n, exp_seed=42, out_dir=out_dir,
                                      attribution=name, tape=tape)
            frames = [np.load(os.path.join(out_dir, f"viz_episode_{ep + 1}.npy")) for ep in range(n)]
            at = [0] * n
            for obs, state, running in tape:
                twin.import_state(state)
                shade = None
                if name is not None:
                    g = agent.input_gradients(obs.reshape(n, -1))[name]
                    shade = attribution_shade(twin, g)
                    assert 0.0 <= float(shade.min()) and float(shade.max()) <= 1.0
                want = twin.render(shade=shade).cpu().numpy()
                for ep in range(n):
                    if running[ep]:
                        assert np.array_equal(frames[ep][at[ep]], want[ep]), (name, ep, at[ep])
                        at[ep] += 1
            assert at == [len(f) for f in frames] and min(at) >= 2
            recs[name] = (rewards, frames)
        assert recs[None][0] == recs["value"][0]
        vehicle = np.array([100, 200, 255], np.uint8)
        changed = 0
        for plain, tinted in zip(recs[None][1], recs["value"][1]):
            assert plain.shape == tinted.shape
            diff = (plain != tinted).any(axis=-1)
            # a tint changes vehicle pixels only
            was_vehicle = np.zeros(diff.shape, bool)
            for colour in (vehicle, (50, 200, 0), (255, 100, 100)):   # traffic, the ego, crashed
                was_vehicle |= (plain == np.array(colour, np.uint8)).all(axis=-1)
            assert not (diff & ~was_vehicle).any()
            changed += int(diff.sum())
        assert changed > 0, "no vehicle pixel differs between the two recordings"
    finally:
        env.close()
        twin.close()


# ------------------------------------------------------------------- 10. the runner
def _exp(seed, on):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64, d_embed=None)
    hp.entropy_coef = 0.005
    hp.steps_per_update = 64  # 4 envs x 16 steps
    extra = {"num_envs": 4, "eval_interval": 4, "log_interval": 50}
    if on:
        extra["eval_orders"] = ["sorted", "shuffled"]
    return Experiment(name=f"orders{int(on)}_{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=12, target_reward=1e9, extra=extra,
                      env_config_overrides={"max_episode_steps": 12})


def test_launch_with_eval_orders_is_the_same_training(tmp_path, monkeypatch):
    import csv
    import json

    from experiments.runner import ExperimentRunner
    from training import routine

    monkeypatch.chdir(tmp_path)
    inner, calls = routine.evaluate, []

    def spy(env, agent, num_episodes=10, render=False, exp_seed=0, order=None):
        value = inner(env, agent, num_episodes, render, exp_seed, order)
        if order is not None:
            # the env's own order is the plain evaluation (at the same weights; no random draw)
            plain = inner(env, agent, num_episodes, render, exp_seed) if order == "sorted" else None
            calls.append((order, num_episodes, exp_seed, value, plain))
        return value

    monkeypatch.setattr(routine, "evaluate", spy)
    runs = {}
    for on in (False, True):
        agents = []

        class Runner(ExperimentRunner):
            def _create_agent(self, *a, **kw):
                agents.append(super()._create_agent(*a, **kw))
                return agents[-1]

        e = _exp(42, on)
        res = Runner(HIGHWAY_CONFIG).launch(e)
        assert res["status"] == "COMPLETED", res.get("error_message")
        torch.cuda.synchronize()
        res["weights"] = [p.detach().clone() for p in agents[0].actor_critic.parameters()]
        art = os.path.join("artifacts", "highway-ppo")
        res["json"] = json.load(open(os.path.join(art, f"training_metrics_{e.name}.json")))
        res["summary"] = list(csv.DictReader(open(os.path.join(art, f"summary_{e.name}.csv"))))[0]
        runs[on] = res
    on, off = runs[True], runs[False]
    assert on["rewards"] == off["rewards"] and on["avg_rewards"] == off["avg_rewards"]
    assert all(torch.equal(a, b) for a, b in zip(on["weights"], off["weights"]))
    assert on["summary"]["final_reward"] == off["summary"]["final_reward"]
    m1, m0 = on["metrics_history"], off["metrics_history"]
    assert set(m1) - {"order_rewards"} == set(m0) and "order_rewards" not in off["json"]
    for k in m0:
        if k in ("timestamps", "experiment_name"):
            continue
        if k == "policy_updates":
            assert [u["loss"] for u in m1[k]] == [u["loss"] for u in m0[k]]
        else:
            assert m1[k] == m0[k], k
    booked = m1["order_rewards"]
    assert booked == on["json"]["order_rewards"] and list(booked) == ["sorted", "shuffled"]
    assert all(np.isfinite(v) for v in booked.values())
    # the booked values are evaluate(num_episodes=10, order=name) after the training, and
    # `sorted`, this env's own order, is the plain evaluation at the final weights
    assert [c[:3] for c in calls] == [("sorted", 10, 42), ("shuffled", 10, 42)]
    assert booked == {c[0]: c[3] for c in calls}
    assert calls[0][4] == booked["sorted"]


def test_grouped_launches_refuse_eval_orders():
    from experiments.runner import ExperimentRunner

    with pytest.raises(ValueError, match="eval_orders"):
        ExperimentRunner.check_batch([[_exp(42, True), _exp(1042, True)]], own_schedules=True)
    with pytest.raises(ValueError, match="eval_orders"):
        ExperimentRunner(HIGHWAY_CONFIG).launch_group([_exp(42, True), _exp(1042, True)])
