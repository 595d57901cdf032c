"""hwy_sense on the device: the null sensor against hwy_observe's bits, visibility and counts
against tests/sense_model.py (exactly on the hand-stated states and for the draws, on every
decided entry for range and line of sight), the observation by composition with hwy_observe on
the perceived state, relaunch, graph capture and the Python surface.

Every launch of the kernel-level tests runs between guard words: each output sits inside a larger
buffer whose other words must come back untouched."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest
import torch

import sense_model as sm
import sense_util as su
from config.base_config import HIGHWAY_CONFIG
from env_util import HipEnv
from hwy import SensorModel, _abi
from parity_util import make_cfg, policy_actions
from test_observe_gpu import PE, Guarded, _vec, observe, same_bits, table_for

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
OUTPUTS = _abi.SENSE_OUTPUTS


def sense(hip, sensor, order=-1, outputs=OUTPUTS):
    """one hwy_sense launch on a HipEnv's handle between guard words; numpy results by name"""
    from hwy.native import check, lib

    E, N, Fo = hip.E, hip.N, hip.Fo
    words = {"obs": (E * N * Fo, torch.float32), "row_vehicle": (E * N, torch.int32),
             "visible": (E * 16, torch.uint8), "hidden": (E * 64, torch.float32),
             "counts": (E * 4, torch.int32)}
    bufs = {k: Guarded(*words[k]) for k in outputs}
    a = SensorModel.from_dict(sensor).fill(_abi.SenseArgs())
    a.order = int(order)
    for k, b in bufs.items():
        setattr(a, k, b.ptr())
    check(lib().hwy_sense(hip.h, ctypes.byref(a), None), "hwy_sense")
    torch.cuda.synchronize()
    shapes = {"obs": (E, N, Fo), "row_vehicle": (E, N), "visible": (E, 64), "hidden": (E, 64),
              "counts": (E, 4)}
    out = {}
    for k, b in bufs.items():
        b.check(k)
        out[k] = b.view.cpu().numpy().reshape(shapes[k])
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def stepped(cfg, table=None, steps=6, seed=5):
    """a HipEnv after `steps` steps of seeded random actions (autoresets included)"""
    hip = HipEnv(cfg, table)
    hip.reset()
    rng = np.random.default_rng(seed)
    for t in range(steps):
        hip.step(policy_actions(rng, cfg.num_envs, t))
    return hip


# ------------------------------------------------------------------- 1. the null sensor
def null_is_observe(hip, what):
    before = hip.state()
    for order in (-1, 0, 1):
        want = observe(hip, order)
        got = sense(hip, su.NULL, order)
        same_bits(got["obs"], want["obs"], f"{what}: obs, order {order}")
        assert np.array_equal(got["row_vehicle"], want["row_vehicle"]), f"{what}: map, order {order}"
        pres = sm.fields(hip.cfg, before)["present"]
        assert np.array_equal(got["visible"] != 0, pres), f"{what}: visible is not present"
        assert not got["hidden"].any() and not got["counts"][:, 1:].any()
    assert np.array_equal(before, hip.state()), f"{what}: the call changed the state"


@pytest.mark.parametrize("stored", ("sorted", "shuffled"))
@pytest.mark.parametrize("pe", list(PE))
def test_null_sensor_is_observe(pe, stored):
    kind, d = PE[pe]
    cfg = make_cfg(E=6, order=stored, pe=kind, d=d, max_episode_steps=5)
    hip = stepped(cfg, table_for(kind, d, cfg.obs_vehicles), steps=8)
    try:
        null_is_observe(hip, f"{pe} {stored}")
    finally:
        hip.close()


@pytest.mark.parametrize("E, N, cars", [(1, 2, 3), (16, 64, 63), (6, 2, 63), (16, 15, 3), (1, 64, 50)])
def test_null_sensor_is_observe_across_shapes(E, N, cars):
    kind, d = PE["rope"]
    cfg = make_cfg(E=E, N=N, vehicles_count=cars, order="shuffled", pe=kind, d=d)
    hip = stepped(cfg, table_for(kind, d, N), steps=4)
    try:
        null_is_observe(hip, f"E{E} N{N} {cars} cars")
    finally:
        hip.close()


@pytest.mark.parametrize("stored", ("sorted", "shuffled"))
def test_null_sensor_is_observe_with_per_group_rank_tables(stored):
    from hwy.native import check, lib

    kind, d = PE["rank"]
    cfg = make_cfg(E=6, order=stored, pe=kind, d=d, max_episode_steps=5)
    cfg.seed_stride = 2
    tables = np.stack([table_for(kind, d, cfg.obs_vehicles, seed=s) for s in (1, 2, 3)])
    hip = HipEnv(cfg, tables[0])
    try:
        hip.set_seed_groups([100, 2000, 30000], 2)
        t = np.ascontiguousarray(tables, np.float32)
        check(lib().hwy_set_pe_table(hip.h, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
              "hwy_set_pe_table")
        hip.reset()
        rng = np.random.default_rng(5)
        for t_ in range(7):
            hip.step(policy_actions(rng, 6, t_))
        null_is_observe(hip, f"groups {stored}")
        got = sense(hip, su.NULL)["obs"]
        assert not np.array_equal(got[0], got[2]) and not np.array_equal(got[2], got[4])
    finally:
        hip.close()


# ------------------------------------------------------------------- 2. against the model
def against_model(hip, sensor, what, exact=False):
    """visible, hidden and counts of one launch against the model; returns (kernel, model)"""
    st = hip.state()
    got = sense(hip, sensor)
    m = sm.sense(hip.cfg, st, sensor)
    if exact:
        assert not m["undecided"].any(), f"{what}: the model leaves entries undecided"
    ok = ~m["undecided"]
    bad = np.argwhere(((got["visible"] != 0) != m["visible"]) & ok)
    assert not len(bad), f"{what}: visible differs at {bad[:5].tolist()} ({len(bad)} entries)"
    rows = m["counts_ok"]
    assert np.array_equal(got["counts"][rows], m["counts"][rows]), f"{what}: counts"
    vis = got["visible"] != 0
    assert np.array_equal(got["hidden"].view(np.uint32), (m["present"] & ~vis).astype(np.float32).view(np.uint32))
    c = got["counts"]
    assert np.array_equal(c[:, 1] + c[:, 2] + c[:, 3] + vis[:, 1:].sum(1), c[:, 0]), f"{what}: counts do not add up"
    assert np.array_equal(c[:, 0], m["present"][:, 1:].sum(1))
    assert np.array_equal(vis[:, 0], m["present"][:, 0]) and not vis[~m["present"]].any()
    return got, m


def test_hand_stated_states_match_exactly():
    cfg = su.hand_cfg()
    hip = HipEnv(cfg)
    try:
        hip.set_state(su.hand_state(cfg))
        su.check_hand(lambda s: sense(hip, s)["visible"], "kernel: ")
        for s in (su.LOS, su.RANGE40, su.LOS40):
            against_model(hip, s, f"hand {s}", exact=True)
    finally:
        hip.close()


@pytest.mark.parametrize("name", list(su.NATURAL))
def test_line_of_sight_and_range_on_natural_states(name):
    cfg, st = su.natural_state(name)
    hip = HipEnv(cfg)
    try:
        hip.set_state(st)
        seen = 0
        for sensor in (su.LOS, SensorModel(range=120.0), SensorModel(los=True, range=120.0), su.FULL):
            got, m = against_model(hip, sensor, f"{name} {sensor}")
            seen += int(m["blocked"].sum() + (~m["in_range"]).sum())
        assert seen or cfg.vehicles_count < 50
    finally:
        hip.close()


@pytest.mark.parametrize("sensor", [SensorModel(dropout=0.3), SensorModel(dropout=1.0),
                                    SensorModel(dropout=0.3, salt=65535),
                                    SensorModel(noise=(2.0, 1.0, 3.0), salt=2)], ids=repr)
def test_dropout_alone_and_noise_alone_are_exact(sensor):
    cfg, st = su.natural_state("E6-N15-50cars")
    hip = HipEnv(cfg)
    try:
        hip.set_state(st)
        got, m = against_model(hip, sensor, repr(sensor), exact=True)
        if sensor.dropout:
            assert np.array_equal(got["counts"][:, 3], (m["dropped"] & m["present"])[:, 1:].sum(1))
            assert got["counts"][:, 3].sum() > 0
        else:
            assert np.array_equal(got["visible"] != 0, m["present"])
    finally:
        hip.close()


def test_ring_at_the_range_stays_in_range_under_noise():
    cfg = make_cfg(E=4, vehicles_count=len(su.RING), N=5)
    hip = HipEnv(cfg)
    try:
        hip.set_state(su.ring_state(cfg))
        got, _ = against_model(hip, su.RING_SENSOR, "ring", exact=True)
        assert (got["visible"][:, 1:len(su.RING) + 1] != 0).all()
    finally:
        hip.close()


# ------------------------------------------------------------------- 3. composition
@pytest.mark.parametrize("name, pe", [("E6-N15-50cars", "rank"), ("E6-N15-50cars-shuffled", "dist"),
                                      ("E16-N64-63cars", "rope"), ("E1-N2-3cars", "none")])
def test_obs_is_observe_of_the_perceived_state(name, pe):
    """the kernel's own visible and the model's perturbed x, y and speed, imported into a second
    handle: its hwy_observe is hwy_sense's obs and map, bit for bit, under either order"""
    kind, d = PE[pe]
    cfg, st = su.natural_state(name, pe=kind, d=d)
    table = table_for(kind, d, cfg.obs_vehicles)
    hip, twin = HipEnv(cfg, table), HipEnv(cfg, table)
    try:
        hip.set_state(st)
        for sensor in (su.FULL, SensorModel(noise=(3.0, 0.5, 2.0)), SensorModel(los=True, range=150.0)):
            m = sm.sense(cfg, st, sensor)
            for order in (-1, 0, 1):
                got = sense(hip, sensor, order)
                twin.set_state(sm.perceived_state(cfg, st, got["visible"] != 0, m))
                want = observe(twin, order)
                same_bits(got["obs"], want["obs"], f"{name} {sensor} order {order}: obs")
                assert np.array_equal(got["row_vehicle"], want["row_vehicle"]), f"{name} {sensor} {order}"
            if cfg.vehicles_count >= 50:
                assert not np.array_equal(got["obs"], observe(hip, order)["obs"])
        assert np.array_equal(hip.state(), st), "the calls changed the state"
    finally:
        hip.close()
        twin.close()


def test_hidden_vehicles_leave_the_rows_and_the_rows_close_up():
    cfg = su.hand_cfg()
    hip = HipEnv(cfg)
    try:
        hip.set_state(su.hand_state(cfg))
        e = su.HAND_NAMES.index("leader")
        # by |dx|: 4 alongside, the leader 1, 3 in the next lane, then 2 -- which the leader hides
        assert list(observe(hip, 0)["row_vehicle"][e]) == [0, 4, 1, 3, 2]
        assert list(sense(hip, su.LOS, 0)["row_vehicle"][e]) == [0, 4, 1, 3, -1]
        e = su.HAND_NAMES.index("chain")
        assert list(observe(hip, 0)["row_vehicle"][e]) == [0, 1, 2, 3, -1]
        assert list(sense(hip, su.LOS, 0)["row_vehicle"][e]) == [0, 1, -1, -1, -1]
    finally:
        hip.close()


# ------------------------------------------------------------------- 4. outputs, relaunch, capture
def test_every_single_output_and_a_relaunch_give_the_same_bits():
    cfg, st = su.natural_state("E6-N15-50cars")
    hip = HipEnv(cfg)
    try:
        hip.set_state(st)
        for order in (-1, 1):
            full = sense(hip, su.FULL, order)
            again = sense(hip, su.FULL, order)
            for k in OUTPUTS:
                assert np.array_equal(bits(full[k]), bits(again[k])), f"relaunch: {k}"
                part = sense(hip, su.FULL, order, outputs=(k,))
                assert np.array_equal(bits(part[k]), bits(full[k])), f"{k} alone"
            pair = sense(hip, su.FULL, order, outputs=("row_vehicle", "counts"))
            assert all(np.array_equal(bits(pair[k]), bits(full[k])) for k in pair)
        other = sense(hip, SensorModel.from_dict({**su.FULL.to_dict(), "salt": 8}))
        assert not np.array_equal(other["visible"], full["visible"])
        assert not np.array_equal(bits(other["obs"]), bits(sense(hip, su.FULL)["obs"]))
    finally:
        hip.close()


def test_captured_sense_replays_on_the_later_state():
    from utils.graphs import capture

    env = _vec(6)
    try:
        env.reset(seed=3)
        E, N, Fo = 6, env.obs_rows, env.obs_features
        kw = dict(obs=torch.zeros(E, N, Fo, device=DEV),
                  row_vehicle=torch.zeros(E, N, dtype=torch.int32, device=DEV),
                  visible=torch.zeros(E, 64, dtype=torch.uint8, device=DEV),
                  hidden=torch.zeros(E, 64, device=DEV),
                  counts=torch.zeros(E, 4, dtype=torch.int32, device=DEV))
        env.sense_into(su.FULL, "shuffled", **kw)  # eager first: the code object loads outside the capture
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                env.sense_into(su.FULL, "shuffled", **kw)
        torch.cuda.current_stream().wait_stream(s)
        first = {k: t.clone() for k, t in kw.items()}
        for _ in range(3):
            env.step(torch.full((E, 2), 0.3, device=DEV))
        for t in kw.values():
            t.zero_()
        g.replay()
        torch.cuda.synchronize()
        eager = {k: torch.zeros_like(t) for k, t in kw.items()}
        env.sense_into(su.FULL, "shuffled", **eager)
        torch.cuda.synchronize()
        for k in kw:
            assert torch.equal(kw[k].view(torch.uint8), eager[k].view(torch.uint8)), k
        assert not torch.equal(kw["obs"], first["obs"])
    finally:
        env.close()


# ------------------------------------------------------------------- 5. the Python surface
def test_conveniences_and_the_one_env_facade():
    from hwy.single_env import HighwayEnv

    env = _vec(4, order="shuffled", autoreset=True)
    try:
        step_obs, _ = env.reset(seed=11)
        env.step(torch.full((4, 2), 0.1, device=DEV))
        E, N, Fo = 4, env.obs_rows, env.obs_features
        o = env.sense(SensorModel())
        assert o.shape == (E, N, Fo) and o.dtype == torch.float32 and torch.equal(o, step_obs)
        assert torch.equal(env.sense({}, "sorted"), env.observe("sorted"))
        buf = torch.empty(E * N * Fo, device=DEV)
        assert env.sense(su.FULL, out=buf).data_ptr() == buf.data_ptr()
        assert not torch.equal(buf.view(E, N, Fo), o)
        hid = env.hidden_vehicles(su.FULL)
        assert hid.shape == (E, 64) and hid.dtype == torch.float32 and hid.sum() > 0
        m = sm.sense(env.hwy_config, env.export_state().cpu().numpy().view(np.uint32), su.FULL)
        ok = ~m["undecided"]
        assert np.array_equal(hid.cpu().numpy()[ok], m["hidden"][ok])
        assert not torch.equal(env.render(shade=hid), env.render())   # the layout render takes
        with pytest.raises(ValueError, match="at least one"):
            env.sense_into(su.FULL)
        with pytest.raises(ValueError, match="order must be"):
            env.sense(su.FULL, "reversed")
        with pytest.raises(ValueError, match="dropout"):
            env.sense({"dropout": 3})
        with pytest.raises(ValueError, match="^obs must be"):
            env.sense(su.FULL, out=torch.zeros(5, device=DEV))
        with pytest.raises(ValueError, match="^visible must be"):
            env.sense_into(su.FULL, visible=torch.zeros(E, 64, dtype=torch.bool, device=DEV))
    finally:
        env.close()
    one = HighwayEnv(HIGHWAY_CONFIG)
    try:
        first, _ = one.reset(seed=5)
        got = one.sense(SensorModel())
        assert isinstance(got, np.ndarray) and got.shape == first.shape and np.array_equal(got, first)
        assert not np.array_equal(one.sense(su.FULL), first)
    finally:
        one.close()


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
        assert torch.equal(env.sense(su.NULL), env.obs_buf)
        env.set_seed_groups(None)
        with pytest.raises(ValueError, match="hwy_sense"):
            env.sense(su.NULL)
        env.set_pe_table(table_for(kind, d, N))
        env.sense(su.NULL)
    finally:
        env.close()
