"""hwy_lidar on the device: the hand-stated cases, the kernel against tests/lidar_model.py on
natural states over the shapes at which it can go wrong, the padding and what lies past the
outputs, every subset of outputs, that it only reads, a lone car's exact range without a model,
graph capture, that it follows the state, the refusals, and the Python surface.

Every kernel-level call runs between guard words: each output sits inside a larger NaN-filled
buffer whose other words must come back untouched."""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest
import torch

import lidar_cases as lc
import lidar_model as lm
from config.base_config import HIGHWAY_CONFIG
from env_util import HipEnv, _put
from hwy import LidarSpec, _abi
from parity_util import make_cfg, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 256            # words on either side of every buffer
CANARY = 0x7FC0BEEF    # a NaN no output holds
FILL = 0x7FC12345      # another one, where the kernel must write
OUTPUTS = ("obs", "hit_vehicle", "seen", "counts")


class Guarded:
    """n 32-bit words between two runs of NaN canaries"""

    def __init__(self, n):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), CANARY, dtype=torch.int32, device=DEV)
        self.mid = self.buf[GUARD:GUARD + n]
        self.mid.fill_(FILL)

    def check(self, name):
        b = self.buf.cpu().numpy()
        assert (b[:GUARD] == CANARY).all() and (b[GUARD + self.n:] == CANARY).all(), \
            f"{name}: a word outside the output was written"

    def words(self):
        return self.mid.cpu().numpy().view(np.uint32)


def sizes(spec, E, F, stride=None):
    return {"obs": E * (spec.stride(F) if stride is None else stride),
            "hit_vehicle": E * spec.cells, "seen": E * 64, "counts": E * 4}


def lidar_call(hip, spec, outputs=OUTPUTS, stride=None, expect=0, **override):
    """one hwy_lidar launch on a HipEnv's handle; numpy results by name (all of them written in
    full, or with expect = HWY_EINVAL none of them touched)"""
    from hwy.native import HWY_EINVAL, last_error, lib

    F = hip.cfg.n_features
    a = spec.fill(_abi.LidarArgs(), F)
    if stride is not None:
        a.row_stride = stride
    bufs = {k: Guarded(n) for k, n in sizes(spec, hip.E, F, stride).items() if k in outputs}
    for k, b in bufs.items():
        setattr(a, k, b.mid.data_ptr())
    for k, v in override.items():
        setattr(a, k, v)
    rc = lib().hwy_lidar(hip.h, ctypes.byref(a), None)
    torch.cuda.synchronize()
    assert rc == expect, (rc, last_error())
    for k, b in bufs.items():
        b.check(k)
    if expect == HWY_EINVAL:
        for k, b in bufs.items():
            assert (b.words() == FILL).all(), f"{k} was written by a refused call"
        return last_error()
    out = {}
    for k, b in bufs.items():
        w = b.words()
        assert not (w == FILL).any(), f"{k}: an entry was left unwritten"
        out[k] = w.view(np.float32 if k in ("obs", "seen") else np.int32).reshape(hip.E, -1)
    return out


def consistent(hip, spec, got, what):
    """what the model leaves open, the kernel still keeps consistent with itself: seen, counts
    and hit_vehicle say the same, and a cell without a vehicle is written as no return"""
    V, n = hip.cfg.vehicles_count + 1, spec.cells
    hv, seen, cn, obs = got["hit_vehicle"], got["seen"], got["counts"], got["obs"]
    assert ((hv == -1) | ((hv >= 1) & (hv < V))).all(), f"{what}: a hit_vehicle out of 1..V-1"
    assert np.isin(seen, (0.0, 1.0)).all() and not np.signbit(seen).any()
    present = (hip.state()[_abi.F_FLAGS][:, :V] & _abi.FLAG_PRESENT) != 0
    none = (np.float32(1.0) if spec.normalize else np.float32(spec.range_m), np.float32(0.0))
    for e in range(hip.E):
        want = np.zeros(64, np.float32)
        want[hv[e][hv[e] >= 0]] = 1.0
        assert np.array_equal(seen[e], want), f"{what}: env {e}: seen is not the set of returns"
        assert cn[e, 0] == present[e, 1:].sum() and cn[e, 1] == want.sum()
        assert cn[e, 2] == (hv[e] >= 0).sum() and 0 <= cn[e, 3] <= n - cn[e, 2]
        assert present[e][hv[e][hv[e] >= 0]].all(), f"{what}: env {e}: an absent vehicle returned"
        d, v = obs[e, 0:2 * n:2], obs[e, 1:2 * n:2]
        empty = hv[e] < 0
        assert (d[empty] == none[0]).all() and (v[empty].view(np.uint32) == 0).all(), \
            f"{what}: env {e}: a cell without a vehicle is not (range, +0.0)"
    if spec.p_drop == 0.0:
        assert (cn[:, 3] == 0).all()
    if spec.p_drop == 1.0:
        assert (cn[:, 3] == n).all() and (hv == -1).all() and not seen.any()


def check_against_model(hip, spec, what, stride=None):
    """every output against the model on the handle's state; (cells, undecided, returning)"""
    F = hip.cfg.n_features
    st = hip.state()
    got = lidar_call(hip, spec, stride=stride)
    assert np.array_equal(st, hip.state()), f"{what}: hwy_lidar changed the state"
    m = lm.lidar_model(hip.cfg, st, spec)
    width = spec.width(F)
    assert (got["obs"][:, width:].view(np.uint32) == 0).all(), f"{what}: padding is not +0.0"
    if stride is not None:   # the model pads to spec.stride: compare the width, then the padding
        got = dict(got, obs=np.ascontiguousarray(np.concatenate(
            [got["obs"][:, :width], np.zeros((hip.E, spec.stride(F) - width), np.float32)], 1)))
    lm.compare(m, got, what + ": ")
    consistent(hip, spec, got, what)
    return m.cells, m.undecided, m.returning


# ------------------------------------------------------------------- 0. what the model assumes
def test_device_sin_and_cos_are_exact_at_zero():
    from hwy import ops

    x = torch.zeros(4, device=DEV)
    assert (ops.math_selftest(0, x).cpu().numpy().view(np.uint32) == 0).all()           # +0.0
    assert (ops.math_selftest(1, x).cpu().numpy() == np.float32(1.0)).all()


# ------------------------------------------------------------------- 1. the hand-stated cases
def test_kernel_gives_the_hand_cases():
    cfg = lc.hand_cfg()
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(lc.hand_state(cfg))
        outs = {spec: lidar_call(hip, spec) for spec in lc.SPECS}
        for e, name in enumerate(lc.CASE_NAMES):
            lc.check_case(name, e, cfg.n_features, **outs[lc.CASES[name]["spec"]])
    finally:
        hip.close()
    cfg = lc.v1_cfg()
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(lc.v1_state(cfg))
        lc.check_case(lc.V1_CASE, 0, cfg.n_features, **lidar_call(hip, lc.V1_SPEC))
    finally:
        hip.close()


# ------------------------------------------------------------------- 2. natural states
_OFF = dict(normalize=False, ego_tail=False, pad_to=1)
SPECS = {
    # one cell; 63, 64 and 65 cells and rays straddle the lane-strided loop's boundary; 1,024
    # cells and 4,096 rays are the caps; sub 1, 2 and 16
    "1": LidarSpec(cells=1, align=True, **_OFF),
    "1x16": LidarSpec(cells=1, sub=16, range_m=80.0, align=True),
    "63-errors": LidarSpec(cells=63, p_drop=0.3, sigma_r=0.5, salt=7, range_m=45.0),
    "64": LidarSpec(cells=64, speed_scale=25.0),
    "32x2-aligned": LidarSpec(cells=32, sub=2, align=True, **_OFF),
    "65-all-dropped": LidarSpec(cells=65, p_drop=1.0, sigma_r=1.0),
    "4x16-noise": LidarSpec(cells=4, sub=16, sigma_r=0.25, salt=65535, align=True, **_OFF),
    "21x3": LidarSpec(cells=21, sub=3, align=True, pad_to=8),
    "13x5": LidarSpec(cells=13, sub=5, normalize=False),
    "1024": LidarSpec(cells=1024, align=True, range_m=100.0),
    "1024x4": LidarSpec(cells=1024, sub=4, align=True, p_drop=0.3, salt=1, **_OFF),
    "256x16": LidarSpec(cells=256, sub=16, align=True),
    "default": LidarSpec(),
}
# (E, vehicles_count, lanes_count, spec): E in {1, 5, 16} (partial blocks), vehicles_count in {0, 1,
# 20, 63} (V = 1, 2 and 64), every spec
NATURAL = [(1, 0, 4, "1"), (5, 63, 4, "1x16"), (16, 20, 4, "63-errors"), (5, 63, 4, "64"),
           (16, 63, 2, "32x2-aligned"), (5, 20, 4, "65-all-dropped"), (5, 63, 4, "4x16-noise"),
           (16, 1, 4, "21x3"), (5, 63, 8, "13x5"), (5, 63, 4, "1024"), (5, 63, 4, "1024x4"),
           (1, 63, 4, "256x16"), (16, 63, 4, "default"), (5, 1, 1, "64"), (1, 20, 4, "default")]


def drive(hip, steps, seed=5, steer=0.3):
    rng = np.random.default_rng(seed)
    hip.reset()
    for t in range(steps):
        a = np.tanh(rng.normal(size=(hip.E, 2)) * np.array([0.6, steer])).astype(np.float32)
        hip.step(a)
    return rng


@pytest.mark.parametrize("E, vc, lanes, name", NATURAL)
def test_kernel_against_model_on_natural_states(E, vc, lanes, name):
    spec = SPECS[name]
    cfg = make_cfg(E=E, vehicles_count=vc, lanes_count=lanes, max_episode_steps=30)
    hip = HipEnv(cfg)
    try:
        rng = drive(hip, 3, seed=E + vc)
        tag = f"{name} E{E} V{vc} L{lanes}"
        cells, und, ret = check_against_model(hip, spec, tag + " as it is")
        # once more with the ego moved into the traffic, where the lidar has returns
        hip.set_state(lc.ego_into_traffic(cfg, hip.state(), rng))
        c, u, r = check_against_model(hip, spec, tag + " in traffic")
        cells, und, ret = cells + c, und + u, ret + r
        print(f"{tag}: {und} of {cells} cells undecided, {ret} return")
        # the comparison is not mostly skipped (sub > 1 unaligned: mirror-symmetric sub-rays tie
        # up to rounding on a natural ego, tests/test_lidar_model.py)
        assert und <= max(2, 0.05 * cells)
        if vc >= 20 and spec.cells * spec.sub >= 16:
            assert ret >= E, "no returns: the comparison shows nothing"
    finally:
        hip.close()


def test_the_shapes_cover_what_the_kernel_branches_on():
    assert {s.cells for s in SPECS.values()} >= {1, 63, 64, 65, 1024}
    assert {s.cells * s.sub for s in SPECS.values()} >= {63, 64, 65, 4096}
    assert {s.sub for s in SPECS.values()} >= {1, 2, 16}
    for flag in ("align", "normalize", "ego_tail"):
        assert {getattr(s, flag) for s in SPECS.values()} == {True, False}, flag
    assert {s.p_drop for s in SPECS.values()} >= {0.0, 0.3, 1.0}
    assert {s.sigma_r == 0 for s in SPECS.values()} == {True, False}
    assert {n[0] for n in NATURAL} == {1, 5, 16} and {n[1] for n in NATURAL} >= {0, 1, 63}
    assert {n[3] for n in NATURAL} == set(SPECS)


# ------------------------------------------------------------------- 3. padding and bounds
@pytest.mark.parametrize("extra", [0, 3])
def test_a_custom_row_stride(extra):
    spec = SPECS["21x3"]
    cfg = make_cfg(E=5, vehicles_count=20, max_episode_steps=30)
    width = spec.width(cfg.n_features)
    assert width == 46 and spec.stride(cfg.n_features) == 48
    hip = HipEnv(cfg)
    try:
        rng = drive(hip, 4)
        hip.set_state(lc.ego_into_traffic(cfg, hip.state(), rng))
        check_against_model(hip, spec, f"row_stride = width + {extra}", stride=width + extra)
    finally:
        hip.close()


def test_every_combination_of_outputs():
    spec = SPECS["63-errors"]
    cfg = make_cfg(E=5, vehicles_count=20)
    hip = HipEnv(cfg)
    try:
        rng = drive(hip, 3)
        hip.set_state(lc.ego_into_traffic(cfg, hip.state(), rng))
        full = lidar_call(hip, spec)
        assert (full["hit_vehicle"] >= 0).any()
        n = 0
        for mask in range(1, 16):
            names = tuple(k for i, k in enumerate(OUTPUTS) if mask >> i & 1)
            part = lidar_call(hip, spec, outputs=names)
            assert set(part) == set(names)
            assert all(np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)) for k in part)
            n += 1
        assert n == 15
    finally:
        hip.close()


# ------------------------------------------------------------------- 4. without a model
def test_a_lone_car_dead_ahead_returns_its_gap_exactly():
    """a car at heading 0 whose centre is g ahead of the ego's, nothing else: cell 0 is exactly
    g - 2.5 and its speed difference, every other cell has no return (16 cells: none of the other
    rays meets a body 2 m wide at 8 m or more)"""
    gaps = [8.0, 12.5, 20.0, 33.25, 47.0, 62.5]
    cfg = make_cfg(E=len(gaps), vehicles_count=3)
    spec = LidarSpec(cells=16, range_m=60.0, **_OFF)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        st = np.zeros((_abi.NFIELDS, cfg.num_envs, 64), np.uint32)
        for e, g in enumerate(gaps):
            _put(st, e, 0, 300.0, 8.0, speed=20.0)
            _put(st, e, 2, 300.0 + g, 8.0, speed=20.0 + e)
        hip.set_state(st)
        got = lidar_call(hip, spec)
        for e, g in enumerate(gaps):
            assert got["obs"][e, 0] == np.float32(g - 2.5) and got["obs"][e, 1] == np.float32(e)
            assert got["hit_vehicle"][e].tolist() == [2] + [-1] * 15
            assert (got["obs"][e, 2::2] == np.float32(60.0)).all() and not got["obs"][e, 3::2].any()
            assert got["counts"][e].tolist() == [1, 1, 1, 0]
            assert np.flatnonzero(got["seen"][e]).tolist() == [2]
    finally:
        hip.close()


def test_lidar_follows_reset_autoreset_and_cut():
    spec = SPECS["default"]
    cfg = make_cfg(E=6, max_episode_steps=3)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        check_against_model(hip, spec, "after reset")
        rng = np.random.default_rng(2)
        resets = 0
        for t in range(4):
            out = hip.step(policy_actions(rng, 6, t))
            resets += int((out[2] | out[3]).sum())
            check_against_model(hip, spec, f"after step {t}")
        assert resets >= 6
        hip.cut_episodes()
        check_against_model(hip, spec, "after cut_episodes")
        hip.reset(9000 + np.arange(6), (np.arange(6) % 2).astype(np.uint8))
        check_against_model(hip, spec, "after a masked seeded reset")
    finally:
        hip.close()


def test_the_errors_follow_the_step_word_the_seed_and_the_salt():
    """the draws are keyed by (cell, step, channel, salt) and the episode's seed: the same state
    gives the same rows twice; another salt, another step word or another seed gives other drops"""
    spec = LidarSpec(cells=64, p_drop=0.5, salt=3, **_OFF)
    cfg = make_cfg(E=4, vehicles_count=20)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        st = hip.state()
        a = lidar_call(hip, spec)
        b = lidar_call(hip, spec)
        assert all(np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)) for k in a)
        drops = lambda s, sp=spec: lm.lidar_model(cfg, s, sp).dropped  # noqa: E731
        assert np.array_equal(a["counts"][:, 3], drops(st).sum(1))
        salted = LidarSpec(cells=64, p_drop=0.5, salt=4, **_OFF)
        assert not np.array_equal(drops(st, salted), drops(st))
        other = lidar_call(hip, salted)
        assert np.array_equal(other["counts"][:, 3], drops(st, salted).sum(1))
        st2 = st.copy()
        st2[_abi.F_ENV][:, _abi.E_STEP] += 1
        st2[_abi.F_ENV][:, _abi.E_SEED_HI] ^= 0x55
        assert not np.array_equal(drops(st2), drops(st))
        hip.set_state(st2)
        c = lidar_call(hip, spec)
        assert np.array_equal(c["counts"][:, 3], drops(st2).sum(1))
    finally:
        hip.close()


# ------------------------------------------------------------------- 5. capture
def _vec(E, autoreset=False, **kw):
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(kw)
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=autoreset)


def test_captured_lidar_replays_bit_identically_and_on_the_later_state():
    from utils.graphs import capture

    env = _vec(5)
    spec = LidarSpec(cells=63, sub=2, align=True)   # no dropout, no noise
    try:
        env.reset(seed=3)
        E, F = 5, 4
        kw = dict(out=torch.zeros(E, spec.stride(F), device=DEV),
                  hit_vehicle=torch.zeros(E, spec.cells, dtype=torch.int32, device=DEV),
                  seen=torch.zeros(E, 64, device=DEV),
                  counts=torch.zeros(E, 4, dtype=torch.int32, device=DEV))
        env.lidar_into(spec, **kw)  # eager first: the code object loads outside the capture
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                env.lidar_into(spec, **kw)
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        first = {k: t.clone() for k, t in kw.items()}
        for t in kw.values():
            t.fill_(-7)
        g.replay()  # the same state: the same bits
        torch.cuda.synchronize()
        for k in kw:
            assert torch.equal(kw[k].view(torch.int32), first[k].view(torch.int32)), k
        for _ in range(3):
            env.step(torch.full((E, 2), 0.3, device=DEV))
        for t in kw.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager = {k: torch.full_like(t, -9) for k, t in kw.items()}
        env.lidar_into(spec, **eager)
        torch.cuda.synchronize()
        for k in kw:
            assert torch.equal(kw[k].view(torch.int32), eager[k].view(torch.int32)), k
        assert not torch.equal(kw["out"], first["out"])
    finally:
        env.close()


# ------------------------------------------------------------------- 6. the refusals
def test_each_refusal_leaves_the_outputs_untouched():
    from hwy.native import HWY_EINVAL

    cfg = make_cfg(E=3, vehicles_count=5)
    spec = LidarSpec()
    hip = HipEnv(cfg)
    nan, inf = float("nan"), float("inf")
    try:
        hip.reset()
        before = hip.state()
        for word, kw in (
                ("cells must", dict(cells=0)), ("cells must", dict(cells=1025)),
                ("sub must", dict(sub=0)), ("sub must", dict(sub=17)),
                ("cells * sub", dict(cells=1024, sub=5, row_stride=4096)),
                ("range_m and speed_scale", dict(range_m=0.0)),
                ("range_m and speed_scale", dict(range_m=inf)),
                ("range_m and speed_scale", dict(speed_scale=nan)),
                ("range_m and speed_scale", dict(speed_scale=-1.0)),
                ("p_drop", dict(p_drop=-0.5)), ("p_drop", dict(p_drop=1.25)), ("p_drop", dict(p_drop=nan)),
                ("sigma_r", dict(sigma_r=-1.0)), ("sigma_r", dict(sigma_r=inf)),
                ("salt", dict(salt=-1)), ("salt", dict(salt=65536)),
                ("row_stride", dict(row_stride=32)), ("row_stride", dict(row_stride=4097)),
                # the handle's four features: the width is 36
                ("below the width", dict(row_stride=35))):
            msg = lidar_call(hip, spec, stride=40, expect=HWY_EINVAL, **kw)
            assert word in msg, (word, msg)
        msg = lidar_call(hip, spec, outputs=(), expect=HWY_EINVAL)
        assert "no output" in msg
        assert np.array_equal(before, hip.state())
        lidar_call(hip, spec, stride=36)   # the width itself is taken
    finally:
        hip.close()


# ------------------------------------------------------------------- 7. the Python surface
def test_python_surface_and_the_one_env_facade():
    from hwy.single_env import HighwayEnv

    env = _vec(4, autoreset=True)
    spec = LidarSpec()
    try:
        env.reset(seed=11)
        env.step(torch.full((4, 2), 0.1, device=DEV))
        g = env.lidar(spec)
        assert g.shape == (4, 36) and g.dtype == torch.float32
        assert torch.equal(g, env.lidar(True)) and torch.equal(g, env.lidar(spec.to_dict()))
        buf = torch.empty(4 * 36, device=DEV)
        assert env.lidar(spec, out=buf).data_ptr() == buf.data_ptr()
        hits = env.lidar_hits(spec)
        assert hits.shape == (4, 16) and hits.dtype == torch.int32
        assert torch.equal(g[:, 0:32:2] < 1.0, (hits >= 0) & (g[:, 0:32:2] < 1.0))
        st = env.export_state().cpu().numpy().view(np.uint32)
        m = lm.lidar_model(env.hwy_config, st, spec)
        seen = torch.zeros(4, 64, device=DEV)
        cn = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
        env.lidar_into(spec, seen=seen, counts=cn)
        lm.compare(m, dict(obs=g.cpu().numpy(), hit_vehicle=hits.cpu().numpy(),
                           seen=seen.cpu().numpy(), counts=cn.cpu().numpy()))
        with pytest.raises(ValueError, match="^out must be"):
            env.lidar_into(spec, out=torch.zeros(4, 40, device=DEV))
        with pytest.raises(ValueError, match="^counts must be"):
            env.lidar_into(spec, counts=torch.zeros(4, 4, device=DEV))
        with pytest.raises(ValueError, match="at least one"):
            env.lidar_into(spec)
        with pytest.raises(ValueError, match="unknown lidar keys"):
            env.lidar({"nx": 3})
    finally:
        env.close()
    one = HighwayEnv(HIGHWAY_CONFIG)
    try:
        one.reset(seed=5)
        one.step(np.array([0.1, 0.0], np.float32))
        row = one.lidar(spec)
        assert isinstance(row, np.ndarray) and row.shape == (36,) and row.dtype == np.float32
        st = one.vec_env.export_state().cpu().numpy().view(np.uint32)
        lm.compare(lm.lidar_model(one.vec_env.hwy_config, st, spec), dict(obs=row[None]))
    finally:
        one.close()
