"""hwy_grid on the device: the hand-stated cases, the kernel against tests/grid_model.py on natural
states over the shapes at which it can go wrong, the padding and what lies past the outputs, the
grid against hwy_observe's own bits without a model, that it only reads, graph capture, that it
follows the state, the refusals, and the Python surface.

Every kernel-level call runs between guard words: each output sits inside a larger NaN-filled
buffer whose other words must come back untouched."""

from __future__ import annotations

import copy
import ctypes

import numpy as np
import pytest
import torch

import grid_cases as gc
import grid_model as gm
from config.base_config import HIGHWAY_CONFIG
from env_util import HipEnv
from hwy import GridSpec, _abi
from parity_util import make_cfg, pe_table_for, policy_actions

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
GUARD = 256            # words on either side of every buffer
CANARY = 0x7FC0BEEF    # a NaN no output holds
FILL = 0x7FC12345      # another one, where the kernel must write
OUTPUTS = ("grid", "cell_vehicle", "veh_cell", "counts")


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
    return {"grid": E * (spec.stride(F) if stride is None else stride),
            "cell_vehicle": E * spec.nx * spec.ny, "veh_cell": E * 64, "counts": E * 4}


def grid_call(hip, spec, outputs=OUTPUTS, stride=None, expect=0, **override):
    """one hwy_grid launch on a HipEnv's handle; numpy results by name (all of them written in
    full, or with expect = HWY_EINVAL none of them touched)"""
    from hwy.native import HWY_EINVAL, last_error, lib

    F = hip.cfg.n_features
    a = spec.fill(_abi.GridArgs(), F)
    if stride is not None:
        a.row_stride = stride
    bufs = {k: Guarded(n) for k, n in sizes(spec, hip.E, F, stride).items() if k in outputs}
    for k, b in bufs.items():
        setattr(a, k, b.mid.data_ptr())
    for k, v in override.items():
        setattr(a, k, v)
    rc = lib().hwy_grid(hip.h, ctypes.byref(a), None)
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
        out[k] = w.view(np.float32 if k == "grid" else np.int32).reshape(hip.E, -1)
    return out


def check_against_model(hip, spec, what, stride=None):
    """every output against the model on the handle's state; (pairs, undecided, others inside)"""
    F = hip.cfg.n_features
    st = hip.state()
    got = grid_call(hip, spec, stride=stride)
    assert np.array_equal(st, hip.state()), f"{what}: hwy_grid changed the state"
    m = gm.grid_model(hip.cfg, st, spec)
    width = spec.width(F)
    if stride is not None:   # the model pads to spec.stride: compare the width, then the padding
        assert (got["grid"][:, width:].view(np.uint32) == 0).all(), f"{what}: padding is not +0.0"
        got["grid"] = np.ascontiguousarray(
            np.concatenate([got["grid"][:, :width],
                            np.zeros((hip.E, spec.stride(F) - width), np.float32)], 1))
    gm.compare(m, got, what + ": ")
    assert (got["grid"][:, width:].view(np.uint32) == 0).all(), f"{what}: padding is not +0.0"
    # what the model leaves open, the kernel still keeps consistent with itself
    vc, cv, cn = got["veh_cell"], got["cell_vehicle"], got["counts"]
    V = hip.cfg.vehicles_count + 1
    assert (vc[:, V:] == -1).all() and ((vc >= -1) & (vc < spec.nx * spec.ny)).all()
    for e in range(hip.E):
        ins = np.flatnonzero(vc[e] >= 0)
        want = np.full(spec.nx * spec.ny, -1, np.int32)
        for k in ins[::-1]:
            want[vc[e, k]] = k
        assert np.array_equal(cv[e], want), f"{what}: env {e}: cell_vehicle is not the least index"
        others = ins[ins >= 1]
        assert cn[e, 1] == len(others) and cn[e, 1] + cn[e, 3] == cn[e, 0]
        assert cn[e, 2] == sum(cv[e, vc[e, k]] != k for k in others)
    return m.pairs, m.undecided, int(cn[:, 1].sum())


# ------------------------------------------------------------------- 1. the hand-stated cases
def test_kernel_gives_the_hand_cases():
    cfg = gc.hand_cfg()
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(gc.hand_state(cfg))
        outs = {spec: grid_call(hip, spec) for spec in gc.SPECS}
        for e, name in enumerate(gc.CASE_NAMES):
            gc.check_case(name, e, cfg.n_features, **outs[gc.CASES[name]["spec"]])
    finally:
        hip.close()


# ------------------------------------------------------------------- 2. natural states
_R4 = {"x": (-100.0, 100.0), "y": (-16.0, 16.0), "vx": (-80.0, 80.0), "vy": (-80.0, 80.0)}
SPECS = {
    # one cell; 63, 64 and 65 cells straddle the lane-strided loops' boundary; 1,024 is the cap.
    # The ego (u = w = 0) is in the middle of its cell in each, so an aligned ego is decided.
    "1x1": GridSpec(layers=("presence",), nx=1, ny=1, x0=-50.0, y0=-8.0, step_x=100.0, step_y=16.0,
                    ego_tail=False, pad_to=1),
    "7x9-8layers": GridSpec(layers=("presence", "x", "y", "vx", "vy", "cos_h", "sin_h", "on_road"),
                            nx=7, ny=9, x0=-35.0, y0=-9.0, step_x=15.0, step_y=2.0, ranges=_R4,
                            ego_tail=True, pad_to=4),
    "8x8-aligned": GridSpec(layers=("presence", "heading", "on_road"), nx=8, ny=8, x0=-35.0,
                            y0=-7.0, step_x=10.0, step_y=2.0, align=True, ego_tail=False, pad_to=4),
    "5x13-odd": GridSpec(layers=("vx", "on_road", "y"), nx=5, ny=13, x0=-22.5, y0=-13.0, step_x=15.0,
                         step_y=2.0, ranges={"vx": (-30.0, 30.0)}, clip=False, ego_tail=True, pad_to=1),
    "32x32": GridSpec(layers=("presence", "vx"), nx=32, ny=32, x0=-63.0, y0=-16.5, step_x=6.0,
                      step_y=1.0, ego_tail=True, pad_to=4),
    "default": GridSpec(),
    "default-aligned": GridSpec(align=True),
    "8layers-aligned": GridSpec(layers=("on_road", "presence", "x", "y", "vx", "vy", "heading", "sin_h"),
                                nx=9, ny=7, x0=-31.5, y0=-10.5, step_x=9.0, step_y=3.0, ranges=_R4,
                                align=True, ego_tail=True, pad_to=4),
}
# (E, vehicles_count, lanes_count, spec): E in {1, 3, 5, 37} (partial blocks), every vehicles_count
# of {0, 1, 20, 63}, every lanes_count of {1, 4, 8}, every spec
NATURAL = [(1, 0, 1, "1x1"), (1, 63, 4, "5x13-odd"), (3, 1, 4, "8x8-aligned"), (3, 20, 8, "32x32"),
           (5, 20, 8, "7x9-8layers"), (5, 63, 1, "default-aligned"), (37, 63, 4, "default"),
           (37, 20, 4, "8layers-aligned"), (5, 0, 4, "7x9-8layers"), (37, 1, 8, "1x1"),
           (3, 63, 8, "8layers-aligned"), (5, 20, 4, "5x13-odd")]


def drive(hip, steps, seed=5, steer=0.3):
    rng = np.random.default_rng(seed)
    hip.reset()
    for t in range(steps):
        a = np.tanh(rng.normal(size=(hip.E, 2)) * np.array([0.6, steer])).astype(np.float32)
        hip.step(a)


@pytest.mark.parametrize("E, vc, lanes, name", NATURAL)
def test_kernel_against_model_on_natural_states(E, vc, lanes, name):
    spec = SPECS[name]
    cfg = make_cfg(E=E, vehicles_count=vc, lanes_count=lanes, max_episode_steps=30)
    hip = HipEnv(cfg)
    try:
        pairs = undecided = inside = 0
        hip.reset()
        rng = np.random.default_rng(E + vc)
        for t in range(7):
            if t:
                hip.step(np.tanh(rng.normal(size=(E, 2)) * np.array([0.6, 0.3])).astype(np.float32))
            if t % 3 == 0:
                p, u, _ = check_against_model(hip, spec, f"{name} E{E} V{vc} L{lanes} step {t}")
                pairs, undecided = pairs + p, undecided + u
        # the last state once more with the ego moved into the traffic, where the grid fills up
        natural = hip.state()
        hip.set_state(gc.ego_into_traffic(cfg, natural, rng))
        p, u, inside = check_against_model(hip, spec, f"{name} E{E} V{vc} L{lanes} in traffic")
        pairs, undecided = pairs + p, undecided + u
        print(f"{name} E{E} V{vc} L{lanes}: {undecided} of {pairs} pairs undecided, {inside} "
              f"others inside the grid in traffic")
        assert pairs >= 4 * E and undecided <= 0.01 * pairs
        assert inside >= (E if vc >= 20 else 1 if vc else 0)
    finally:
        hip.close()


def test_the_shapes_cover_what_the_kernel_branches_on():
    assert {s.nx * s.ny for s in SPECS.values()} >= {1, 63, 64, 65, 1024}
    assert {len(s.layers) for s in SPECS.values()} >= {1, 8}
    assert any("on_road" in s.layers and len(s.layers) == 8 for s in SPECS.values())
    assert {s.ego_tail for s in SPECS.values()} == {True, False}
    assert {n[0] for n in NATURAL} == {1, 3, 5, 37} and {n[1] for n in NATURAL} == {0, 1, 20, 63}
    assert {n[2] for n in NATURAL} == {1, 4, 8} and {n[3] for n in NATURAL} == set(SPECS)


# ------------------------------------------------------------------- 3. padding and bounds
@pytest.mark.parametrize("extra", [0, 3])
def test_a_width_that_is_no_multiple_of_four(extra):
    spec = SPECS["5x13-odd"]
    cfg = make_cfg(E=5, vehicles_count=20, max_episode_steps=30)
    width = spec.width(cfg.n_features)
    assert width == 199 and width % 4
    hip = HipEnv(cfg)
    try:
        drive(hip, 4)
        check_against_model(hip, spec, f"row_stride = width + {extra}", stride=width + extra)
    finally:
        hip.close()


def test_every_combination_of_outputs():
    spec = SPECS["7x9-8layers"]
    hip = HipEnv(make_cfg(E=3, vehicles_count=20))
    try:
        drive(hip, 3)
        full = grid_call(hip, spec)
        n = 0
        for mask in range(1, 16):
            names = tuple(k for i, k in enumerate(OUTPUTS) if mask >> i & 1)
            part = grid_call(hip, spec, outputs=names)
            assert set(part) == set(names)
            assert all(np.array_equal(part[k].view(np.uint32), full[k].view(np.uint32)) for k in part)
            n += 1
        assert n == 15
    finally:
        hip.close()


# ------------------------------------------------------------------- 4. against hwy_observe
def observe_rows(hip):
    from hwy.native import check, lib

    obs = torch.zeros(hip.E, hip.N, hip.Fo, device=DEV)
    rv = torch.zeros(hip.E, hip.N, dtype=torch.int32, device=DEV)
    a = _abi.ObserveArgs(-1, obs.data_ptr(), rv.data_ptr(), None, None)
    check(lib().hwy_observe(hip.h, ctypes.byref(a), None), "hwy_observe")
    torch.cuda.synchronize()
    return obs.cpu().numpy(), rv.cpu().numpy()


def test_grid_values_are_the_observations_own_bits():
    """no model: with the handle's own ranges, the grid's x, y, vx, vy of a vehicle that won its
    cell are the bits of the Kinematics row that shows it; the ego tail is row 0"""
    cfg = make_cfg(E=16, N=30, max_episode_steps=30)   # x, y, vx, vy; absolute off
    assert not cfg.absolute and cfg.normalize and cfg.clip
    names = [n for f in range(cfg.n_features) for n, i in _abi.FEATURES.items()
             if i == cfg.feature_ids[f]]
    assert names == ["x", "y", "vx", "vy"]
    ranges = {n: (cfg.features_range[f][0], cfg.features_range[f][1]) for f, n in enumerate(names)}
    spec = GridSpec(layers=names, ranges=ranges, clip=True, nx=24, ny=5, pad_to=4)
    hip = HipEnv(cfg)
    kind, d = _abi.PE_RANK, 8
    wrapped = HipEnv(make_cfg(E=16, N=30, max_episode_steps=30, pe=kind, d=d),
                     pe_table_for(kind, d, 30))
    try:
        drive(hip, 6)
        hip.set_state(gc.ego_into_traffic(cfg, hip.state(), np.random.default_rng(1), heading=0))
        obs, rv = observe_rows(hip)
        got = grid_call(hip, spec)
        n, ncells, F = 0, spec.nx * spec.ny, cfg.n_features
        layers = got["grid"][:, :4 * ncells].reshape(16, 4, ncells).view(np.uint32)
        for e in range(16):
            for r in range(1, 30):
                k = rv[e, r]
                c = got["veh_cell"][e, k] if k >= 1 else -1
                if c >= 0 and got["cell_vehicle"][e, c] == k:
                    assert np.array_equal(layers[e, :, c], obs[e, r].view(np.uint32)), (e, r, k)
                    n += 1
        assert n >= 16 * 3, n   # rows compared: a few vehicles per env won a cell
        tail = got["grid"][:, 4 * ncells:4 * ncells + F].view(np.uint32)
        assert np.array_equal(tail, obs[:, 0].view(np.uint32)), "the ego tail is not row 0"
        # a handle with a fused wrapper holding the same state: the same tail, before any wrapper
        wrapped.reset()
        wrapped.set_state(hip.state())
        assert wrapped.Fo == F + d
        wtail = grid_call(wrapped, spec)["grid"][:, 4 * ncells:4 * ncells + F].view(np.uint32)
        assert np.array_equal(wtail, tail)
    finally:
        hip.close()
        wrapped.close()


# ------------------------------------------------------------------- 5. it follows the state
def test_grid_follows_reset_autoreset_and_cut():
    spec = SPECS["default"]
    cfg = make_cfg(E=6, max_episode_steps=3)
    hip = HipEnv(cfg)
    try:
        hip.reset()
        check_against_model(hip, spec, "after reset")
        first = grid_call(hip, spec, outputs=("grid",))["grid"]
        rng = np.random.default_rng(2)
        resets = 0
        for t in range(4):
            out = hip.step(policy_actions(rng, 6, t))
            resets += int((out[2] | out[3]).sum())
            check_against_model(hip, spec, f"after step {t}")
            done = (out[2] | out[3]) != 0   # autoreset: the grid shows the new episode
            assert (hip.state()[_abi.F_ENV][done, _abi.E_STEP] == 0).all()
        again = grid_call(hip, spec, outputs=("grid",))["grid"]
        assert not np.array_equal(again, first)   # new seeds: other traffic
        assert resets >= 6
        hip.cut_episodes()
        check_against_model(hip, spec, "after cut_episodes")
        hip.reset(9000 + np.arange(6), (np.arange(6) % 2).astype(np.uint8))
        check_against_model(hip, spec, "after a masked seeded reset")
    finally:
        hip.close()


# ------------------------------------------------------------------- 6. capture
def _vec(E, autoreset=False, **kw):
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(kw)
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=autoreset)


def test_captured_grid_replays_on_the_later_state():
    from utils.graphs import capture

    env = _vec(5)
    spec = SPECS["7x9-8layers"]
    try:
        env.reset(seed=3)
        E, F = 5, 4
        kw = dict(out=torch.zeros(E, spec.stride(F), device=DEV),
                  cell_vehicle=torch.zeros(E, spec.nx, spec.ny, dtype=torch.int32, device=DEV),
                  veh_cell=torch.zeros(E, 64, dtype=torch.int32, device=DEV),
                  counts=torch.zeros(E, 4, dtype=torch.int32, device=DEV))
        env.grid_into(spec, **kw)  # eager first: the code object loads outside the capture
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                env.grid_into(spec, **kw)
        torch.cuda.current_stream().wait_stream(s)
        first = {k: t.clone() for k, t in kw.items()}
        for _ in range(3):
            env.step(torch.full((E, 2), 0.3, device=DEV))
        for t in kw.values():
            t.fill_(-7)
        g.replay()
        torch.cuda.synchronize()
        eager = {k: torch.full_like(t, -9) for k, t in kw.items()}
        env.grid_into(spec, **eager)
        torch.cuda.synchronize()
        for k in kw:
            assert torch.equal(kw[k].view(torch.int32), eager[k].view(torch.int32)), k
        assert not torch.equal(kw["out"], first["out"])
    finally:
        env.close()


# ------------------------------------------------------------------- 7. the refusals
def test_each_refusal_leaves_the_outputs_untouched():
    from hwy.native import HWY_EINVAL

    cfg = make_cfg(E=3, vehicles_count=5)
    spec = GridSpec()
    hip = HipEnv(cfg)
    I32x8, F32x2x8 = ctypes.c_int32 * 8, (ctypes.c_float * 2) * 8
    nan, inf = float("nan"), float("inf")
    try:
        hip.reset()
        before = hip.state()
        for word, kw in (
                ("nx and ny", dict(nx=0)), ("nx and ny", dict(ny=-3)), ("nx and ny", dict(nx=33, ny=32)),
                ("x0 and y0", dict(x0=nan)), ("x0 and y0", dict(y0=inf)),
                ("step_x and step_y", dict(step_x=0.0)), ("step_x and step_y", dict(step_y=nan)),
                ("step_x and step_y", dict(step_x=inf)),
                ("n_layers", dict(n_layers=0)), ("n_layers", dict(n_layers=9)),
                ("layer_ids[1]", dict(layer_ids=I32x8(0, 9, 4))), ("layer_ids[0]", dict(layer_ids=I32x8(-1, 3, 4))),
                ("given twice", dict(layer_ids=I32x8(0, 3, 3))),
                ("range[1]", dict(range=F32x2x8((0, 0), (5.0, 5.0), (-80.0, 80.0)))),
                ("range[2]", dict(range=F32x2x8((0, 0), (-80.0, 80.0), (nan, 80.0)))),
                ("row_stride", dict(row_stride=360)), ("row_stride", dict(row_stride=4097)),
                # the handle's four features: the width is 364
                ("below the width", dict(row_stride=363))):
            msg = grid_call(hip, spec, stride=368, expect=HWY_EINVAL, **kw)
            assert word in msg, (word, msg)
        msg = grid_call(hip, spec, outputs=(), expect=HWY_EINVAL)
        assert "no output" in msg
        assert np.array_equal(before, hip.state())
        grid_call(hip, spec, stride=364)   # the width itself is taken
    finally:
        hip.close()


# ------------------------------------------------------------------- 8. the Python surface
def test_python_surface_and_the_one_env_facade():
    from hwy.single_env import HighwayEnv

    env = _vec(4, autoreset=True)
    spec = GridSpec()
    try:
        env.reset(seed=11)
        env.step(torch.full((4, 2), 0.1, device=DEV))
        g = env.grid(spec)
        assert g.shape == (4, 364) and g.dtype == torch.float32
        assert torch.equal(g, env.grid(True)) and torch.equal(g, env.grid(spec.to_dict()))
        buf = torch.empty(4 * 364, device=DEV)
        assert env.grid(spec, out=buf).data_ptr() == buf.data_ptr()
        cells = env.grid_cells(spec)
        assert cells.shape == (4, 24, 5) and cells.dtype == torch.int32
        assert (cells[:, 6, 2] == 0).all()   # the ego: (0 + 32.5) / 5 = 6.5, (0 + 10) / 4 = 2.5
        assert torch.equal(g[:, :120].reshape(4, 24, 5) != 0, cells >= 0)   # the presence layer
        st = env.export_state().cpu().numpy().view(np.uint32)
        m = gm.grid_model(env.hwy_config, st, spec)
        vc = torch.zeros(4, 64, dtype=torch.int32, device=DEV)
        cn = torch.zeros(4, 4, dtype=torch.int32, device=DEV)
        env.grid_into(spec, veh_cell=vc, counts=cn)
        gm.compare(m, dict(grid=g.cpu().numpy(), cell_vehicle=cells.cpu().numpy(),
                           veh_cell=vc.cpu().numpy(), counts=cn.cpu().numpy()))
        with pytest.raises(ValueError, match="^out must be"):
            env.grid_into(spec, out=torch.zeros(4, 368, device=DEV))
        with pytest.raises(ValueError, match="^counts must be"):
            env.grid_into(spec, counts=torch.zeros(4, 4, device=DEV))
        with pytest.raises(ValueError, match="at least one"):
            env.grid_into(spec)
        with pytest.raises(ValueError, match="unknown grid keys"):
            env.grid({"cells": 3})
    finally:
        env.close()
    one = HighwayEnv(HIGHWAY_CONFIG)
    try:
        one.reset(seed=5)
        one.step(np.array([0.1, 0.0], np.float32))
        row = one.grid(spec)
        assert isinstance(row, np.ndarray) and row.shape == (364,) and row.dtype == np.float32
        st = one.vec_env.export_state().cpu().numpy().view(np.uint32)
        gm.compare(gm.grid_model(one.vec_env.hwy_config, st, spec), dict(grid=row[None]))
    finally:
        one.close()
