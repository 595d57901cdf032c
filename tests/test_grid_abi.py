"""hwy_grid's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_grid_check, and hwy_grid's own NULL checks), GridSpec and the Python layer's argument
checks."""

from __future__ import annotations

import copy
import ctypes
import json
import math

import pytest
import torch

import hwy
from config.base_config import HIGHWAY_CONFIG
from hwy import GridSpec, _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import grid_args

INF, NAN = math.inf, math.nan


def test_symbols_and_struct_layout():
    for name in ("hwy_grid_args_size", "hwy_grid_check", "hwy_grid"):
        assert hasattr(lib(), name)
    assert lib().hwy_grid_args_size() == ctypes.sizeof(_abi.GridArgs) == 208
    a = _abi.GridArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == [
        0, 4, 8, 12, 16, 20, 24, 28, 32, 64, 96, 160, 164, 168, 176, 184, 192, 200]
    assert _abi.GRID_ON_ROAD == 8 and _abi.GRID_LAYERS["on_road"] == 8
    assert {k: v for k, v in _abi.GRID_LAYERS.items() if k != "on_road"} == _abi.FEATURES


def default_args(F=5, **kw):
    """the default spec's hwy_grid_args with `grid` given, then `kw` written over it"""
    a = GridSpec().fill(_abi.GridArgs(), F)
    a.grid = 16
    for k, v in kw.items():
        if k in ("layer_ids", "has_range"):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        elif k == "range":
            for i, (lo, hi) in enumerate(v):
                a.range[i][0], a.range[i][1] = lo, hi
        else:
            setattr(a, k, v)
    return a


def test_check_accepts_the_default_and_the_edges():
    a = default_args()
    assert lib().hwy_grid_check(ctypes.byref(a)) == HWY_OK, last_error()
    assert (a.nx, a.ny, a.n_layers, a.row_stride, a.clip, a.ego_tail, a.align) == (24, 5, 3, 368, 1, 1, 0)
    assert list(a.layer_ids)[:3] == [0, 3, 4] and list(a.has_range)[:3] == [0, 1, 1]
    for kw in (dict(grid=None, counts=16), dict(grid=None, veh_cell=16), dict(grid=None, cell_vehicle=16),
               dict(nx=32, ny=32, n_layers=1, row_stride=4096), dict(nx=1024, ny=1, n_layers=1, row_stride=1030),
               dict(nx=1, ny=1, row_stride=4), dict(row_stride=361), dict(ego_tail=0, row_stride=360),
               dict(n_layers=8, nx=4, ny=4, layer_ids=[8, 7, 6, 5, 4, 3, 2, 1], has_range=[0] * 8,
                    row_stride=129),
               dict(x0=-3e38, y0=3e38, step_x=1e-30, step_y=3e38),
               dict(has_range=[0, 0, 0], range=[(NAN, NAN), (1.0, 1.0), (INF, 0.0)])):
        assert lib().hwy_grid_check(ctypes.byref(default_args(**kw))) == HWY_OK, (kw, last_error())


@pytest.mark.parametrize("kw, word", [
    (dict(grid=None), "no output"),
    (dict(nx=0), "nx and ny"), (dict(ny=0), "nx and ny"), (dict(nx=-1), "nx and ny"),
    (dict(nx=1025, ny=1, n_layers=1), "nx and ny"), (dict(nx=33, ny=32, n_layers=1), "nx and ny"),
    (dict(nx=65536, ny=65536), "nx and ny"),
    (dict(x0=NAN), "x0 and y0"), (dict(x0=INF), "x0 and y0"), (dict(y0=-INF), "x0 and y0"),
    (dict(step_x=0.0), "step_x and step_y"), (dict(step_x=-1.0), "step_x and step_y"),
    (dict(step_y=INF), "step_x and step_y"), (dict(step_y=NAN), "step_x and step_y"),
    (dict(n_layers=0), "n_layers"), (dict(n_layers=9), "n_layers"), (dict(n_layers=-1), "n_layers"),
    (dict(layer_ids=[0, 9]), "layer_ids[1]"), (dict(layer_ids=[-1]), "layer_ids[0]"),
    (dict(layer_ids=[0, 3, 0]), "given twice"), (dict(layer_ids=[8, 8]), "given twice"),
    (dict(range=[(0.0, 0.0), (2.0, 2.0)]), "range[1]"), (dict(range=[(0.0, 0.0), (-80.0, INF)]), "range[1]"),
    (dict(range=[(0.0, 0.0), (-80.0, 80.0), (NAN, 80.0)]), "range[2]"),
    (dict(row_stride=360), "row_stride"), (dict(ego_tail=0, row_stride=359), "row_stride"),
    (dict(row_stride=4097), "row_stride"), (dict(row_stride=-4), "row_stride"),
])
def test_check_refuses(kw, word):
    assert lib().hwy_grid_check(ctypes.byref(default_args(**kw))) == HWY_EINVAL, kw
    assert word in last_error(), last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_grid_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_grid(None, ctypes.byref(default_args()), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


# ------------------------------------------------------------------------------ GridSpec
def test_default_spec_and_value_semantics():
    g = GridSpec()
    assert g.layers == ("presence", "vx", "vy") and (g.nx, g.ny) == (24, 5)
    assert (g.x0, g.y0, g.step_x, g.step_y) == (-32.5, -10.0, 5.0, 4.0)
    assert dict(g.ranges) == {"vx": (-80.0, 80.0), "vy": (-80.0, 80.0)}
    assert g.clip and g.ego_tail and not g.align and g.pad_to == 4
    assert g.shape == (3, 24, 5)
    assert (g.width(5), g.stride(5)) == (365, 368)     # a five-feature row
    assert (g.width(4), g.stride(4)) == (364, 364)     # the shipped x, y, vx, vy row
    assert GridSpec(ego_tail=False).width(5) == GridSpec(ego_tail=False).stride(5) == 360
    assert GridSpec(pad_to=1).stride(5) == 365 and GridSpec(pad_to=64).stride(5) == 384
    assert hash(g) == hash(GridSpec()) and g == GridSpec(layers=["presence", "vx", "vy"])
    assert len({g, GridSpec(), GridSpec(align=True), GridSpec(nx=23)}) == 3
    assert hwy.GridSpec is GridSpec
    with pytest.raises(AttributeError):
        g.nx = 3
    with pytest.raises(ValueError, match="above hwy_grid's"):
        GridSpec(layers=("presence", "x", "y", "vx", "vy"), nx=32, ny=32).stride(5)


def test_spec_round_trips_through_json_and_from_dict():
    g = GridSpec(layers=("presence", "on_road", "x"), nx=7, ny=9, x0=-1.5, y0=2.0, step_x=0.5,
                 step_y=3.0, ranges={"x": (-10, 30)}, clip=False, align=True, ego_tail=False, pad_to=8)
    d = json.loads(json.dumps(g.to_dict()))
    assert GridSpec.from_dict(d) == g and GridSpec.from_dict(g) is g
    assert GridSpec.from_dict({}) == GridSpec.from_dict(True) == GridSpec()
    with pytest.raises(ValueError, match="unknown grid keys"):
        GridSpec.from_dict({"nx": 3, "cells": 4})
    for bad in (None, "grid", False, 3):
        with pytest.raises(ValueError, match="a grid is"):
            GridSpec.from_dict(bad)


@pytest.mark.parametrize("kw", [
    dict(layers=()), dict(layers=("presence", "speed")), dict(layers=("vx", "vx")), dict(layers="vx"),
    dict(layers=("presence", "x", "y", "vx", "vy", "cos_h", "sin_h", "heading", "on_road")),
    dict(nx=0), dict(ny=-1), dict(nx=2.5), dict(nx=33, ny=32), dict(nx="a"),
    dict(x0=NAN), dict(y0=INF), dict(step_x=0), dict(step_y=-1.0), dict(step_x=INF),
    dict(ranges={"vx": (1.0, 1.0)}), dict(ranges={"vx": (0.0, INF)}), dict(ranges={"x": (0.0, 1.0)}),
    dict(layers=("presence", "on_road"), ranges={"on_road": (0.0, 1.0)}), dict(ranges={"vx": 3}),
    dict(pad_to=0), dict(pad_to=1.5),
])
def test_spec_refuses_what_the_check_refuses(kw):
    with pytest.raises(ValueError):
        GridSpec(**kw)


def test_from_observation_config():
    # upstream's default: [-27.5, 27.5]^2 at step 5 -> 11 x 11
    g = GridSpec.from_observation_config({"type": "OccupancyGrid"})
    assert (g.nx, g.ny, g.x0, g.y0, g.step_x, g.step_y) == (11, 11, -27.5, -27.5, 5.0, 5.0)
    assert g.layers == ("presence", "vx", "vy") and g.clip and not g.align and g.ego_tail
    assert dict(g.ranges) == {"vx": (-80.0, 80.0), "vy": (-80.0, 80.0)}
    # a size whose quotient is no integer: floor(55 / 4) = 13, floor(21 / 2.5) = 8
    g = GridSpec.from_observation_config({
        "features": ["presence", "x", "on_road"], "grid_size": [[-20, 35], [-10.5, 10.5]],
        "grid_step": [4, 2.5], "features_range": {"x": [-50, 50], "vx": [-20, 20]},
        "align_to_vehicle_axes": True, "clip": False}, ego_tail=False, pad_to=8)
    assert (g.nx, g.ny, g.x0, g.y0, g.step_x, g.step_y) == (13, 8, -20.0, -10.5, 4.0, 2.5)
    assert g.layers == ("presence", "x", "on_road") and dict(g.ranges) == {"x": (-50.0, 50.0)}
    assert g.align and not g.clip and not g.ego_tail and g.pad_to == 8
    # the cell count is floor in float64, as upstream takes it: 0.3 / 0.1 = 2.9999999999999996
    g = GridSpec.from_observation_config({"grid_size": [[0, 0.3], [0, 1]], "grid_step": [0.1, 0.5]})
    assert (g.nx, g.ny) == (2, 2)
    # the default spec is this project's road-ahead grid in upstream's keys
    assert GridSpec.from_observation_config({"grid_size": [[-32.5, 87.5], [-10, 10]],
                                             "grid_step": [5, 4]}) == GridSpec()
    for bad, word in (({"absolute": True}, "absolute"), ({"as_image": True}, "as_image"),
                      ({"vehicles_count": 5}, "unknown OccupancyGrid keys"),
                      ({"type": "Kinematics"}, "not an OccupancyGrid"),
                      ({"grid_step": [0, 5]}, "grid_step"), ({"grid_size": [[0, 1]]}, "grid_size"),
                      ({"features": ["presence", "speed"]}, "unknown grid layer")):
        with pytest.raises(ValueError, match=word):
            GridSpec.from_observation_config(bad)


def test_the_env_config_still_refuses_the_occupancy_grid_type():
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["type"] = "OccupancyGrid"
    with pytest.raises(ValueError, match=r"observation type 'OccupancyGrid' is not supported \(Kinematics only\)"):
        _abi.config_from_dict(cfg)


# ------------------------------------------------------------------------------ grid_args
E, F = 3, 5
CPU = torch.device("cpu")


def good(spec=GridSpec()):
    return dict(out=torch.zeros(E, spec.stride(F)),
                cell_vehicle=torch.zeros(E, spec.nx, spec.ny, dtype=torch.int32),
                veh_cell=torch.zeros(E, 64, dtype=torch.int32),
                counts=torch.zeros(E, 4, dtype=torch.int32))


def test_python_args_accept_and_fill_the_struct():
    t = good()
    a = grid_args(E, F, CPU, GridSpec(), **t)
    assert [a.grid, a.cell_vehicle, a.veh_cell, a.counts] == [v.data_ptr() for v in t.values()]
    assert lib().hwy_grid_check(ctypes.byref(a)) == HWY_OK
    a = grid_args(E, F, CPU, True, counts=t["counts"])
    assert (a.grid, a.cell_vehicle, a.veh_cell) == (None, None, None) and a.row_stride == 368
    a = grid_args(E, 4, CPU, {"align": True}, out=torch.zeros(E, 364))
    assert (a.align, a.row_stride) == (1, 364)
    assert lib().hwy_grid_check(ctypes.byref(a)) == HWY_OK


@pytest.mark.parametrize("name, bad", [
    ("out", lambda: torch.zeros(E, 365)),
    ("out", lambda: torch.zeros(E, 368, dtype=torch.float64)),
    ("out", lambda: torch.zeros(368, E).t()),
    ("out", lambda: torch.zeros(E, 368, device="meta")),
    ("cell_vehicle", lambda: torch.zeros(E, 24, 5, dtype=torch.int64)),
    ("cell_vehicle", lambda: torch.zeros(E, 24, 4, dtype=torch.int32)),
    ("veh_cell", lambda: torch.zeros(E, 63, dtype=torch.int32)),
    ("veh_cell", lambda: torch.zeros(E, 64)),
    ("counts", lambda: torch.zeros(E, 3, dtype=torch.int32)),
    ("counts", lambda: torch.zeros(E, 4, dtype=torch.uint8)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = good()
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        grid_args(E, F, CPU, GridSpec(), **t)


def test_python_args_refuse_no_output_and_bad_specs():
    with pytest.raises(ValueError, match="at least one"):
        grid_args(E, F, CPU, GridSpec())
    with pytest.raises(ValueError, match="unknown grid keys"):
        grid_args(E, F, CPU, {"cells": 3}, out=torch.zeros(E, 368))
    with pytest.raises(ValueError, match="a grid is"):
        grid_args(E, F, CPU, None, out=torch.zeros(E, 368))
