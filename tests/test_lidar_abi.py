"""hwy_lidar's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_lidar_check, and hwy_lidar's own NULL checks), LidarSpec, the Python layer's argument checks
and the run option's record."""

from __future__ import annotations

import copy
import ctypes
import json
import math

import pytest
import torch

import hwy
from config.base_config import HIGHWAY_CONFIG
from hwy import LidarSpec, _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import lidar_args
from ppo import options
from ppo.rollout import check_lidar

INF, NAN = math.inf, math.nan


def test_symbols_and_struct_layout():
    for name in ("hwy_lidar_args_size", "hwy_lidar_check", "hwy_lidar"):
        assert hasattr(lib(), name)
    assert lib().hwy_lidar_args_size() == ctypes.sizeof(_abi.LidarArgs) == 80
    a = _abi.LidarArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == [
        0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48, 56, 64, 72]
    assert _abi.HWY_LIDAR_SALT == 0x4C494441 == int.from_bytes(b"LIDA", "big")
    assert _abi.LIDAR_OUTPUTS == ("obs", "hit_vehicle", "seen", "counts")


def default_args(F=5, **kw):
    """the default spec's hwy_lidar_args with `obs` given, then `kw` written over it"""
    a = LidarSpec().fill(_abi.LidarArgs(), F)
    a.obs = 16
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_check_accepts_the_default_and_the_edges():
    a = default_args()
    assert lib().hwy_lidar_check(ctypes.byref(a)) == HWY_OK, last_error()
    assert (a.cells, a.sub, a.range_m, a.align, a.normalize, a.speed_scale) == (16, 1, 60.0, 0, 1, 60.0)
    assert (a.p_drop, a.sigma_r, a.salt, a.ego_tail, a.row_stride) == (0.0, 0.0, 0, 1, 40)
    for kw in (dict(obs=None, counts=16), dict(obs=None, seen=16), dict(obs=None, hit_vehicle=16),
               dict(cells=1, row_stride=3), dict(cells=1024, row_stride=2049),
               dict(cells=1024, sub=4, row_stride=4096), dict(cells=256, sub=16, row_stride=600),
               dict(cells=1, sub=16), dict(row_stride=33), dict(ego_tail=0, row_stride=32),
               dict(range_m=1e-30), dict(range_m=3e38, speed_scale=1e-30), dict(p_drop=1.0),
               dict(sigma_r=3e38), dict(salt=65535)):
        assert lib().hwy_lidar_check(ctypes.byref(default_args(**kw))) == HWY_OK, (kw, last_error())


@pytest.mark.parametrize("kw, word", [
    (dict(obs=None), "no output"),
    (dict(cells=0), "cells must"), (dict(cells=-1), "cells must"), (dict(cells=1025), "cells must"),
    (dict(sub=0), "sub must"), (dict(sub=17), "sub must"), (dict(sub=-1), "sub must"),
    (dict(cells=1024, sub=5, row_stride=4096), "cells * sub"),
    (dict(cells=257, sub=16, row_stride=4096), "cells * sub"),
    (dict(range_m=0.0), "range_m and speed_scale"), (dict(range_m=-1.0), "range_m and speed_scale"),
    (dict(range_m=INF), "range_m and speed_scale"), (dict(range_m=NAN), "range_m and speed_scale"),
    (dict(speed_scale=0.0), "range_m and speed_scale"),
    (dict(speed_scale=INF), "range_m and speed_scale"),
    (dict(speed_scale=NAN), "range_m and speed_scale"),
    (dict(p_drop=-0.1), "p_drop"), (dict(p_drop=1.5), "p_drop"), (dict(p_drop=NAN), "p_drop"),
    (dict(sigma_r=-1.0), "sigma_r"), (dict(sigma_r=INF), "sigma_r"), (dict(sigma_r=NAN), "sigma_r"),
    (dict(salt=-1), "salt"), (dict(salt=65536), "salt"),
    (dict(row_stride=32), "row_stride"), (dict(ego_tail=0, row_stride=31), "row_stride"),
    (dict(row_stride=4097), "row_stride"), (dict(row_stride=-4), "row_stride"),
])
def test_check_refuses(kw, word):
    assert lib().hwy_lidar_check(ctypes.byref(default_args(**kw))) == HWY_EINVAL, kw
    assert word in last_error(), last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_lidar_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_lidar(None, ctypes.byref(default_args()), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


# ------------------------------------------------------------------------------ LidarSpec
def test_default_spec_and_value_semantics():
    g = LidarSpec()
    assert (g.cells, g.sub, g.range_m, g.speed_scale) == (16, 1, 60.0, 60.0)
    assert g.normalize and g.ego_tail and not g.align and g.pad_to == 4
    assert (g.p_drop, g.sigma_r, g.salt) == (0.0, 0.0, 0)
    assert g.shape == (16, 2)
    assert (g.width(5), g.stride(5)) == (37, 40)     # a five-feature row
    assert (g.width(4), g.stride(4)) == (36, 36)     # the shipped x, y, vx, vy row
    assert LidarSpec(ego_tail=False).width(5) == LidarSpec(ego_tail=False).stride(5) == 32
    assert LidarSpec(pad_to=1).stride(5) == 37 and LidarSpec(pad_to=64).stride(5) == 64
    assert LidarSpec(range_m=80).speed_scale == 80.0 and LidarSpec(speed_scale=25).speed_scale == 25.0
    assert hash(g) == hash(LidarSpec()) and g == LidarSpec(cells=16.0)
    assert len({g, LidarSpec(), LidarSpec(align=True), LidarSpec(cells=17)}) == 3
    assert hwy.LidarSpec is LidarSpec
    with pytest.raises(AttributeError):
        g.cells = 3
    assert LidarSpec(cells=1024, pad_to=4096).stride(5) == 4096
    with pytest.raises(ValueError, match="above hwy_lidar's"):
        LidarSpec(cells=1024, pad_to=4097).stride(5)


def test_spec_round_trips_through_json_and_from_dict():
    g = LidarSpec(cells=63, sub=3, range_m=45.5, align=True, normalize=False, speed_scale=30.0,
                  p_drop=0.25, sigma_r=0.125, salt=77, ego_tail=False, pad_to=8)
    d = json.loads(json.dumps(g.to_dict()))
    assert LidarSpec.from_dict(d) == g and LidarSpec.from_dict(g) is g
    assert LidarSpec.from_dict({}) == LidarSpec.from_dict(True) == LidarSpec()
    with pytest.raises(ValueError, match="unknown lidar keys"):
        LidarSpec.from_dict({"cells": 3, "nx": 4})
    for bad in (None, "lidar", False, 3):
        with pytest.raises(ValueError, match="a lidar is"):
            LidarSpec.from_dict(bad)


@pytest.mark.parametrize("kw", [
    dict(cells=0), dict(cells=1025), dict(cells=2.5), dict(cells="a"), dict(sub=0), dict(sub=17),
    dict(sub=1.5), dict(cells=1024, sub=5), dict(range_m=0), dict(range_m=-1.0), dict(range_m=INF),
    dict(range_m=NAN), dict(speed_scale=0), dict(speed_scale=INF), dict(p_drop=-0.1),
    dict(p_drop=1.5), dict(p_drop=NAN), dict(sigma_r=-1), dict(sigma_r=INF), dict(sigma_r=NAN),
    dict(salt=-1), dict(salt=65536), dict(salt=1.5), dict(pad_to=0), dict(pad_to=1.5),
])
def test_spec_refuses_what_the_check_refuses(kw):
    with pytest.raises(ValueError):
        LidarSpec(**kw)


def test_from_observation_config():
    g = LidarSpec.from_observation_config({"type": "LidarObservation"})
    assert g == LidarSpec() and (g.cells, g.range_m, g.normalize) == (16, 60.0, True)
    g = LidarSpec.from_observation_config({"cells": 64, "maximum_range": 80, "normalize": False},
                                          ego_tail=False, pad_to=8, sub=2, align=True)
    assert (g.cells, g.range_m, g.normalize, g.speed_scale) == (64, 80.0, False, 80.0)
    assert (g.sub, g.align, g.ego_tail, g.pad_to) == (2, True, False, 8)
    for bad, word in (({"vehicles_count": 5}, "unknown LidarObservation keys"),
                      ({"type": "Kinematics"}, "not a LidarObservation"),
                      ({"cells": 0}, "cells must"), ({"maximum_range": -1}, "range_m")):
        with pytest.raises(ValueError, match=word):
            LidarSpec.from_observation_config(bad)


def test_the_env_config_still_refuses_the_lidar_type():
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg["observation"]["type"] = "LidarObservation"
    with pytest.raises(ValueError, match=r"observation type 'LidarObservation' is not supported \(Kinematics only\)"):
        _abi.config_from_dict(cfg)


# ------------------------------------------------------------------------------ lidar_args
E, F = 3, 5
CPU = torch.device("cpu")


def good(spec=LidarSpec()):
    return dict(out=torch.zeros(E, spec.stride(F)),
                hit_vehicle=torch.zeros(E, spec.cells, dtype=torch.int32),
                seen=torch.zeros(E, 64),
                counts=torch.zeros(E, 4, dtype=torch.int32))


def test_python_args_accept_and_fill_the_struct():
    t = good()
    a = lidar_args(E, F, CPU, LidarSpec(), **t)
    assert [a.obs, a.hit_vehicle, a.seen, a.counts] == [v.data_ptr() for v in t.values()]
    assert lib().hwy_lidar_check(ctypes.byref(a)) == HWY_OK
    a = lidar_args(E, F, CPU, True, counts=t["counts"])
    assert (a.obs, a.hit_vehicle, a.seen) == (None, None, None) and a.row_stride == 40
    a = lidar_args(E, 4, CPU, {"align": True, "cells": 63}, out=torch.zeros(E, 132))
    assert (a.align, a.cells, a.row_stride) == (1, 63, 132)
    assert lib().hwy_lidar_check(ctypes.byref(a)) == HWY_OK


@pytest.mark.parametrize("name, bad", [
    ("out", lambda: torch.zeros(E, 37)),
    ("out", lambda: torch.zeros(E, 40, dtype=torch.float64)),
    ("out", lambda: torch.zeros(40, E).t()),
    ("out", lambda: torch.zeros(E, 40, device="meta")),
    ("hit_vehicle", lambda: torch.zeros(E, 16, dtype=torch.int64)),
    ("hit_vehicle", lambda: torch.zeros(E, 15, dtype=torch.int32)),
    ("seen", lambda: torch.zeros(E, 63)),
    ("seen", lambda: torch.zeros(E, 64, dtype=torch.int32)),
    ("counts", lambda: torch.zeros(E, 3, dtype=torch.int32)),
    ("counts", lambda: torch.zeros(E, 4, dtype=torch.uint8)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = good()
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        lidar_args(E, F, CPU, LidarSpec(), **t)


def test_python_args_refuse_no_output_and_bad_specs():
    with pytest.raises(ValueError, match="at least one"):
        lidar_args(E, F, CPU, LidarSpec())
    with pytest.raises(ValueError, match="unknown lidar keys"):
        lidar_args(E, F, CPU, {"nx": 3}, out=torch.zeros(E, 40))
    with pytest.raises(ValueError, match="a lidar is"):
        lidar_args(E, F, CPU, None, out=torch.zeros(E, 40))


# ------------------------------------------------------------------------------ the run option
def test_the_option_record():
    opt = options.BY_NAME["lidar"]
    assert options.OPTIONS[-1] is opt
    assert opt.rollout and opt.group == "launch" and opt.metrics == "value" and not opt.grouped
    assert [n for n, _ in opt.excludes] == ["grid", "sensor", "shield", "truncation",
                                            "episode_schedule"]
    assert opt.excludes_late == options.BY_NAME["grid"].excludes_late
    for order in (options.ROUTINE_ORDER, options.LAUNCH_ORDER, options.GROUPED_ORDER):
        assert order[-1] == "lidar" and len(set(order)) == len(order) == len(options.OPTIONS)
    assert not opt.given(None) and not opt.given(False) and opt.given(True) and opt.given({})
    assert opt.normalise(True) == LidarSpec() and opt.normalise(None) is None
    assert opt.normalise({"cells": 8}) == LidarSpec(cells=8)
    assert options.initial_metrics({"lidar": LidarSpec(cells=8)}) == {
        "lidar": LidarSpec(cells=8).to_dict()}


@pytest.mark.parametrize("others, word", [
    (dict(grid=True), "lidar does not go with grid"),
    (dict(sensor={"range": 80.0}), "lidar does not go with sensor"),
    (dict(shield={"horizon": 4}), "lidar does not go with shield"),
    (dict(truncation="bootstrap"), 'lidar does not go with truncation="bootstrap"'),
    (dict(episode_schedule="reference"), 'lidar does not go with episode_schedule="reference"'),
])
def test_the_option_refuses_what_it_excludes(others, word):
    kw = dict(truncation="terminal", episode_schedule="lockstep", sensor=None, shield=None,
              grid=None)
    kw.update(others)
    with pytest.raises(ValueError, match=word):
        check_lidar(True, **kw)
    assert check_lidar(None, **kw) is None  # not given: nothing to refuse
    assert check_lidar(True) == LidarSpec()


def _values(**kw):
    v = {o.name: o.default for o in options.OPTIONS}
    v.update(kw)
    return v


def test_check_run_refuses_for_the_lidar():
    ok = options.check_run(_values(lidar={"cells": 8}), lambda: True, False)
    assert ok["lidar"] == LidarSpec(cells=8) and ok["grid"] is None
    with pytest.raises(ValueError, match="lidar needs a HighwayVecEnv"):
        options.check_run(_values(lidar=True), lambda: False, False)
    with pytest.raises(ValueError, match="lidar does not run over a process group"):
        options.check_run(_values(lidar=True), lambda: True, True)
    with pytest.raises(ValueError, match="lidar does not go with grid"):
        options.check_run(_values(lidar=True, grid=True), lambda: True, False)
    for late in (dict(attribution=True), dict(eval_orders=["sorted"]),
                 dict(eval_sensors={"s": {"range": 80.0}}), dict(eval_shields={"none": None})):
        with pytest.raises(ValueError, match="lidar does not go with attribution, eval_orders"):
            options.check_run(_values(lidar=True, **late), lambda: True, False)
    # a run without the option is checked as before
    assert options.check_run(_values(), lambda: False, False)["lidar"] is None
