"""hwy_sense's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_sense_check, and hwy_sense's own NULL checks), the accepted edges, SensorModel and the
Python layer's argument checks."""

from __future__ import annotations

import ctypes
import json
import math

import pytest
import torch

from hwy import SensorModel, _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import sense_args

INF, NAN = math.inf, math.nan


def test_struct_layout():
    assert lib().hwy_sense_args_size() == ctypes.sizeof(_abi.SenseArgs) == 72
    a = _abi.SenseArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == [0, 4, 8, 12, 16, 28, 32, 40, 48, 56, 64]
    assert _abi.HWY_SENSE_SALT == 0x53454E53 != 0x53485546


def args(order=-1, los=0, range_m=INF, p_drop=0.0, sigma=(0.0, 0.0, 0.0), salt=0, obs=None,
         row_vehicle=None, visible=None, hidden=None, counts=None):
    return _abi.SenseArgs(order, los, range_m, p_drop, (ctypes.c_float * 3)(*sigma), salt, obs,
                          row_vehicle, visible, hidden, counts)


@pytest.mark.parametrize("kw", [
    dict(obs=16), dict(row_vehicle=16), dict(visible=16), dict(hidden=16), dict(counts=16),
    dict(obs=16, order=0), dict(obs=16, order=1, los=1), dict(obs=16, los=7),
    dict(obs=16, range_m=INF), dict(obs=16, range_m=1e-30), dict(obs=16, range_m=3e38),
    dict(obs=16, p_drop=0.0), dict(obs=16, p_drop=1.0), dict(obs=16, p_drop=-0.0),
    dict(obs=16, salt=65535), dict(obs=16, sigma=(0.0, 3e38, -0.0)),
    dict(obs=16, row_vehicle=32, visible=48, hidden=64, counts=80, los=1, range_m=50.0,
         p_drop=0.5, sigma=(1.0, 2.0, 3.0), salt=1),
])
def test_check_accepts(kw):
    assert lib().hwy_sense_check(ctypes.byref(args(**kw))) == HWY_OK, last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(obs=16, order=2), "order"), (dict(obs=16, order=-2), "order"),
    (dict(obs=16, range_m=0.0), "range_m"), (dict(obs=16, range_m=-1.0), "range_m"),
    (dict(obs=16, range_m=-INF), "range_m"), (dict(obs=16, range_m=NAN), "range_m"),
    (dict(obs=16, p_drop=-1e-9), "p_drop"), (dict(obs=16, p_drop=1.0000001), "p_drop"),
    (dict(obs=16, p_drop=NAN), "p_drop"), (dict(obs=16, p_drop=INF), "p_drop"),
    (dict(obs=16, sigma=(-1e-9, 0.0, 0.0)), "sigma[0]"), (dict(obs=16, sigma=(0.0, INF, 0.0)), "sigma[1]"),
    (dict(obs=16, sigma=(0.0, 0.0, NAN)), "sigma[2]"),
    (dict(obs=16, salt=-1), "salt"), (dict(obs=16, salt=65536), "salt"),
    (dict(), "no output"), (dict(los=1, range_m=10.0), "no output"),
])
def test_check_refuses(kw, word):
    assert lib().hwy_sense_check(ctypes.byref(args(**kw))) == HWY_EINVAL
    assert word in last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_sense_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_sense(None, ctypes.byref(args(obs=16)), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


# ------------------------------------------------------------------------------ SensorModel
def test_sensor_model_defaults_and_value_semantics():
    s = SensorModel()
    assert (s.los, s.range, s.dropout, s.noise, s.salt) == (False, None, 0.0, (0.0, 0.0, 0.0), 0)
    assert s.is_null and not SensorModel(los=True).is_null and not SensorModel(range=5).is_null
    assert SensorModel(salt=3).is_null
    assert SensorModel(range=INF) == s and hash(SensorModel(noise=[0, 0, 0])) == hash(s)
    assert SensorModel(los=True) != s and len({s, SensorModel(), SensorModel(dropout=0.1)}) == 2
    with pytest.raises(AttributeError):
        s.los = True


def test_sensor_model_round_trips_through_json():
    s = SensorModel(los=True, range=80.0, dropout=0.25, noise=(0.5, 0.25, 1.0), salt=11)
    d = json.loads(json.dumps(s.to_dict()))
    assert SensorModel.from_dict(d) == s and SensorModel.from_dict(s) is s
    assert json.loads(json.dumps(SensorModel().to_dict()))["range"] is None
    assert SensorModel.from_dict({}) == SensorModel()
    assert SensorModel.from_dict({"los": True}) == SensorModel(los=True)


@pytest.mark.parametrize("kw", [
    dict(range=0), dict(range=-3.0), dict(range=NAN), dict(range=-INF), dict(range="far"),
    dict(dropout=-0.1), dict(dropout=1.5), dict(dropout=NAN), dict(dropout=None),
    dict(noise=(0, 0)), dict(noise=(0, 0, 0, 0)), dict(noise=(-1, 0, 0)), dict(noise=(0, INF, 0)),
    dict(noise=(0, 0, NAN)), dict(noise=1.0),
    dict(salt=-1), dict(salt=65536), dict(salt=1.5), dict(salt="a"),
])
def test_sensor_model_refuses_what_the_check_refuses(kw):
    with pytest.raises(ValueError):
        SensorModel(**kw)


def test_from_dict_refuses_unknown_keys_and_other_types():
    with pytest.raises(ValueError, match="unknown sensor keys"):
        SensorModel.from_dict({"los": True, "fog": 1})
    with pytest.raises(ValueError, match="a sensor is"):
        SensorModel.from_dict("los")
    with pytest.raises(ValueError, match="a sensor is"):
        SensorModel.from_dict(None)


def test_fill_passes_the_check():
    for s in (SensorModel(), SensorModel(los=True, range=80.0, dropout=1.0, noise=(1, 2, 3), salt=65535)):
        a = s.fill(_abi.SenseArgs())
        a.order, a.obs = -1, 16
        assert lib().hwy_sense_check(ctypes.byref(a)) == HWY_OK
        assert a.range_m == (INF if s.range is None else s.range) and a.salt == s.salt
        assert (a.los, a.p_drop, tuple(a.sigma)) == (int(s.los), s.dropout, s.noise)


# ------------------------------------------------------------------------------ sense_args
E, N, FO = 3, 5, 6
CPU = torch.device("cpu")


def good():
    return dict(obs=torch.zeros(E, N, FO), row_vehicle=torch.zeros(E, N, dtype=torch.int32),
                visible=torch.zeros(E, 64, dtype=torch.uint8), hidden=torch.zeros(E, 64),
                counts=torch.zeros(E, 4, dtype=torch.int32))


def test_python_args_accept_and_fill_the_struct():
    t = good()
    a = sense_args(E, N, FO, CPU, SensorModel(los=True, salt=4), "shuffled", **t)
    assert (a.order, a.los, a.salt) == (1, 1, 4)
    assert [getattr(a, k) for k in t] == [v.data_ptr() for v in t.values()]
    a = sense_args(E, N, FO, CPU, {"range": 50}, None, counts=t["counts"])
    assert (a.order, a.obs, a.visible, a.range_m) == (-1, None, None, 50.0)
    assert lib().hwy_sense_check(ctypes.byref(a)) == HWY_OK


@pytest.mark.parametrize("name, bad", [
    ("obs", lambda: torch.zeros(E, N, FO + 1)),
    ("obs", lambda: torch.zeros(E, N, FO, dtype=torch.float64)),
    ("obs", lambda: torch.zeros(E, FO, N).transpose(1, 2)),
    ("obs", lambda: torch.zeros(E, N, FO, device="meta")),
    ("row_vehicle", lambda: torch.zeros(E, N, dtype=torch.int64)),
    ("visible", lambda: torch.zeros(E, 64, dtype=torch.bool)),
    ("visible", lambda: torch.zeros(E, 63, dtype=torch.uint8)),
    ("hidden", lambda: torch.zeros(E, 64, dtype=torch.float16)),
    ("hidden", lambda: torch.zeros(E, 65)),
    ("counts", lambda: torch.zeros(E, 3, dtype=torch.int32)),
    ("counts", lambda: torch.zeros(E, 4)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = good()
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        sense_args(E, N, FO, CPU, SensorModel(), None, **t)


def test_python_args_refuse_no_output_bad_orders_and_bad_sensors():
    t = good()
    with pytest.raises(ValueError, match="at least one"):
        sense_args(E, N, FO, CPU, SensorModel())
    with pytest.raises(ValueError, match="order must be"):
        sense_args(E, N, FO, CPU, SensorModel(), "reversed", obs=t["obs"])
    with pytest.raises(ValueError, match="dropout"):
        sense_args(E, N, FO, CPU, {"dropout": 2}, obs=t["obs"])
    with pytest.raises(ValueError, match="a sensor is"):
        sense_args(E, N, FO, CPU, None, obs=t["obs"])
