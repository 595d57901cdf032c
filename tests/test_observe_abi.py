"""hwy_observe's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_observe_check, and hwy_observe's own NULL checks) and the Python layer's argument checks."""

from __future__ import annotations

import ctypes

import pytest
import torch

from hwy import _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import observe_args


def test_struct_layout():
    assert lib().hwy_observe_args_size() == ctypes.sizeof(_abi.ObserveArgs) == 40
    a = _abi.ObserveArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == [0, 8, 16, 24, 32]


def args(order=-1, obs=None, row_vehicle=None, row_values=None, veh_values=None):
    return _abi.ObserveArgs(order, obs, row_vehicle, row_values, veh_values)


@pytest.mark.parametrize("kw", [dict(obs=16), dict(row_vehicle=16), dict(obs=16, order=0),
                                dict(row_values=16, veh_values=32, order=1),
                                dict(obs=16, row_vehicle=32, row_values=48, veh_values=64)])
def test_check_accepts(kw):
    assert lib().hwy_observe_check(ctypes.byref(args(**kw))) == HWY_OK


@pytest.mark.parametrize("kw, word", [
    (dict(obs=16, order=2), "order"), (dict(obs=16, order=-2), "order"),
    (dict(obs=16, order=1 << 20), "order"),
    (dict(), "all NULL"), (dict(order=0), "all NULL"),
    (dict(row_values=16), "all NULL"),
    (dict(obs=16, row_values=16), "go together"),
    (dict(obs=16, veh_values=16), "go together"),
    (dict(veh_values=16), "go together"),
])
def test_check_refuses(kw, word):
    assert lib().hwy_observe_check(ctypes.byref(args(**kw))) == HWY_EINVAL
    assert word in last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_observe_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_observe(None, ctypes.byref(args(obs=16)), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


def test_order_names():
    assert [_abi.observe_order(o) for o in (None, "sorted", "shuffled")] == [-1, 0, 1]
    assert (_abi.ORDER_SORTED, _abi.ORDER_SHUFFLED) == (0, 1)
    for bad in ("Sorted", "", 0, 1, -1, ["sorted"], b"sorted"):
        with pytest.raises(ValueError, match="order must be"):
            _abi.observe_order(bad)


E, N, FO = 3, 5, 6
CPU = torch.device("cpu")


def good():
    return dict(obs=torch.zeros(E, N, FO), row_vehicle=torch.zeros(E, N, dtype=torch.int32),
                row_values=torch.zeros(E, N), veh_values=torch.zeros(E, 64))


def test_python_args_accepts_and_fills_the_struct():
    t = good()
    a = observe_args(E, N, FO, CPU, "shuffled", **t)
    assert a.order == 1
    assert [getattr(a, k) for k in t] == [v.data_ptr() for v in t.values()]
    a = observe_args(E, N, FO, CPU, None, row_vehicle=t["row_vehicle"])
    assert (a.order, a.obs, a.row_values, a.veh_values) == (-1, None, None, None)
    assert lib().hwy_observe_check(ctypes.byref(a)) == HWY_OK


@pytest.mark.parametrize("name, bad", [
    ("obs", lambda: torch.zeros(E, N, FO + 1)),
    ("obs", lambda: torch.zeros(E, N, FO, dtype=torch.float64)),
    ("obs", lambda: torch.zeros(E, FO, N).transpose(1, 2)),
    ("obs", lambda: torch.zeros(E, N, FO).numpy()),
    ("obs", lambda: torch.zeros(E, N, FO, device="meta")),
    ("row_vehicle", lambda: torch.zeros(E, N, dtype=torch.int64)),
    ("row_vehicle", lambda: torch.zeros(E, N + 1, dtype=torch.int32)),
    ("row_values", lambda: torch.zeros(E, N, dtype=torch.float16)),
    ("row_values", lambda: torch.zeros(E * N + 1)),
    ("veh_values", lambda: torch.zeros(E, 63)),
    ("veh_values", lambda: torch.zeros(E, 64, dtype=torch.int32)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = good()
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        observe_args(E, N, FO, CPU, None, **t)


def test_python_args_refuse_combinations_and_orders():
    t = good()
    with pytest.raises(ValueError, match="at least one"):
        observe_args(E, N, FO, CPU)
    with pytest.raises(ValueError, match="at least one"):
        observe_args(E, N, FO, CPU, row_values=None)
    with pytest.raises(ValueError, match="go together"):
        observe_args(E, N, FO, CPU, obs=t["obs"], row_values=t["row_values"])
    with pytest.raises(ValueError, match="go together"):
        observe_args(E, N, FO, CPU, veh_values=t["veh_values"])
    with pytest.raises(ValueError, match="order must be"):
        observe_args(E, N, FO, CPU, "reversed", obs=t["obs"])
