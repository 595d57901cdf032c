"""hwy_lookahead's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_lookahead_check, and hwy_lookahead's own NULL check), the accepted edges, hwy.Shield and the
Python layer's argument checks."""

from __future__ import annotations

import ctypes
import json
import math

import pytest
import torch

from hwy import Shield, _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import lookahead_args

INF, NAN = math.inf, math.nan


def test_struct_layout():
    assert lib().hwy_lookahead_args_size() == ctypes.sizeof(_abi.LookaheadArgs) == 104
    a = _abi.LookaheadArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == \
        [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72, 80, 88, 96]
    assert [n for n, _ in a._fields_][6:] == list(_abi.LOOKAHEAD_OUTPUTS)
    assert (_abi.LOOKAHEAD_MAX_K, _abi.LOOKAHEAD_MAX_H, _abi.LOOKAHEAD_MAX_BRANCHES) == (64, 64, 1 << 22)


def args(k=2, horizon=3, hold=0, lazy=0, gamma=1.0, actions=16, **out):
    a = _abi.LookaheadArgs()
    a.k, a.horizon, a.hold, a.lazy, a.gamma, a.actions = k, horizon, hold, lazy, gamma, actions
    for n, v in out.items():
        assert n in _abi.LOOKAHEAD_OUTPUTS
        setattr(a, n, v)
    return a


@pytest.mark.parametrize("kw", [
    *[{n: 32} for n in _abi.LOOKAHEAD_OUTPUTS[:7]],
    dict(steps=32, k=1, horizon=1), dict(steps=32, k=64, horizon=64),
    dict(ret=32, gamma=0.0), dict(ret=32, gamma=-0.0), dict(ret=32, gamma=1.0), dict(ret=32, gamma=0.9),
    dict(steps=32, terminated=48, lazy=1), dict(steps=32, terminated=48, lazy=5, hold=3),
    dict(steps=32, terminated=48, chosen=64),
    dict(steps=32, terminated=48, chosen=64, chosen_action=80, lazy=1, hold=1),
    dict(steps=32, terminated=48, truncated=64, rewards=80, ret=96, ego_final=112, obs=128,
         chosen=144, chosen_action=160),
])
def test_check_accepts(kw):
    assert lib().hwy_lookahead_check(ctypes.byref(args(**kw))) == HWY_OK, last_error()


@pytest.mark.parametrize("kw, word", [
    (dict(steps=32, k=0), "k must"), (dict(steps=32, k=65), "k must"), (dict(steps=32, k=-1), "k must"),
    (dict(steps=32, horizon=0), "horizon"), (dict(steps=32, horizon=65), "horizon"),
    (dict(ret=32, gamma=-1e-9), "gamma"), (dict(ret=32, gamma=1.0000001), "gamma"),
    (dict(ret=32, gamma=NAN), "gamma"), (dict(ret=32, gamma=INF), "gamma"),
    (dict(ret=32, gamma=-INF), "gamma"),
    (dict(steps=32, actions=None), "actions is NULL"),
    (dict(), "no output"), (dict(hold=1), "no output"),
    (dict(lazy=1, steps=32), "lazy and chosen need"), (dict(lazy=1, terminated=32), "lazy and chosen need"),
    (dict(lazy=1, ret=32), "lazy and chosen need"),
    (dict(chosen=32), "lazy and chosen need"), (dict(chosen=32, steps=48), "lazy and chosen need"),
    (dict(chosen=32, terminated=48), "lazy and chosen need"),
    (dict(chosen_action=32, steps=48, terminated=64), "chosen_action needs chosen"),
    (dict(chosen_action=32), "chosen_action needs chosen"),
])
def test_check_refuses(kw, word):
    assert lib().hwy_lookahead_check(ctypes.byref(args(**kw))) == HWY_EINVAL
    assert word in last_error(), last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_lookahead_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_lookahead(None, ctypes.byref(args(steps=32)), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


# ------------------------------------------------------------------------------ Shield
def test_shield_defaults_and_value_semantics():
    s = Shield()
    assert (s.horizon, s.fallbacks, s.lazy) == (3, ((-1.0, 0.0), (0.0, 0.0), (1.0, 0.0)), True)
    assert s.k == 4
    assert Shield(fallbacks=[[-1, 0], [0, 0], [1, 0]]) == s
    assert hash(Shield(3, [(-1, 0), (0, 0), (1, 0)], 1)) == hash(s)
    assert Shield(horizon=4) != s and Shield(lazy=False) != s
    assert len({s, Shield(), Shield(horizon=2)}) == 2
    with pytest.raises(AttributeError):
        s.horizon = 5
    assert Shield(horizon=64, fallbacks=[(0.5, 0.5)] * 63).k == 64


def test_shield_round_trips_through_json():
    s = Shield(horizon=5, fallbacks=((-1.0, 0.25), (0.5, -0.5)), lazy=False)
    d = json.loads(json.dumps(s.to_dict()))
    assert Shield.from_dict(d) == s and Shield.from_dict(s) is s
    assert Shield.from_dict({}) == Shield() and Shield.from_dict({"horizon": 2}) == Shield(horizon=2)


@pytest.mark.parametrize("kw", [
    dict(horizon=0), dict(horizon=65), dict(horizon=-1), dict(horizon=2.5), dict(horizon="3"),
    dict(horizon=None), dict(fallbacks=()), dict(fallbacks=[(0.0, 0.0)] * 64),
    dict(fallbacks=[(NAN, 0.0)]), dict(fallbacks=[(0.0, INF)]), dict(fallbacks=[(0.0, -INF)]),
    dict(fallbacks=[(0.0,)]), dict(fallbacks=[(0.0, 0.0, 0.0)]), dict(fallbacks=1.0),
    dict(fallbacks=[("a", 0)]),
])
def test_shield_refuses(kw):
    with pytest.raises(ValueError):
        Shield(**kw)


def test_shield_from_dict_refuses_unknown_keys_and_other_types():
    with pytest.raises(ValueError, match="unknown shield keys"):
        Shield.from_dict({"horizon": 3, "depth": 1})
    for bad in ("shield", None, 3):
        with pytest.raises(ValueError, match="a shield is"):
            Shield.from_dict(bad)


# ------------------------------------------------------------------------------ lookahead_args
E, K, H, N, FO = 3, 4, 5, 5, 6
CPU = torch.device("cpu")


def good():
    return dict(steps=torch.zeros(E, K, dtype=torch.int32),
                terminated=torch.zeros(E, K, dtype=torch.uint8),
                truncated=torch.zeros(E, K, dtype=torch.uint8), rewards=torch.zeros(E, K, H),
                ret=torch.zeros(E, K), ego_final=torch.zeros(E, K, 4),
                obs=torch.zeros(E, K, N, FO), chosen=torch.zeros(E, dtype=torch.int32),
                chosen_action=torch.zeros(E, 2))


def test_python_args_accept_and_fill_the_struct():
    t, acts = good(), torch.zeros(E, K, H, 2)
    a = lookahead_args(E, N, FO, CPU, acts, H, gamma=0.5, lazy=True, **t)
    assert (a.k, a.horizon, a.hold, a.lazy, a.gamma, a.actions) == (K, H, 0, 1, 0.5, acts.data_ptr())
    assert [getattr(a, k) for k in t] == [v.data_ptr() for v in t.values()]
    assert lib().hwy_lookahead_check(ctypes.byref(a)) == HWY_OK
    held = torch.zeros(E, K, 2)
    a = lookahead_args(E, N, FO, CPU, held, 64, hold=True, ret=t["ret"])
    assert (a.k, a.horizon, a.hold, a.lazy, a.steps, a.obs) == (K, 64, 1, 0, None, None)
    assert lib().hwy_lookahead_check(ctypes.byref(a)) == HWY_OK


@pytest.mark.parametrize("name, bad", [
    ("steps", lambda: torch.zeros(E, K, dtype=torch.int64)),
    ("steps", lambda: torch.zeros(E, K + 1, dtype=torch.int32)),
    ("terminated", lambda: torch.zeros(E, K, dtype=torch.bool)),
    ("truncated", lambda: torch.zeros(E, K)),
    ("rewards", lambda: torch.zeros(E, K, H - 1)),
    ("rewards", lambda: torch.zeros(E, H, K).transpose(1, 2)),
    ("ret", lambda: torch.zeros(E, K, dtype=torch.float64)),
    ("ego_final", lambda: torch.zeros(E, K, 3)),
    ("obs", lambda: torch.zeros(E, K, N, FO + 1)),
    ("obs", lambda: torch.zeros(E, K, N, FO, device="meta")),
    ("chosen", lambda: torch.zeros(E, 2, dtype=torch.int32)),
    ("chosen_action", lambda: torch.zeros(E, 3)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = good()
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        lookahead_args(E, N, FO, CPU, torch.zeros(E, K, H, 2), H, **t)


@pytest.mark.parametrize("acts, kw", [
    (lambda: torch.zeros(E, K, H, 3), {}), (lambda: torch.zeros(E + 1, K, H, 2), {}),
    (lambda: torch.zeros(E, K, H + 1, 2), {}), (lambda: torch.zeros(E, K, 2), {}),
    (lambda: torch.zeros(E, K, H, 2), dict(hold=True)), (lambda: torch.zeros(E, 0, H, 2), {}),
    (lambda: torch.zeros(E, 65, H, 2), {}), (lambda: torch.zeros(E, K, H, 2, dtype=torch.float64), {}),
    (lambda: torch.zeros(E, K, 2, H).transpose(2, 3), {}), (lambda: [[0.0, 0.0]], {}),
])
def test_python_args_refuse_wrong_actions(acts, kw):
    with pytest.raises(ValueError, match="^actions must be|K must lie"):
        lookahead_args(E, N, FO, CPU, acts(), H, ret=torch.zeros(E, K), **kw)


def test_python_args_refuse_what_the_check_refuses():
    t, acts = good(), torch.zeros(E, K, H, 2)
    with pytest.raises(ValueError, match="at least one"):
        lookahead_args(E, N, FO, CPU, acts, H)
    for h in (0, 65, 2.5, None):
        with pytest.raises(ValueError, match="horizon"):
            lookahead_args(E, N, FO, CPU, torch.zeros(E, K, 2), h, hold=True, ret=t["ret"])
    for g in (-0.1, 1.1, NAN, INF, "x"):
        with pytest.raises(ValueError, match="gamma"):
            lookahead_args(E, N, FO, CPU, acts, H, gamma=g, ret=t["ret"])
    with pytest.raises(ValueError, match="lazy and chosen need"):
        lookahead_args(E, N, FO, CPU, acts, H, lazy=True, steps=t["steps"])
    with pytest.raises(ValueError, match="lazy and chosen need"):
        lookahead_args(E, N, FO, CPU, acts, H, chosen=t["chosen"], terminated=t["terminated"])
    with pytest.raises(ValueError, match="chosen_action needs chosen"):
        lookahead_args(E, N, FO, CPU, acts, H, chosen_action=t["chosen_action"], steps=t["steps"],
                       terminated=t["terminated"])
    # E * K over 2^22 (no tensor of that size is needed: the actions' shape is read first)
    big = torch.zeros(1 << 17, 64, 2, device="meta")
    with pytest.raises(ValueError, match="E \\* K"):
        lookahead_args(1 << 17, N, FO, torch.device("meta"), big, 1, hold=True,
                       ret=torch.zeros(1, device="meta"))
