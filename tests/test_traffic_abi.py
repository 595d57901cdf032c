"""hwy_traffic's ABI without a device: the struct layout, every refusal that needs no handle
(hwy_traffic_check, and hwy_traffic's own NULL checks) and the Python layer's argument checks."""

from __future__ import annotations

import ctypes

import pytest
import torch

from hwy import _abi
from hwy.native import HWY_EINVAL, HWY_OK, last_error, lib
from hwy.vec_env import TRAFFIC_OUTPUTS, alloc_traffic, traffic_args

OUTS = _abi.TRAFFIC_VEHICLE_OUTPUTS + ("ego", "acc")
INF, NAN = float("inf"), float("nan")


def test_struct_layout():
    assert lib().hwy_traffic_args_size() == ctypes.sizeof(_abi.TrafficArgs) == 120
    a = _abi.TrafficArgs
    assert [getattr(a, n).offset for n, _ in a._fields_] == \
        [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 80, 104, 108, 112, 116]
    assert [n for n, _ in a._fields_][:10] == list(TRAFFIC_OUTPUTS)


def args(restart=(), thresholds=(2.0, 1.0, 4.0, 50.0), **ptrs):
    a = _abi.TrafficArgs()
    for k, v in ptrs.items():
        setattr(a, k, v)
    for k, v in enumerate(restart):
        a.restart[k] = v
    a.ttc_thresh, a.thw_thresh, a.risk_horizon, a.near_range = thresholds
    return a


@pytest.mark.parametrize("kw", [{k: 16} for k in OUTS] + [
    dict(acc=16, ep_stats=32), dict(acc=16, restart=(48,)), dict(acc=16, restart=(48, 64, 80)),
    dict(acc=16, ep_stats=32, restart=(None, None, 80)), {k: 16 * (i + 1) for i, k in enumerate(OUTS)},
    dict(ego=16, thresholds=(1e-30, 1e30, 0.5, 3e38))])
def test_check_accepts(kw):
    assert lib().hwy_traffic_check(ctypes.byref(args(**kw))) == HWY_OK


@pytest.mark.parametrize("kw, word", [
    (dict(), "no output"), (dict(ep_stats=16), "no output"), (dict(restart=(16,)), "no output"),
    (dict(ego=16, ep_stats=32), "ep_stats needs acc"),
    (dict(ego=16, restart=(32,)), "restart[0] needs acc"),
    (dict(gap=16, restart=(None, None, 32)), "restart[2] needs acc"),
] + [(dict(ego=16, thresholds=tuple(bad if i == k else 1.0 for i in range(4))), name)
     for k, name in enumerate(("ttc_thresh", "thw_thresh", "risk_horizon", "near_range"))
     for bad in (0.0, -1.0, INF, -INF, NAN)])
def test_check_refuses(kw, word):
    assert lib().hwy_traffic_check(ctypes.byref(args(**kw))) == HWY_EINVAL
    assert word in last_error()


def test_null_args_and_null_handle():
    assert lib().hwy_traffic_check(None) == HWY_EINVAL and "args is NULL" in last_error()
    assert lib().hwy_traffic(None, ctypes.byref(args(ego=16)), None) == HWY_EINVAL
    assert "handle is NULL" in last_error()


E = 3
CPU = torch.device("cpu")


def test_alloc_traffic_shapes_and_python_args_fill_the_struct():
    t = alloc_traffic(E, CPU)
    assert tuple(t) == TRAFFIC_OUTPUTS
    assert {k: (tuple(v.shape), v.dtype) for k, v in t.items()} == dict(
        {k: ((E, 64), torch.int32) for k in ("front", "rear")},
        **{k: ((E, 64), torch.float32) for k in ("gap", "closing", "ttc", "thw", "risk")},
        ego=((E, 16), torch.float32), acc=((E, 8), torch.float32), ep_stats=((E, 8), torch.float32))
    assert not t["acc"].any()
    masks = [torch.zeros(E, dtype=torch.uint8) for _ in range(3)]
    a = traffic_args(E, CPU, restart=masks, near_range=30.0, **t)
    assert [getattr(a, k) for k in t] == [v.data_ptr() for v in t.values()]
    assert list(a.restart) == [m.data_ptr() for m in masks]
    assert (a.ttc_thresh, a.thw_thresh, a.risk_horizon, a.near_range) == (2.0, 1.0, 4.0, 30.0)
    assert lib().hwy_traffic_check(ctypes.byref(a)) == HWY_OK
    a = traffic_args(E, CPU, restart=(None, masks[1]), ego=t["ego"], acc=t["acc"], gap=None)
    assert (a.gap, a.front, a.ep_stats) == (None, None, None)
    assert list(a.restart) == [masks[1].data_ptr(), None, None]


@pytest.mark.parametrize("name, bad", [
    ("front", lambda: torch.zeros(E, 64)),
    ("rear", lambda: torch.zeros(E, 64, dtype=torch.int64)),
    ("gap", lambda: torch.zeros(E, 63)),
    ("closing", lambda: torch.zeros(E, 64, dtype=torch.float64)),
    ("ttc", lambda: torch.zeros(64, E).t()),
    ("thw", lambda: torch.zeros(E, 64).numpy()),
    ("risk", lambda: torch.zeros(E, 64, device="meta")),
    ("ego", lambda: torch.zeros(E, 8)),
    ("acc", lambda: torch.zeros(E, 16)),
    ("ep_stats", lambda: torch.zeros(E + 1, 8)),
])
def test_python_args_refuse_a_wrong_tensor(name, bad):
    t = alloc_traffic(E, CPU)
    t[name] = bad()
    with pytest.raises(ValueError, match=f"^{name} must be"):
        traffic_args(E, CPU, **t)


def test_python_args_refuse_combinations_masks_and_thresholds():
    t = alloc_traffic(E, CPU)
    m = torch.zeros(E, dtype=torch.uint8)
    with pytest.raises(ValueError, match="at least one output"):
        traffic_args(E, CPU)
    with pytest.raises(ValueError, match="at least one output"):
        traffic_args(E, CPU, ep_stats=t["ep_stats"], gap=None)
    with pytest.raises(ValueError, match="ep_stats needs acc"):
        traffic_args(E, CPU, ego=t["ego"], ep_stats=t["ep_stats"])
    with pytest.raises(ValueError, match="restart masks need acc"):
        traffic_args(E, CPU, ego=t["ego"], restart=(m,))
    with pytest.raises(ValueError, match="at most three"):
        traffic_args(E, CPU, acc=t["acc"], restart=(m, m, m, m))
    with pytest.raises(ValueError, match=r"^restart\[1\] must be"):
        traffic_args(E, CPU, acc=t["acc"], restart=(m, torch.zeros(E, dtype=torch.bool)))
    with pytest.raises(ValueError, match=r"^restart\[0\] must be"):
        traffic_args(E, CPU, acc=t["acc"], restart=(torch.zeros(E + 1, dtype=torch.uint8),))
    with pytest.raises(ValueError, match="unknown traffic outputs"):
        traffic_args(E, CPU, ego=t["ego"], headway=t["thw"])
    for name in _abi.TRAFFIC_DEFAULTS:
        for bad in (0.0, -2.0, INF, NAN, 1e39):
            with pytest.raises(ValueError, match=f"^{name} must be finite"):
                traffic_args(E, CPU, ego=t["ego"], **{name: bad})


# ------------------------------------------------------------------- the booking (training/routine.py)
def test_safety_row_near_miss_rate_and_the_files_null():
    import json

    import numpy as np

    from training import routine

    row = np.array([4, 1.5, 0.25, 3.0, 6.5, 1, 3, 4], np.float32)
    assert routine.safety_row(row) == (1.5, 0.25, 3.0, 6.5, 0.25, 0.75)
    never = np.array([7, INF, INF, INF, 40.0, 0, 0, 0], np.float32)
    assert routine.safety_row(never) == (INF, INF, INF, 40.0, 0.0, 0.0)
    assert routine.safety_row(np.zeros(8, np.float32))[4:] == (0.0, 0.0)
    assert routine.SAFETY_KEYS == ("episode_min_ttc", "episode_min_headway", "episode_min_gap",
                                   "episode_min_distance", "episode_ttc_critical_share",
                                   "episode_tailgating_share")
    assert routine.near_miss_rate([]) == 0.0
    assert routine.near_miss_rate([1.0, INF, 1.99, 2.0]) == 0.5
    assert routine.near_miss_rate([1.0] * 50 + [INF] * 100) == 0.0      # the last 100
    assert routine.near_miss_rate([3.0, 5.0], ttc_thresh=4.0) == 0.5
    mh = {"episode_rewards": [1.0, 2.0], "episode_min_ttc": [INF, 1.5], "episode_min_gap": [2.0, INF]}
    out = json.loads(json.dumps(routine._json_ready(mh)))
    assert out == {"episode_rewards": [1.0, 2.0], "episode_min_ttc": [None, 1.5],
                   "episode_min_gap": [2.0, None]}
    assert mh["episode_min_ttc"][0] == INF                   # the dict in memory keeps its floats
    plain = {"episode_rewards": [1.0]}
    assert routine._json_ready(plain) is plain               # without the option: the dict itself


def test_safety_stream_order():
    import numpy as np

    from training.routine import _safety_stream

    T, n = 3, 4
    stats = torch.arange(T * n * 8, dtype=torch.float32).view(T, n, 8)
    dones = torch.tensor([[0, 1, 0, 0], [0, 0, 0, 1], [1, 0, 0, 0]], dtype=torch.uint8)
    rows = _safety_stream(dones, stats)
    assert [int(r[0]) // 8 for r in rows] == [1, 7, 8]       # (step, env) order
    cut = torch.tensor([0, 1, 1, 0], dtype=torch.uint8)
    rows = _safety_stream(dones, stats, cut)
    assert [int(r[0]) // 8 for r in rows] == [1, 7, 8, 9, 10]  # then the cut envs, from row T - 1
    assert isinstance(rows, np.ndarray) and rows.shape == (5, 8)
