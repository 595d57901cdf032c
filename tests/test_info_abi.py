"""hwy_step_with_info / hwy_step_group_info (include/hwy.h) without a GPU: the symbols exist, the
ctypes mirror agrees with the library on hwy_step_info's layout, arguments the calls must refuse
are refused before any device call, and a sweep batch's cells must agree on episode_stats."""

import ctypes

import pytest

from hwy import _abi
from hwy.native import LIB_PATH, HwyStepGroupPlan, HwyStepIO

NEW = ("hwy_step_info_size", "hwy_step_with_info", "hwy_step_group_info_table_bytes",
       "hwy_step_group_info_prepare", "hwy_step_group_info")
FAKE = 4096  # a non-NULL address that no refused call may touch


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB_PATH)
    L.hwy_last_error.restype = ctypes.c_char_p
    return L


def test_info_symbols_and_struct_layout(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.hwy_step_info_size() == ctypes.sizeof(_abi.HwyStepInfo) == 6 * ctypes.sizeof(
        ctypes.c_void_p)
    assert [n for n, _ in _abi.HwyStepInfo._fields_] == ["speed", "crashed", "lane", "rewards",
                                                         "acc", "ep_stats"]
    assert _abi.HWY_INFO_NACC == 8
    # the config's layout is untouched (no field added for the info outputs)
    assert lib.hwy_config_size() == ctypes.sizeof(_abi.HwyConfig)
    assert lib.hwy_abi_version() == _abi.HWY_ABI_VERSION == 1


def test_step_with_info_refuses_bad_arguments_before_any_device_call(lib):
    vp = ctypes.c_void_p
    f = lib.hwy_step_with_info
    f.restype = ctypes.c_int
    f.argtypes = [vp] * 8 + [ctypes.POINTER(_abi.HwyStepInfo), vp]
    bufs = [vp(FAKE)] * 5 + [None, None]
    info = _abi.HwyStepInfo()
    assert f(None, *bufs, ctypes.byref(info), None) == -1  # NULL handle
    assert b"handle" in lib.hwy_last_error()
    # the remaining checks come before the handle is read: a fake non-NULL handle is enough
    h = vp(FAKE)
    assert f(h, *bufs, None, None) == -1  # NULL info
    assert b"info is NULL" in lib.hwy_last_error()
    info = _abi.HwyStepInfo(ep_stats=FAKE)  # ep_stats without acc
    assert f(h, *bufs, ctypes.byref(info), None) == -1
    assert b"acc" in lib.hwy_last_error()
    assert f(h, None, *bufs[1:], ctypes.byref(_abi.HwyStepInfo()), None) == -1  # NULL actions


def test_group_info_table_and_argument_checks(lib):
    vp = ctypes.c_void_p
    nb = lib.hwy_step_group_info_table_bytes
    nb.restype = ctypes.c_int64
    nb.argtypes = [ctypes.c_int]
    assert nb(0) == -1 and nb(-3) == -1
    assert nb(1) == ctypes.sizeof(_abi.HwyStepInfo) and nb(3) == 3 * nb(1) and nb(4) > nb(3)
    p = lib.hwy_step_group_info_prepare
    p.restype = ctypes.c_int
    p.argtypes = [vp, vp, vp, ctypes.c_int, vp, vp, ctypes.POINTER(HwyStepGroupPlan), vp]
    plan = HwyStepGroupPlan()
    io = (HwyStepIO * 1)(HwyStepIO(*([FAKE] * 5 + [None, None])))
    info = (_abi.HwyStepInfo * 1)()
    handles = (vp * 1)(None)
    assert p(handles, io, None, 1, vp(FAKE), vp(FAKE), ctypes.byref(plan), None) == -1
    assert p(handles, io, info, 1, vp(FAKE), None, ctypes.byref(plan), None) == -1
    assert p(handles, io, info, 0, vp(FAKE), vp(FAKE), ctypes.byref(plan), None) == -1
    bad = (_abi.HwyStepInfo * 1)(_abi.HwyStepInfo(ep_stats=FAKE))
    assert p((vp * 1)(FAKE), io, bad, 1, vp(FAKE), vp(FAKE), ctypes.byref(plan), None) == -1
    assert b"acc" in lib.hwy_last_error()
    assert p(handles, io, info, 1, vp(FAKE), vp(FAKE), ctypes.byref(plan), None) == -1  # NULL handle
    assert b"NULL" in lib.hwy_last_error()
    s = lib.hwy_step_group_info
    s.restype = ctypes.c_int
    s.argtypes = [ctypes.POINTER(HwyStepGroupPlan), vp, vp, vp]
    assert s(ctypes.byref(HwyStepGroupPlan(1, 1, 0)), vp(FAKE), None, None) == -1
    assert s(ctypes.byref(HwyStepGroupPlan(0, 0, 0)), vp(FAKE), vp(FAKE), None) == -1
    assert s(None, vp(FAKE), vp(FAKE), None) == -1


def _exp(seed, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=64, hidden_dim=256, d_embed=None)
    hp.steps_per_update = 16 * 32
    return Experiment(name=f"c{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=24, target_reward=1e9,
                      extra=dict({"num_envs": 16, "eval_interval": 8}, **extra),
                      env_config_overrides={})


def test_check_batch_rejects_cells_that_disagree_on_episode_stats():
    from experiments.runner import ExperimentRunner

    for own in (False, True):
        ExperimentRunner.check_batch([[_exp(1, episode_stats=True)], [_exp(2, episode_stats=True)]],
                                     own_schedules=own)
        ExperimentRunner.check_batch([[_exp(1)], [_exp(2, episode_stats=False)]],
                                     own_schedules=own)
        with pytest.raises(ValueError, match="episode_stats"):
            ExperimentRunner.check_batch([[_exp(1, episode_stats=True)], [_exp(2)]],
                                         own_schedules=own)
    # within a cell the experiments differ only in seed and name
    with pytest.raises(ValueError, match="differ only in seed"):
        ExperimentRunner.check_batch([[_exp(1, episode_stats=True), _exp(2)]])


def test_crash_rate_is_over_the_last_hundred_episodes():
    from training.routine import crash_rate

    assert crash_rate([]) == 0.0
    assert crash_rate([True, False, False, True]) == 0.5
    assert crash_rate([True] * 50 + [False] * 100) == 0.0
    assert crash_rate([False] * 100 + [True] * 25) == 0.25
