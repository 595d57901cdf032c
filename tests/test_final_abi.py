"""hwy_step_with_final / hwy_step_group_final / hwy_gae_boot (include/hwy.h) and
hwy_ppo_value_masked (include/hwy_ppo.h) without a GPU: the symbols exist and are bound, the
layouts the option must not touch are untouched, every argument the calls must refuse is refused
before any device call, and the launches that do not support truncation="bootstrap" say so."""

import ctypes

import pytest

from hwy import _abi
from hwy.native import LIB_PATH, HwyStepGroupPlan, HwyStepIO

NEW = ("hwy_step_with_final", "hwy_step_group_final_table_bytes", "hwy_step_group_final_prepare",
       "hwy_step_group_final", "hwy_gae_boot", "hwy_ppo_value_masked")
FAKE = 4096  # a non-NULL address that no refused call may touch
OTHER = 8192


@pytest.fixture(scope="module")
def lib():
    L = ctypes.CDLL(LIB_PATH)
    L.hwy_last_error.restype = ctypes.c_char_p
    return L


def test_final_symbols_and_untouched_layouts(lib):
    for name in NEW:
        assert hasattr(lib, name), name
    assert lib.hwy_abi_version() == _abi.HWY_ABI_VERSION == 1
    assert lib.hwy_config_size() == ctypes.sizeof(_abi.HwyConfig)
    assert lib.hwy_step_info_size() == ctypes.sizeof(_abi.HwyStepInfo) == 6 * ctypes.sizeof(
        ctypes.c_void_p)


def test_ctypes_argtypes_are_bound():
    from hwy import native, ppo_native

    L = ppo_native._bind(native.lib())
    vp = ctypes.c_void_p
    assert len(L.hwy_step_with_final.argtypes) == 11
    assert L.hwy_step_with_final.argtypes[8] == ctypes.POINTER(_abi.HwyStepInfo)
    assert L.hwy_step_group_final_table_bytes.restype == ctypes.c_int64
    assert len(L.hwy_step_group_final_prepare.argtypes) == 9
    assert L.hwy_step_group_final_prepare.argtypes[7] == ctypes.POINTER(HwyStepGroupPlan)
    assert L.hwy_step_group_final.argtypes == [ctypes.POINTER(HwyStepGroupPlan), vp, vp, vp]
    assert len(L.hwy_gae_boot.argtypes) == 13
    assert L.hwy_gae_boot.argtypes[6] == L.hwy_gae_boot.argtypes[7] == ctypes.c_double
    assert L.hwy_ppo_value_masked.argtypes == [ctypes.POINTER(ppo_native.PpoActArgs), vp, vp, vp]
    for name in ("hwy_step_with_final", "hwy_step_group_final_prepare", "hwy_step_group_final",
                 "hwy_gae_boot", "hwy_ppo_value_masked"):
        assert getattr(L, name).restype == ctypes.c_int, name


def test_step_with_final_refuses_bad_arguments_before_any_device_call(lib):
    vp = ctypes.c_void_p
    f = lib.hwy_step_with_final
    f.restype = ctypes.c_int
    f.argtypes = [vp] * 8 + [ctypes.POINTER(_abi.HwyStepInfo), vp, vp]
    bufs = [vp(FAKE)] * 5 + [None, None]  # actions, obs, reward, terminated, truncated
    assert f(None, *bufs, None, vp(OTHER), None) == -1  # NULL handle
    assert b"handle" in lib.hwy_last_error()
    # the remaining checks come before the handle is read: a fake non-NULL handle is enough
    h = vp(FAKE)
    assert f(h, *bufs, None, None, None) == -1  # NULL final_obs
    assert b"final_obs is NULL" in lib.hwy_last_error()
    assert f(h, *bufs, None, vp(FAKE), None) == -1  # final_obs == obs
    assert b"obs buffer" in lib.hwy_last_error()
    info = _abi.HwyStepInfo(ep_stats=FAKE)  # ep_stats without acc
    assert f(h, *bufs, ctypes.byref(info), vp(OTHER), None) == -1
    assert b"acc" in lib.hwy_last_error()
    assert f(h, None, *bufs[1:], None, vp(OTHER), None) == -1  # NULL actions
    assert b"non-NULL" in lib.hwy_last_error()


def test_group_final_table_and_argument_checks(lib):
    vp = ctypes.c_void_p
    nb = lib.hwy_step_group_final_table_bytes
    nb.restype = ctypes.c_int64
    nb.argtypes = [ctypes.c_int]
    assert nb(0) == -1 and nb(-3) == -1
    assert nb(1) >= ctypes.sizeof(_abi.HwyStepInfo) + ctypes.sizeof(vp)
    assert nb(3) == 3 * nb(1) and nb(4) > nb(3)
    p = lib.hwy_step_group_final_prepare
    p.restype = ctypes.c_int
    p.argtypes = [vp, vp, vp, vp, ctypes.c_int, vp, vp, ctypes.POINTER(HwyStepGroupPlan), vp]
    plan = HwyStepGroupPlan()
    io = (HwyStepIO * 1)(HwyStepIO(*([FAKE] * 5 + [None, None])))
    fin = (vp * 1)(OTHER)
    fake_h = (vp * 1)(FAKE)
    args = (1, vp(FAKE), vp(FAKE), ctypes.byref(plan), None)
    assert p(fake_h, io, None, None, *args) == -1  # NULL final_obs array
    assert b"NULL" in lib.hwy_last_error()
    assert p(fake_h, io, None, fin, 1, vp(FAKE), None, ctypes.byref(plan), None) == -1
    assert p(fake_h, io, None, fin, 0, vp(FAKE), vp(FAKE), ctypes.byref(plan), None) == -1
    assert p(fake_h, io, None, (vp * 1)(None), *args) == -1  # a handle's final_obs NULL
    assert b"final_obs is NULL" in lib.hwy_last_error()
    assert p(fake_h, io, None, (vp * 1)(FAKE), *args) == -1  # a handle's final_obs == its obs
    assert b"obs buffer" in lib.hwy_last_error()
    bad = (_abi.HwyStepInfo * 1)(_abi.HwyStepInfo(ep_stats=FAKE))
    assert p(fake_h, io, bad, fin, *args) == -1
    assert b"acc" in lib.hwy_last_error()
    assert p((vp * 1)(None), io, None, fin, *args) == -1  # NULL handle, info NULL is allowed
    assert b"handle 0" in lib.hwy_last_error()
    s = lib.hwy_step_group_final
    s.restype = ctypes.c_int
    s.argtypes = [ctypes.POINTER(HwyStepGroupPlan), vp, vp, vp]
    assert s(ctypes.byref(HwyStepGroupPlan(1, 1, 0)), vp(FAKE), None, None) == -1
    assert s(ctypes.byref(HwyStepGroupPlan(0, 0, 0)), vp(FAKE), vp(FAKE), None) == -1
    assert s(None, vp(FAKE), vp(FAKE), None) == -1


def test_gae_boot_refuses_negative_shapes(lib):
    vp = ctypes.c_void_p
    g = lib.hwy_gae_boot
    g.restype = ctypes.c_int
    g.argtypes = [vp] * 6 + [ctypes.c_double, ctypes.c_double, ctypes.c_int, ctypes.c_int, vp, vp,
                             vp]
    ptrs = [vp(FAKE)] * 6
    assert g(*ptrs, 0.99, 0.95, -1, 4, vp(FAKE), vp(FAKE), None) == -1
    assert b"hwy_gae_boot" in lib.hwy_last_error() and b"T=-1" in lib.hwy_last_error()
    assert g(*ptrs, 0.99, 0.95, 4, -2, vp(FAKE), vp(FAKE), None) == -1
    assert b"E=-2" in lib.hwy_last_error()
    # an empty rollout is a no-op that touches nothing
    assert g(*ptrs, 0.99, 0.95, 0, 4, vp(FAKE), vp(FAKE), None) == 0
    assert g(*ptrs, 0.99, 0.95, 4, 0, vp(FAKE), vp(FAKE), None) == 0


def test_value_masked_refuses_bad_arguments(lib):
    from hwy.ppo_native import PpoActArgs, PpoDims

    vp = ctypes.c_void_p
    f = lib.hwy_ppo_value_masked
    f.restype = ctypes.c_int
    f.argtypes = [ctypes.POINTER(PpoActArgs), vp, vp, vp]

    def args(S=60, H=256, B=40, **kw):
        a = PpoActArgs()
        a.dims = PpoDims(B, S, H, 2)
        a.states, a.params, a.value = FAKE, FAKE, FAKE
        for k, v in kw.items():
            setattr(a, k, v)
        return a

    assert f(None, vp(FAKE), None, None) == -1
    assert f(ctypes.byref(args()), None, None, None) == -1  # NULL mask
    assert f(ctypes.byref(args(noise=FAKE)), vp(FAKE), None, None) == -1  # noise must be NULL
    assert f(ctypes.byref(args(S=62)), vp(FAKE), None, None) == -1  # S % 4 != 0
    assert f(ctypes.byref(args(H=96)), vp(FAKE), None, None) == -1  # H not a multiple of 64
    assert f(ctypes.byref(args(S=2048)), vp(FAKE), None, None) == -1  # past the fused range
    assert f(ctypes.byref(args(B=0)), vp(FAKE), None, None) == -1
    assert f(ctypes.byref(args(value=None)), vp(FAKE), None, None) == -1


def _exp(seed, **extra):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=64, hidden_dim=256, d_embed=None)
    hp.steps_per_update = 16 * 32
    return Experiment(name=f"c{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=24, target_reward=1e9,
                      extra=dict({"num_envs": 16, "eval_interval": 8}, **extra),
                      env_config_overrides={})


def test_grouped_launches_reject_truncation_bootstrap():
    from experiments.runner import ExperimentRunner

    ExperimentRunner.check_batch([[_exp(1, truncation="terminal")], [_exp(2)]])
    for own in (False, True):
        with pytest.raises(ValueError, match="truncation"):
            ExperimentRunner.check_batch([[_exp(1, truncation="bootstrap")]], own_schedules=own)
        with pytest.raises(ValueError, match="truncation"):
            ExperimentRunner.check_batch([[_exp(1)], [_exp(2, truncation="bootstrap")]],
                                         own_schedules=own)
    runner = ExperimentRunner({})
    with pytest.raises(ValueError, match="truncation"):
        runner.launch_group([_exp(1, truncation="bootstrap"), _exp(2, truncation="bootstrap")])
    with pytest.raises(ValueError, match="truncation"):
        runner.launch_batch([[_exp(1, truncation="bootstrap")]])


def test_unknown_truncation_value_raises():
    from experiments.runner import ExperimentRunner
    from ppo.rollout import TRUNCATIONS, check_truncation

    assert TRUNCATIONS == ("terminal", "bootstrap")
    assert check_truncation("terminal") == "terminal"
    assert check_truncation("bootstrap") == "bootstrap"
    with pytest.raises(ValueError, match="truncation"):
        check_truncation("bootstrapped")
    with pytest.raises(ValueError, match="truncation"):
        ExperimentRunner.check_batch([[_exp(1, truncation="value")]])


def test_one_env_loop_and_missing_buffer_refuse_bootstrap():
    import torch

    from ppo.agent import RolloutBuffer
    from ppo.rollout import LockstepRollout
    from training.routine import train_with_experiment_name

    class OneEnv:  # not a vector env: the reference loop
        @property
        def unwrapped(self):
            return self

    with pytest.raises(ValueError, match="truncation"):
        train_with_experiment_name(OneEnv(), object(), truncation="bootstrap")
    with pytest.raises(ValueError, match="truncation"):
        train_with_experiment_name(OneEnv(), object(), truncation="nonsense")
    buf = RolloutBuffer(2, 3, 8, 2, torch.device("cpu"))
    assert buf.final_obs is None and buf.boot_values is None
    with pytest.raises(ValueError, match="truncation_bootstrap"):
        LockstepRollout(object(), OneEnv(), buf, use_graph=False, truncation="bootstrap")
    buf = RolloutBuffer(2, 3, 8, 2, torch.device("cpu"), truncation_bootstrap=True)
    assert tuple(buf.final_obs.shape) == (3, 8) and tuple(buf.boot_values.shape) == (2, 3)
