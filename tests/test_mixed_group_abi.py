"""The mixed-width grouped calls of libhwy.so (include/hwy_ppo.h: hwy_ppo_mixed_*) and
ExperimentRunner.launch_batch's argument checks for cells of different hidden widths, without a
GPU: symbols, table sizes, refused dims and NULL arguments (none of which touches a device)."""

import ctypes

import pytest


def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _table_bytes(L, dims):
    from hwy.ppo_native import PpoDims

    arr = (PpoDims * max(1, len(dims)))(*[PpoDims(*d) for d in dims])
    return L.hwy_ppo_mixed_table_bytes(arr, len(dims))


def test_mixed_symbols_exist():
    L = _lib()
    for name in ("hwy_ppo_mixed_table_bytes", "hwy_ppo_mixed_prepare", "hwy_ppo_mixed_step",
                 "hwy_ppo_mixed_act_table_bytes", "hwy_ppo_mixed_act_prepare",
                 "hwy_ppo_mixed_act"):
        assert hasattr(L, name), name


def test_mixed_table_bytes_grows_with_learners():
    L = _lib()
    dims = [(64, 60, 128, 2), (64, 120, 256, 2), (64, 60, 384, 2)]
    sizes = [_table_bytes(L, dims[:g]) for g in (1, 2, 3)]
    assert sizes[0] > 0 and sizes[0] < sizes[1] < sizes[2], sizes
    # both wave-count classes (H 64 and 192 run 4 waves) in one table
    assert _table_bytes(L, dims + [(64, 60, 64, 2), (64, 120, 192, 2)]) > sizes[2]


def test_mixed_table_bytes_refuses_unsupported_dims():
    L = _lib()
    assert _table_bytes(L, []) == -1                                      # G = 0
    assert L.hwy_ppo_mixed_table_bytes(None, 2) == -1
    assert _table_bytes(L, [(64, 60, 128, 2), (64, 60, 96, 2)]) == -1     # H = 96
    assert _table_bytes(L, [(64, 60, 128, 2), (48, 60, 256, 2)]) == -1    # B differs
    # 8,192 rows take the 32-row tiles on a 256-CU part (the geometry assumed without a device)
    assert _table_bytes(L, [(8192, 60, 128, 2), (8192, 60, 256, 2)]) == -1
    assert _table_bytes(L, [(64, 60, 128, 2), (64, 60, 256, 3)]) == -1    # A differs / not 2
    assert L.hwy_ppo_mixed_act_table_bytes(0) == -1
    assert L.hwy_ppo_mixed_act_table_bytes(3) > 0


def test_mixed_launches_refuse_null_arguments():
    from hwy.ppo_native import PpoMixedActPlan, PpoMixedPlan

    L = _lib()
    assert L.hwy_ppo_mixed_step(None, None, None) == -1
    assert L.hwy_ppo_mixed_act(None, None, None) == -1
    plan, aplan = PpoMixedPlan(), PpoMixedActPlan()
    assert L.hwy_ppo_mixed_step(ctypes.byref(plan), None, None) == -1
    assert L.hwy_ppo_mixed_act(ctypes.byref(aplan), None, None) == -1
    table = ctypes.create_string_buffer(4096)
    assert L.hwy_ppo_mixed_step(None, table, None) == -1
    assert L.hwy_ppo_mixed_act(None, table, None) == -1
    # an empty plan (no learners, no class present) is refused before any launch
    assert L.hwy_ppo_mixed_step(ctypes.byref(plan), table, None) == -1
    assert L.hwy_ppo_mixed_act(ctypes.byref(aplan), table, None) == -1
    assert L.hwy_ppo_mixed_prepare(None, 2, table, ctypes.byref(plan), None) == -1
    assert L.hwy_ppo_mixed_act_prepare(None, 2, table, ctypes.byref(aplan), None) == -1


def test_plan_structs_match_the_header():
    """include/hwy_ppo.h: hwy_ppo_mixed_plan is 11 int32, hwy_ppo_mixed_act_plan 7."""
    from hwy.ppo_native import PpoMixedActPlan, PpoMixedPlan

    assert ctypes.sizeof(PpoMixedPlan) == 44 and ctypes.sizeof(PpoMixedActPlan) == 28
    p = PpoMixedPlan()
    p.present[0], p.present[1] = 3, 0
    assert p.launches == 4
    p.present[1] = 2
    assert p.launches == 5


def _exp(seed, **kw):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=kw.pop("epochs", 2), batch_size=64,
                     hidden_dim=kw.pop("hidden_dim", 256), d_embed=None)
    hp.steps_per_update = 16 * 32
    extra = {"num_envs": 16, "num_minibatches": 8, "eval_interval": 8}
    return Experiment(name=f"g{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=24, target_reward=1e9, extra=extra, env_config_overrides={})


def test_launch_batch_accepts_cells_of_different_hidden_widths():
    """The cells of one launch_batch may differ in hidden_dim (they no longer "must share" it);
    within a cell the experiments still differ only in seed, and the cells still share what one
    GroupBatch's launches share."""
    from experiments.runner import ExperimentRunner

    cells = [[_exp(42, hidden_dim=256), _exp(1042, hidden_dim=256)],
             [_exp(7, hidden_dim=384), _exp(2042, hidden_dim=384)]]
    ExperimentRunner.check_batch(cells)  # no ValueError
    with pytest.raises(ValueError, match="differ only in seed"):
        ExperimentRunner.check_batch([[_exp(42, hidden_dim=256), _exp(1042, hidden_dim=384)]])
    with pytest.raises(ValueError, match="must share"):
        ExperimentRunner.check_batch([[_exp(42, epochs=2)], [_exp(7, epochs=4)]])
