"""Sweep cells that differ in batch_size, num_minibatches and epochs in one batch, without a GPU:
ExperimentRunner.check_batch's rules as launch_batch applies them (own_schedules=True), the schedule arithmetic of ppo/group.py (what
hwy_ppo_sched_prepare writes into its plan and the step kernels evaluate per slot) and the
hwy_ppo_sched_* calls' argument checks, none of which touches a device."""

import ctypes
import functools

import pytest


def _exp(seed, **kw):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=kw.pop("epochs", 2),
                     batch_size=kw.pop("batch_size", 64), hidden_dim=kw.pop("hidden_dim", 256),
                     d_embed=None)
    hp.steps_per_update = kw.pop("steps_per_update", 16 * 32)
    extra = {"num_envs": kw.pop("num_envs", 16), "eval_interval": 8}
    if "num_minibatches" in kw:
        extra["num_minibatches"] = kw.pop("num_minibatches")
    return Experiment(name=f"c{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=kw.pop("max_episodes", 24), target_reward=1e9, extra=extra,
                      env_config_overrides={})


def test_check_batch_accepts_cells_of_different_batch_size_epochs_and_minibatch_count():
    from experiments.runner import ExperimentRunner

    check = functools.partial(ExperimentRunner.check_batch, own_schedules=True)
    check([[_exp(42, batch_size=64), _exp(1042, batch_size=64)], [_exp(7, batch_size=32)]])
    check([[_exp(42, epochs=2)], [_exp(7, epochs=3)], [_exp(9, epochs=10)]])
    check([[_exp(42, num_minibatches=8)], [_exp(7, num_minibatches=4)]])
    check([[_exp(42, batch_size=64, epochs=6, hidden_dim=128)],
           [_exp(7, batch_size=32, epochs=10, hidden_dim=384)]])
    # the reference grid's update: 16 envs x 128 steps = 2,048 samples
    check([[_exp(s + 10 * e + b, steps_per_update=2048, epochs=e, batch_size=b)]
           for s, e in enumerate((6, 8, 10)) for b in (32, 64)])


def test_check_batch_without_own_schedules_keeps_one_schedule_per_batch():
    """The default is the stricter check of a batch whose cells step the same minibatch index
    together; launch_batch asks for own_schedules."""
    from experiments.runner import ExperimentRunner

    for kw in (dict(epochs=3), dict(batch_size=32), dict(num_minibatches=4)):
        cells = [[_exp(42)], [_exp(7, **kw)]]
        with pytest.raises(ValueError, match="must share"):
            ExperimentRunner.check_batch(cells)
        ExperimentRunner.check_batch(cells, own_schedules=True)
    ExperimentRunner.check_batch([[_exp(42)], [_exp(7, hidden_dim=384)]])


def test_check_batch_still_rejects_cells_that_cannot_share_the_rollout():
    from experiments.runner import ExperimentRunner

    check = functools.partial(ExperimentRunner.check_batch, own_schedules=True)
    with pytest.raises(ValueError, match="must share.*c7"):
        check([[_exp(42)], [_exp(7, num_envs=8)]])
    with pytest.raises(ValueError, match="must share.*c7"):
        check([[_exp(42)], [_exp(7, steps_per_update=16 * 64)]])
    with pytest.raises(ValueError, match="must share.*c7"):
        check([[_exp(42)], [_exp(7, max_episodes=48)]])
    with pytest.raises(ValueError, match="differ only in seed"):
        check([[_exp(42, epochs=2), _exp(1042, epochs=3)]])


def test_check_batch_rejects_a_cell_with_unequal_or_oversized_minibatches():
    from experiments.runner import GROUPED_MINIBATCH_ROWS, ExperimentRunner

    check = functools.partial(ExperimentRunner.check_batch, own_schedules=True)
    # 2,048 samples in minibatches of 48: 42 of them and a short one of 32
    with pytest.raises(ValueError, match=r"cell c7 .*\[32, 48\]"):
        check([[_exp(42, steps_per_update=2048)],
               [_exp(7, steps_per_update=2048, batch_size=48)]])
    with pytest.raises(ValueError, match=r"cell c7 .*\[170, 171\]"):
        check([[_exp(42)], [_exp(7, num_minibatches=3)]])  # 512 = 171 + 171 + 170
    n = 2 * GROUPED_MINIBATCH_ROWS
    with pytest.raises(ValueError, match="cell c7 .*16-row tiles"):
        check([[_exp(42, steps_per_update=n)],
               [_exp(7, steps_per_update=n, batch_size=GROUPED_MINIBATCH_ROWS)]])
    check([[_exp(42, steps_per_update=n)],
           [_exp(7, steps_per_update=n, batch_size=GROUPED_MINIBATCH_ROWS // 2)]])


# (nmb, epochs) per learner: the ABI test's six, the reference grid's six classes at 2,048
# samples, a single learner, and co-prime step counts
SCHEDULES = [
    [(4, 2), (8, 3), (4, 3), (8, 2), (6, 2), (4, 2)],
    [(64, 6), (32, 6), (64, 8), (32, 8), (64, 10), (32, 10)],
    [(5, 3)],
    [(3, 3), (2, 2), (7, 1)],
]


@pytest.mark.parametrize("learners", SCHEDULES)
def test_schedule_arithmetic_against_a_plain_double_loop(learners):
    from ppo.group import graph_slots, slot_minibatch, update_schedule

    nmbs, epochs = [l[0] for l in learners], [l[1] for l in learners]
    max_steps, period = update_schedule(nmbs, epochs)
    steps = [n * e for n, e in learners]
    assert max_steps == max(steps)
    assert all(s % period == 0 for s in steps)
    assert not any(all(s % d == 0 for s in steps) for d in range(period + 1, max_steps + 1))
    for nmb, ep in learners:
        # a solo update: epochs outside, minibatches inside
        want = [i for _ in range(ep) for i in range(nmb)]
        got = [slot_minibatch(s, nmb, ep) for s in range(max_steps + 3)]
        assert got[:len(want)] == want
        assert all(g is None for g in got[len(want):])
        assert slot_minibatch(-1, nmb, ep) is None
    # the captured graph: P slots replayed ceil(max_steps / P) times covers every slot once
    P = graph_slots(period)
    assert period % P == 0 and 1 <= P <= 256
    replays = -(-max_steps // P)
    assert (replays - 1) * P < max_steps <= replays * P


def test_schedule_of_the_issue_tables():
    from ppo.group import graph_slots, update_schedule

    assert update_schedule([4, 8, 4, 8, 6, 4], [2, 3, 3, 2, 2, 2]) == (24, 4)
    # the reference grid at 2,048 samples: 640 slots instead of 2,304 steps class by class
    assert update_schedule([64, 32, 64, 32, 64, 32], [6, 6, 8, 8, 10, 10]) == (640, 64)
    assert sum(n * e for n, e in SCHEDULES[1]) == 2304
    assert graph_slots(64) == 64 and graph_slots(640) == 160 and graph_slots(1) == 1
    assert graph_slots(2 * 3 * 127, cap=256) == 254
    with pytest.raises(ValueError):
        update_schedule([4, 0], [2, 2])
    with pytest.raises(ValueError):
        update_schedule([4, 4], [2, 0])


# ---------------------------------------------------------------- the C ABI, on the host
def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _table_bytes(L, dims, nmb):
    from hwy.ppo_native import PpoDims

    arr = (PpoDims * max(1, len(dims)))(*[PpoDims(*d) for d in dims])
    n = (ctypes.c_int32 * max(1, len(nmb)))(*nmb)
    return L.hwy_ppo_sched_table_bytes(arr, n, len(dims))


def test_sched_symbols_and_plan_struct():
    """include/hwy_ppo.h: hwy_ppo_sched_plan is 12 int32."""
    from hwy.ppo_native import PpoSchedPlan

    L = _lib()
    for name in ("hwy_ppo_sched_table_bytes", "hwy_ppo_sched_prepare", "hwy_ppo_sched_begin",
                 "hwy_ppo_sched_step", "hwy_ppo_sched_advance"):
        assert hasattr(L, name), name
    assert ctypes.sizeof(PpoSchedPlan) == 48
    assert [f[0] for f in PpoSchedPlan._fields_] == [
        "G", "present", "grid_rows", "lds_bytes", "grid_wgrad", "grid_wsum", "grid_adam",
        "max_steps", "period"]
    p = PpoSchedPlan()
    p.present[0], p.present[1] = 4, 2
    assert p.launches == 5
    p.present[1] = 0
    assert p.launches == 4


def test_sched_table_bytes_grows_with_learners_and_minibatches():
    L = _lib()
    dims = [(64, 60, 128, 2), (32, 120, 256, 2), (40, 60, 192, 2)]   # B differs per learner
    sizes = [_table_bytes(L, dims[:g], [4, 8, 6][:g]) for g in (1, 2, 3)]
    assert 0 < sizes[0] < sizes[1] < sizes[2], sizes
    assert _table_bytes(L, dims, [64, 64, 64]) > sizes[2]
    assert _table_bytes(L, [], []) == -1
    assert L.hwy_ppo_sched_table_bytes(None, None, 2) == -1
    assert _table_bytes(L, dims, [4, 0, 6]) == -1                       # nmb < 1
    assert _table_bytes(L, dims[:2] + [(40, 60, 96, 2)], [4, 8, 6]) == -1   # H = 96
    assert _table_bytes(L, dims[:2] + [(40, 60, 192, 3)], [4, 8, 6]) == -1  # A differs
    # 8,192 rows take the 32-row tiles on a 256-CU part (the geometry assumed without a device)
    assert _table_bytes(L, dims[:2] + [(8192, 60, 192, 2)], [4, 8, 6]) == -1


def test_sched_calls_refuse_null_and_empty_arguments():
    from hwy.ppo_native import PpoSchedPlan

    L = _lib()
    plan = PpoSchedPlan()
    table = ctypes.create_string_buffer(8192)
    one = (ctypes.c_int32 * 2)(1, 1)
    assert L.hwy_ppo_sched_prepare(None, one, one, 2, table, ctypes.byref(plan), None) == -1
    for call in (lambda p, t: L.hwy_ppo_sched_begin(p, t, None),
                 lambda p, t: L.hwy_ppo_sched_step(p, t, 0, None),
                 lambda p, t: L.hwy_ppo_sched_advance(p, t, 4, None)):
        assert call(None, table) == -1
        assert call(ctypes.byref(plan), None) == -1
        assert call(ctypes.byref(plan), table) == -1   # an empty plan: refused before any launch
