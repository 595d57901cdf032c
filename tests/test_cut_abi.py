"""The reference episode schedule without a GPU: hwy_cut_episodes' argument checks, the runner's
batch checks (num_envs 1 only on the reference schedule, one schedule per batch) and the order
of the episode stream (training/routine.py:_episode_stream)."""

import numpy as np
import pytest
import torch


def _exp(seed, schedule=None, num_envs=1, name=None):
    from experiments.config import Condition, ConditionHP, Experiment

    hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=8, hidden_dim=64, d_embed=None)
    hp.steps_per_update = 24
    extra = {"num_envs": num_envs, "eval_interval": 8}
    if schedule is not None:
        extra["episode_schedule"] = schedule
    return Experiment(name=name or f"c{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                      max_episodes=12, target_reward=1e9, extra=extra, env_config_overrides={})


def test_cut_episodes_rejects_null_handle_and_null_obs():
    from hwy.native import HWY_EINVAL, last_error, lib

    L = lib()
    assert L.hwy_abi_version() == 1
    assert L.hwy_cut_episodes(None, None, None, None, None, None) == HWY_EINVAL == -1
    assert "NULL" in last_error()


def test_check_batch_accepts_one_env_on_the_reference_schedule():
    from experiments.runner import ExperimentRunner

    ExperimentRunner.check_batch([[_exp(42, "reference"), _exp(1042, "reference")]],
                                 own_schedules=True)
    ExperimentRunner.check_batch([[_exp(42, "reference")], [_exp(7, "reference")]],
                                 own_schedules=True)


def test_check_batch_refuses_one_env_without_the_reference_schedule():
    from experiments.runner import ExperimentRunner

    for schedule in (None, "lockstep"):
        with pytest.raises(ValueError, match="num_envs"):
            ExperimentRunner.check_batch([[_exp(42, schedule), _exp(1042, schedule)]],
                                         own_schedules=True)


def test_check_batch_refuses_mixed_schedules_and_unknown_ones():
    from experiments.runner import ExperimentRunner

    with pytest.raises(ValueError, match="episode_schedule"):
        ExperimentRunner.check_batch([[_exp(42, "reference", num_envs=4)],
                                      [_exp(7, "lockstep", num_envs=4)]], own_schedules=True)
    with pytest.raises(ValueError, match="episode_schedule"):
        ExperimentRunner.check_batch([[_exp(42, "reference", num_envs=4)],
                                      [_exp(7, None, num_envs=4)]], own_schedules=True)
    with pytest.raises(ValueError, match="episode_schedule"):
        ExperimentRunner.check_batch([[_exp(42, "sometimes", num_envs=4)]], own_schedules=True)


def test_episode_stream_books_finished_episodes_before_cut_ones():
    from training.routine import _episode_ends, _episode_stream

    T, E = 4, 3
    dones = torch.zeros(T, E, dtype=torch.uint8)
    rets = torch.zeros(T, E)
    # finished: (t 1, env 2) 5.0, (t 3, env 0) 7.0, (t 3, env 1) 9.0 -- (step, env) order
    for t, e, r in ((3, 1, 9.0), (1, 2, 5.0), (3, 0, 7.0)):
        dones[t, e] = 1
        rets[t, e] = r
    rets[0, 0] = 123.0  # a return where nothing finished is not an episode
    # envs 0 and 1 finished on the last step (nothing to cut); env 2 is cut at 2.5
    cut = torch.tensor([0, 0, 1], dtype=torch.uint8)
    cut_ret = torch.tensor([0.0, 0.0, 2.5])
    got = _episode_stream(dones, rets, cut, cut_ret)
    assert got.tolist() == [5.0, 7.0, 9.0, 2.5]
    assert _episode_ends(dones, rets).tolist() == [5.0, 7.0, 9.0]
    # every env cut, none finished: env order; a cut byte of 0 hides its return
    none = torch.zeros(T, E, dtype=torch.uint8)
    got = _episode_stream(none, rets, torch.tensor([1, 0, 1], dtype=torch.uint8),
                          torch.tensor([1.5, 99.0, 0.25]))
    assert got.tolist() == [1.5, 0.25]
    assert isinstance(got, np.ndarray)


def test_rollout_chunks_cover_the_rollout_once():
    from ppo.rollout import REFERENCE_GRAPH_CHUNK, rollout_chunks

    assert rollout_chunks(2048, "lockstep") == [(0, 2048)]
    assert rollout_chunks(24, "reference") == [(0, 24)]
    for T in (REFERENCE_GRAPH_CHUNK + 1, 2048, 2049):
        ch = rollout_chunks(T, "reference")
        assert ch[0][0] == 0 and ch[-1][1] == T
        assert all(a[1] == b[0] for a, b in zip(ch, ch[1:]))
        assert all(0 < t1 - t0 <= REFERENCE_GRAPH_CHUNK for t0, t1 in ch)


def test_train_refuses_the_reference_schedule_over_a_process_group():
    from training.routine import train_with_experiment_name

    class _Agent:
        _dist = object()

    with pytest.raises(ValueError, match="process group"):
        train_with_experiment_name(env=None, agent=_Agent(), episode_schedule="reference")
