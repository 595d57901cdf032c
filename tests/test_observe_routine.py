"""What training/routine.py and experiments/runner.py build on hwy_observe, without a device:
attribution_shade's arithmetic, and the refusals of evaluate(order=...), eval_orders and
visualize_agent(attribution=...)."""

from __future__ import annotations

import numpy as np
import pytest
import torch

from training import routine


class FakeVec:
    """HighwayVecEnv's part in attribution_shade: the row values come back as they went in"""

    def __init__(self, E, N):
        self.num_envs, self.obs_rows, self.calls = E, N, []

    def rows_to_vehicles(self, row_values, order=None, out=None):
        self.calls.append((row_values, order))
        return row_values


def shade_loop(grad, E, N):
    """attribution_shade's statistic as a float64 loop"""
    g = np.asarray(grad, np.float64).reshape(E, N, -1)
    out = np.zeros((E, N))
    for e in range(E):
        mass = [sum(abs(float(x)) for x in g[e, r]) for r in range(N)]
        top = max(mass)
        for r in range(N):
            out[e, r] = mass[r] / top if top > 0 else 0.0
    return out


def test_attribution_shade_against_the_loop():
    E, N, Fo = 6, 5, 7
    rng = np.random.default_rng(0)
    grad = rng.normal(size=(E, N * Fo)).astype(np.float32)
    grad[1] = 0.0                      # an all-zero gradient
    grad[2, Fo:] = 0.0                 # all the mass on row 0
    grad[3] *= 1e-30                   # tiny masses still divide to 1.0 on the largest row
    grad[4, :Fo] = grad[4, 2 * Fo:3 * Fo]   # two rows share the largest mass...
    grad[4, :Fo] *= 4.0
    grad[4, 2 * Fo:3 * Fo] *= -4.0          # ...with opposite signs
    vec = FakeVec(E, N)
    got = routine.attribution_shade(vec, torch.from_numpy(grad), order="shuffled")
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (E, N)
    assert vec.calls[0][1] == "shuffled"
    got = got.numpy()
    want = shade_loop(grad, E, N)
    # float32 against float64: a sum of Fo = 7 non-negative terms carries at most Fo - 1
    # roundings, the quotient of two such sums both and one of its own
    np.testing.assert_allclose(got, want, rtol=(2 * (Fo - 1) + 1) * 2.0 ** -24, atol=0)
    assert (got.max(axis=1)[[0, 2, 3, 4, 5]] == 1.0).all(), "exactly 1.0 on the largest row"
    assert (got[1] == 0.0).all() and not np.signbit(got[1]).any(), "exactly 0 for a zero gradient"
    assert list(got[2]) == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert got[4, 0] == 1.0 and got[4, 2] == 1.0
    assert ((got >= 0.0) & (got <= 1.0)).all()


def test_attribution_shade_takes_the_envs_own_order_by_default():
    vec = FakeVec(2, 3)
    routine.attribution_shade(vec, torch.ones(2, 12))
    assert vec.calls[0][1] is None and torch.equal(vec.calls[0][0], torch.ones(2, 3))


class OneEnv:
    """a non-vector env: nothing of it may be touched before the refusal"""

    @property
    def unwrapped(self):
        return self

    def reset(self, **kw):
        raise AssertionError("the env was used")


@pytest.mark.parametrize("order", ["sorted", "shuffled", "other"])
def test_evaluate_order_needs_a_vector_env(order):
    with pytest.raises(ValueError, match="HighwayVecEnv"):
        routine.evaluate(OneEnv(), agent=None, num_episodes=2, exp_seed=1, order=order)


def test_evaluate_order_refuses_an_unknown_order_before_running():
    class Vec(OneEnv):
        is_vector_env = True

    with pytest.raises(ValueError, match="order must be"):
        routine.evaluate(Vec(), agent=None, num_episodes=2, exp_seed=1, order="reversed")


def test_eval_orders_names():
    assert routine.check_eval_orders(None) == [] and routine.check_eval_orders([]) == []
    assert routine.check_eval_orders(("shuffled", "sorted")) == ["shuffled", "sorted"]
    for bad in (["sorted", "sorted"], ["both"], [None], "sorted"):
        with pytest.raises(ValueError, match="eval_orders"):
            routine.check_eval_orders(bad)


def test_training_with_eval_orders_needs_a_vector_env():
    with pytest.raises(ValueError, match="eval_orders needs a HighwayVecEnv"):
        routine.train_with_experiment_name(OneEnv(), agent=None, eval_orders=["sorted"])


def test_visualize_agent_refuses_an_unknown_output():
    with pytest.raises(ValueError, match="attribution must be"):
        routine.visualize_agent(OneEnv(), agent=None, attribution="speed")


def test_grouped_launches_refuse_eval_orders():
    from config.base_config import HIGHWAY_CONFIG
    from experiments.config import Condition, ConditionHP, Experiment
    from experiments.runner import ExperimentRunner

    def exp(seed):
        hp = ConditionHP(lr=3e-4, clip_eps=0.2, epochs=2, batch_size=16, hidden_dim=64,
                         d_embed=None)
        hp.steps_per_update = 64
        return Experiment(name=f"o{seed}", condition=Condition.SORTED, hp=hp, seed=seed,
                          max_episodes=12, target_reward=1e9,
                          extra={"num_envs": 4, "eval_orders": ["sorted", "shuffled"]},
                          env_config_overrides={})

    r = ExperimentRunner(HIGHWAY_CONFIG)
    with pytest.raises(ValueError, match="eval_orders"):
        r.launch_group([exp(42), exp(1042)])
    with pytest.raises(ValueError, match="eval_orders"):
        r.launch_batch([[exp(42)], [exp(7)]])
