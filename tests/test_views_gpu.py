"""The view seam on the device: HighwayVecEnv.view / view_into write, bit for bit, what the
per-kind methods (sense, grid, lidar) write on the same states.  What a rollout under a view
computes is pinned by test_sense_gpu.py, test_grid_routine_gpu.py and test_lidar_routine_gpu.py."""

from __future__ import annotations

import pytest
import torch

from config.base_config import HIGHWAY_CONFIG
from hwy import GridSpec, LidarSpec, SensorModel
from hwy.vec_env import HighwayVecEnv

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E = 2
SPECS = {
    "sensor": (SensorModel(los=True, range=60.0, dropout=0.2, noise=(0.5, 0.2, 0.4), salt=7),
               lambda env, s: env.sense(s).reshape(E, -1)),
    "grid": (GridSpec(), lambda env, s: env.grid(s)),
    "lidar": (LidarSpec(cells=8, sub=2, p_drop=0.25, sigma_r=0.5), lambda env, s: env.lidar(s)),
}


@pytest.fixture(scope="module")
def env():
    """the default config's env, one reset and one step in"""
    env = HighwayVecEnv(HIGHWAY_CONFIG, num_envs=E, device=DEV)
    env.reset(seed=42)
    env.step(torch.tensor([[0.3, -0.1], [-0.5, 0.2]], device=DEV))
    yield env
    env.close()


@pytest.mark.parametrize("name", list(SPECS))
def test_view_is_the_kinds_own_method_bit_for_bit(env, name):
    spec, own = SPECS[name]
    want = own(env, spec)
    width = env.view_width(spec)
    assert want.shape == (E, width) and bool(want.abs().sum() > 0)
    got = env.view(spec)
    assert got.shape == (E, width) and got.dtype == torch.float32
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    # into a caller's buffer, and through view_into into a slice of a larger one
    out = torch.full((E, width), -7.0, device=DEV)
    assert env.view(spec, out=out).data_ptr() == out.data_ptr()
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    states = torch.full((3, E, width), -7.0, device=DEV)
    env.view_into(spec, states[1])
    assert torch.equal(states[1].view(torch.int32), want.view(torch.int32))
    assert bool((states[0] == -7.0).all()) and bool((states[2] == -7.0).all())


def test_what_is_not_a_view_is_refused(env):
    for bad in (True, {}, None):
        with pytest.raises(ValueError, match="^a view is one of "):
            env.view(bad)
    with pytest.raises(ValueError, match="out must be a contiguous"):
        env.view_into(SPECS["grid"][0], torch.zeros(E, 7, device=DEV))
