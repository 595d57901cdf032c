"""visualize.py without a GPU: the condition and d_embed from a checkpoint's name, and the
network's dimensions from a checkpoint the test writes itself."""

import os

import pytest
import torch

import visualize
from experiments.config import Condition


@pytest.mark.parametrize("name, want", [
    ("ppo_highway_best_sorted_lr0.0003_hidden_dim256.pth", (Condition.SORTED, None)),
    ("ppo_highway_solved_shuffled_seed3.pth", (Condition.SHUFFLED, None)),
    ("ppo_highway_best_shuffled_rankpe_d_embed8_lr0.0001.pth", (Condition.SHUFFLED_RANKPE, 8)),
    ("ppo_highway_best_shuffled_distpe_lr0.0001_d_embed4.pth", (Condition.SHUFFLED_DISTPE, 4)),
    ("ppo_highway_solved_shuffled_rope_d_embed2.pth", (Condition.SHUFFLED_ROPE, 2)),
    ("shuffled_rope_d_embed4_run7.pth", (Condition.SHUFFLED_ROPE, 4)),  # not routine's naming
])
def test_condition_and_d_embed_from_the_name(name, want):
    assert visualize.parse_name(visualize.experiment_name(os.path.join("a", "b", name))) == want


@pytest.mark.parametrize("name", ["ppo_highway_best_shuffled_rope_lr0.1.pth",  # no d_embed
                                  "ppo_highway_best_baseline.pth"])             # no condition
def test_a_name_that_does_not_tell_is_refused(name):
    with pytest.raises(ValueError):
        visualize.parse_name(visualize.experiment_name(name))


def test_dimensions_from_a_saved_checkpoint(tmp_path):
    from ppo.agent import ActorCritic

    net = ActorCritic(15 * 9, 2, hidden_dim=96)
    path = tmp_path / "ppo_highway_best_shuffled_distpe_d_embed2.pth"
    torch.save({"model": net.state_dict()}, path)
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    assert visualize.infer_dims(ckpt["model"]) == (135, 96, 2)


def test_the_cli_needs_a_model(capsys):
    with pytest.raises(SystemExit):
        visualize.main([])
    with pytest.raises(SystemExit):
        visualize.main(["--model", "a.pth", "--models-file", "b.txt"])
