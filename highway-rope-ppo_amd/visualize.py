"""Record episodes of trained checkpoints as frames (the reference's visualize.py role).

    python visualize.py --model artifacts/highway-ppo/checkpoints/ppo_highway_best_<exp>.pth \
        --episodes 3 --out demo_frames
    python visualize.py --models-file best_checkpoints.txt --out demo_frames
    python visualize.py --model <checkpoint> --attribution value     # what the critic looks at
    python visualize.py --model <checkpoint> --tint ttc              # who is about to be hit
    python visualize.py --model <checkpoint> --tint hidden --sensor '{"los": true, "range": 80}'
    python visualize.py --model <checkpoint> --grid true              # a grid-trained checkpoint
    python visualize.py --model <checkpoint> --lidar true --tint lidar   # a lidar-trained one

For every checkpoint the network's dimensions are read from the saved weights
(``shared.0.weight`` is [hidden_dim, state_dim], ``actor_mean.2.weight`` [action_dim,
hidden_dim]), the condition and ``d_embed`` from the checkpoint's name
(``ppo_highway_{best,solved}_<experiment name>.pth``: the name begins with the condition and a
positional-embedding condition carries ``_d_embed<k>``), the condition's env is rebuilt with
``make_env`` and ``--episodes`` deterministic episodes are recorded with
training.routine.visualize_agent into ``--out/<checkpoint stem>/``: per episode a ``.npy`` of
[T + 1, H, W, 3] uint8 frames, and an animated GIF when PIL is importable.  The frames are drawn
on the GPU by hwy_render (include/hwy.h: this project's frame rule at upstream's view geometry,
not pygame's pixels).  ``--attribution`` tints every vehicle toward yellow by the share of the
chosen output's input-gradient mass on the observation row that shows it (hwy_observe's row ->
vehicle map; training.routine.attribution_shade); ``--tint ttc`` tints them by their
time-to-collision risk instead (hwy_traffic's ``risk``: 1 - ttc / 4 s below 4 s), and the two
exclude each other.  ``--sensor JSON`` (hwy.SensorModel's fields) lets the policy act on what that
sensor perceives (hwy_sense), and ``--tint hidden`` with it tints the vehicles the sensor does not
see.  ``--grid JSON`` (hwy.GridSpec's fields, or ``true`` for the default) lets a checkpoint
trained on the occupancy grid (hwy_grid) drive the episodes: its input width is checked against
the spec's stride.  ``--lidar JSON`` (hwy.LidarSpec's fields, or ``true``) does the same for a
checkpoint trained on the ray-cast range observation (hwy_lidar), and ``--tint lidar`` with it
tints the vehicles the lidar returns.  There is no live window and no MP4: neither a display nor
an encoder is a dependency.
"""

from __future__ import annotations

import argparse
import os
import re
import sys
from typing import Iterable, List, Optional, Tuple

_HERE = os.path.dirname(os.path.abspath(__file__))
if _HERE not in sys.path:
    sys.path.insert(0, _HERE)

from experiments.config import Condition  # noqa: E402
from ppo.options import VIEWS, given  # noqa: E402
from training.routine import TINT_NEEDS  # noqa: E402

CHECKPOINT_RE = re.compile(r"^ppo_highway_(?:best|solved)_(?P<exp>.+)\.pth$")
# longest prefix first: every positional-embedding condition's name begins with "shuffled"
_PREFIXES = (("shuffled_rankpe", Condition.SHUFFLED_RANKPE),
             ("shuffled_distpe", Condition.SHUFFLED_DISTPE),
             ("shuffled_rope", Condition.SHUFFLED_ROPE),
             ("shuffled", Condition.SHUFFLED),
             ("sorted", Condition.SORTED))
_PE_CONDITIONS = (Condition.SHUFFLED_RANKPE, Condition.SHUFFLED_DISTPE, Condition.SHUFFLED_ROPE)


def experiment_name(path: str) -> str:
    """The experiment name inside a checkpoint's file name (the bare stem when the file is not
    named as training/routine.py names its checkpoints)."""
    base = os.path.basename(path)
    m = CHECKPOINT_RE.match(base)
    return m.group("exp") if m else os.path.splitext(base)[0]


def parse_name(exp_name: str) -> Tuple[Condition, Optional[int]]:
    """(condition, d_embed) of an experiment name; d_embed is None for the conditions without a
    positional embedding.  ValueError when the name tells neither."""
    low = exp_name.lower()
    cond = next((c for prefix, c in _PREFIXES if low.startswith(prefix)), None)
    if cond is None:
        raise ValueError(f"cannot infer the condition from experiment name {exp_name!r}")
    if cond not in _PE_CONDITIONS:
        return cond, None
    m = re.search(r"_d_embed(\d+)", low)
    if not m:
        raise ValueError(f"cannot parse d_embed from experiment name {exp_name!r}")
    return cond, int(m.group(1))


def infer_dims(state_dict) -> Tuple[int, int, int]:
    """(state_dim, hidden_dim, action_dim) of a saved ActorCritic."""
    hidden_dim, state_dim = state_dict["shared.0.weight"].shape
    action_dim = state_dict["actor_mean.2.weight"].shape[0]
    return int(state_dim), int(hidden_dim), int(action_dim)


def load_agent(path: str, device=None):
    """A PPOAgent of the checkpoint's dimensions holding its weights, on ``device``."""
    import torch

    from ppo.agent import PPOAgent

    if device is None:
        device = torch.device("cuda", torch.cuda.current_device())
    ckpt = torch.load(path, map_location="cpu", weights_only=True)
    state_dim, hidden_dim, action_dim = infer_dims(ckpt["model"])
    agent = PPOAgent(state_dim, action_dim, hidden_dim=hidden_dim, device=torch.device(device))
    agent.load(path, load_optimizer=False)
    agent.actor_critic.eval()
    return agent


def record(path: str, out_dir: str, episodes: int = 1, seed: int = 0, device=None,
           attribution: Optional[str] = None, tint: Optional[str] = None,
           sensor=None, grid=None, lidar=None) -> List[float]:
    """Record ``episodes`` episodes of one checkpoint into out_dir/<checkpoint stem>/; returns
    their rewards.  ``attribution`` ("acceleration", "steering" or "value"): tint every vehicle by
    the policy's input-gradient mass on the row that shows it (visualize_agent).  ``tint``
    ("ttc"): tint them by their time-to-collision risk instead; not together with it.  ``sensor``
    (a hwy.SensorModel or its dict): the policy acts on what it perceives, and ``tint`` "hidden"
    tints the vehicles it does not see.  ``grid`` / ``lidar`` (a hwy.GridSpec / hwy.LidarSpec, its
    dict, or True): the policy acts on the occupancy grid / the ray-cast range observation of the
    states, as a checkpoint trained on it expects; not with another view or ``attribution``;
    ``tint`` "lidar" tints the vehicles the lidar returns."""
    if tint is not None and attribution is not None:
        raise ValueError("tint and attribution both shade the vehicles: give one of them")
    from hwy.vec_env import VIEW_RECORDS

    views = dict(sensor=sensor, grid=grid, lidar=lidar)
    for i, name in enumerate(VIEWS):  # each refuses the views before it; a tint needs its view
        before = VIEWS[:i]
        if views[name] is None:
            if TINT_NEEDS.get(tint) == name:
                raise ValueError(f'tint "{tint}" needs a {name}')
            continue
        views[name] = VIEW_RECORDS[name].from_dict(views[name])
        if before and (attribution is not None or any(views[b] is not None for b in before)):
            raise ValueError(f"{name} does not go with {', '.join(before)} or attribution")
    from config.base_config import HIGHWAY_CONFIG
    from experiments.wrappers import make_env
    from training.routine import visualize_agent

    cond, d_embed = parse_name(experiment_name(path))
    agent = load_agent(path, device=device)
    env = make_env(cond, HIGHWAY_CONFIG, d_embed=d_embed,
                   env_overrides={"vector_env": True, "device": agent.device})
    try:
        have = int(env.observation_space.shape[0] * env.observation_space.shape[1])
        own = next((v for v in views.values() if v is not None and v.REPLACES_ROWS), None)
        if own is not None:  # the policy's input is the view's row
            have = env.unwrapped.view_width(own)
        want = infer_dims(agent.actor_critic.state_dict())[0]
        if have != want:
            raise ValueError(f"{os.path.basename(path)}: the checkpoint takes {want} inputs, the "
                             f"{cond.name} env (d_embed={d_embed}) gives {have}")
        dest = os.path.join(out_dir, os.path.splitext(os.path.basename(path))[0])
        rewards = visualize_agent(env, agent, num_episodes=episodes, exp_seed=seed, out_dir=dest,
                                  attribution=attribution,
                                  **given(tint=tint or None, **views))
    finally:
        env.close()
    for ep, r in enumerate(rewards):
        print(f"{os.path.basename(path)} episode {ep + 1}/{len(rewards)} reward={r:.2f}")
    print(f"frames written to {dest}")
    return rewards


def models_from_file(path: str) -> Iterable[str]:
    with open(path) as f:
        for line in f:
            if line.strip():
                yield line.strip()


def main(argv=None) -> int:
    p = argparse.ArgumentParser(description="Record episodes of trained PPO checkpoints.")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--model", help="one .pth checkpoint")
    g.add_argument("--models-file", help="text file with one checkpoint path per line")
    p.add_argument("--episodes", type=int, default=1)
    p.add_argument("--out", default="demo_frames", help="directory for the recordings")
    p.add_argument("--seed", type=int, default=0,
                   help="episode ep is seeded seed + 2000 + ep, as visualize_agent")
    p.add_argument("--attribution", choices=("acceleration", "steering", "value"), default=None,
                   help="tint each vehicle by |input gradient| of this output on its row")
    p.add_argument("--tint", choices=("ttc", "hidden", "lidar"), default=None,
                   help="tint each vehicle by its time-to-collision risk, or (hidden, with "
                        "--sensor) the vehicles the sensor does not see (not with --attribution)")
    p.add_argument("--sensor", default=None, metavar="JSON",
                   help='the policy acts through this sensor, e.g. \'{"los": true, "range": 80, '
                        '"dropout": 0.1, "noise": [0.5, 0.2, 0.5]}\'')
    p.add_argument("--grid", default=None, metavar="JSON",
                   help="the policy acts on this occupancy grid (a grid-trained checkpoint), e.g. "
                        '\'{"nx": 24, "ny": 5, "align": true}\', or true for the default grid')
    p.add_argument("--lidar", default=None, metavar="JSON",
                   help="the policy acts on this lidar (a lidar-trained checkpoint), e.g. "
                        '\'{"cells": 64, "align": true}\', or true for the default lidar; '
                        "--tint lidar tints the vehicles it returns")
    args = p.parse_args(argv)
    if args.tint and args.attribution:
        p.error("--tint and --attribution both shade the vehicles: give one of them")
    import json

    from hwy.vec_env import VIEW_RECORDS

    views = {}
    for i, name in enumerate(VIEWS):  # each refuses the views before it; a tint needs its view
        raw, before = getattr(args, name), VIEWS[:i]
        if raw is None:
            if TINT_NEEDS.get(args.tint) == name:
                p.error(f"--tint {args.tint} needs --{name}")
            continue
        try:
            views[name] = VIEW_RECORDS[name].from_dict(json.loads(raw))
        except ValueError as e:   # json.JSONDecodeError is a ValueError too
            p.error(f"--{name}: {e}")
        if before and (args.attribution or any(b in views for b in before)):
            p.error(f"--{name} does not go with {', '.join('--' + b for b in before)} or "
                    "--attribution")
    models = [args.model] if args.model else list(models_from_file(args.models_file))
    for m in models:
        record(m, args.out, episodes=args.episodes, seed=args.seed, attribution=args.attribution,
               tint=args.tint, **views)
    return 0


if __name__ == "__main__":
    sys.exit(main())
