"""hwy_render on the GPU against the float64 model of the frame rule (tests/render_model.py): on
every decided pixel the kernel equals the model exactly, in all channels, and no frame has more
than 1 % undecided pixels (the scaling-8 scenes have none).  Then the store tails and bounds, the
env_ids, the shade, that nothing but the frames is written, graph capture, and the Python surface
(HighwayEnv.render, visualize_agent, visualize.py)."""

import copy
import os

import numpy as np
import pytest
import torch

import render_model as rm
from config.base_config import HIGHWAY_CONFIG

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DEFAULT_VIEW = dict(scaling=5.5, centering=(0.3, 0.5))
_MODEL = {}


def _vec(E, autoreset=False, **cfg_kw):
    from hwy.vec_env import HighwayVecEnv

    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(cfg_kw)
    return HighwayVecEnv(cfg, num_envs=E, device=DEV, autoreset=autoreset,
                         seed_base=rm.SEED_BASE)


def _state(env):
    return env.export_state().cpu().numpy().view(np.uint32)


def _model(state, e, lanes, W, H, C, view, shade=None):
    """render_model.render, computed once per input (the RGB frame; luma is derived from it)."""
    key = (state.tobytes(), e, lanes, W, H, view["scaling"], tuple(view["centering"]),
           None if shade is None else shade.tobytes())
    if key not in _MODEL:
        _MODEL[key] = rm.render(state, e, lanes, W, H, 3, view["scaling"], view["centering"], shade)
    rgb, und = _MODEL[key]
    if C == 1:
        r, g, b = (rgb[..., k].astype(np.int64) for k in range(3))
        return ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)[..., None], und
    return rgb, und


def check_frames(frames, state, ids, lanes, view, shade=None, cap=0.01, what=""):
    """frames [n, H, W, C] (numpy) against the model of env ids[i] of state, frame by frame."""
    n, H, W, C = frames.shape
    worst = 0.0
    for i, e in enumerate(ids):
        want, und = _model(state, int(e), lanes, W, H, C, view, shade)
        worst = max(worst, float(und.mean()))
        assert und.mean() <= cap, f"{what} frame {i}: {und.sum()} of {und.size} pixels undecided"
        bad = (frames[i] != want).any(axis=-1) & ~und
        assert not bad.any(), (f"{what} frame {i} (env {e}): {bad.sum()} decided pixels differ, "
                               f"first at {np.argwhere(bad)[0].tolist()}: kernel "
                               f"{frames[i][tuple(np.argwhere(bad)[0])]}, model "
                               f"{want[tuple(np.argwhere(bad)[0])]}")
    print(f"{what}: {n} frames {W}x{H}x{C} equal on every decided pixel; worst undecided share "
          f"{100 * worst:.3f} %")


# ------------------------------------------------------------------------------- 1. crafted scenes
@pytest.mark.parametrize("channels", [3, 1])
@pytest.mark.parametrize("scene", sorted(rm.SCENES))
def test_scaling_8_scenes_match_everywhere(scene, channels):
    env = _vec(2, scaling=8.0, centering_position=[0.5, 0.5])
    try:
        state = rm.SCENES[scene]()
        env.import_state(state)
        frames = env.render(width=64, height=32, channels=channels).cpu().numpy()
        check_frames(frames, state, [0, 1], 4, rm.SCENE_VIEW, cap=0.0, what=scene)
    finally:
        env.close()


# ------------------------------------------------------------------------------- 2. natural states
def _drive(env, case):
    """The case's env (render_model.NATURAL's recipe) reset and stepped with its actions."""
    env.reset()
    for a in rm.natural_actions(case):
        env.step(torch.as_tensor(a, device=DEV))


@pytest.mark.parametrize("case", rm.NATURAL, ids=[c[0] for c in rm.NATURAL])
def test_natural_states_match_the_model(case):
    name, E, _, cfg, _ = case
    env = _vec(E, **cfg)
    try:
        _drive(env, case)
        state = _state(env)
        for channels in (3, 1):
            frames = env.render(channels=channels).cpu().numpy()
            assert frames.shape == (E, 150, 600, channels)
            check_frames(frames, state, range(E), env.hwy_config.lanes_count, DEFAULT_VIEW,
                         what=name)
        rgb = env.render().cpu().numpy()
        # the pixel at 0.3 / 0.5 of the frame lies under the ego whatever its heading
        assert all(tuple(int(v) for v in rgb[e, 75, 180]) in (rm.EGO, rm.CRASHED)
                   for e in range(E)), "an ego is missing"
        if name == "default":
            assert (rgb == np.array(rm.VEHICLE, np.uint8)).all(-1).any(), "no other vehicle in view"
    finally:
        env.close()


# ------------------------------------------------------------------------------- 3. tails and bounds
@pytest.fixture(scope="module")
def env3():
    env = _vec(3)
    _drive(env, rm.TAILS)
    yield env, _state(env)
    env.close()


def _between_canaries(nbytes):
    buf = torch.full((256 + nbytes + 256,), 0xA5, dtype=torch.uint8, device=DEV)
    return buf, buf[256:256 + nbytes]


def _canaries_hold(buf, nbytes):
    host = buf.cpu().numpy()
    return bool((host[:256] == 0xA5).all() and (host[256 + nbytes:] == 0xA5).all())


@pytest.mark.parametrize("centering", rm.TAIL_CENTERINGS)
@pytest.mark.parametrize("channels", [1, 3])
@pytest.mark.parametrize("W, H", rm.TAIL_SIZES)
def test_store_tails_and_bounds(env3, W, H, channels, centering):
    env, state = env3
    old = env.config.get("centering_position")
    env.config["centering_position"] = list(centering)
    try:
        nbytes = 3 * H * W * channels
        buf, out = _between_canaries(nbytes)
        frames = env.render(width=W, height=H, channels=channels, out=out)
        assert frames.data_ptr() == out.data_ptr() and frames.shape == (3, H, W, channels)
        assert _canaries_hold(buf, nbytes)
        check_frames(frames.cpu().numpy(), state, range(3), 4,
                     dict(scaling=5.5, centering=centering), what=f"{W}x{H}x{channels}")
    finally:
        if old is None:
            del env.config["centering_position"]
        else:
            env.config["centering_position"] = old


# ------------------------------------------------------------------------------- 4. env_ids
@pytest.mark.parametrize("ids", [[2, 0, 1, 2, 0], [1], [2, 1]])
def test_env_ids_pick_the_frames_of_the_full_render(env3, ids):
    env, _ = env3
    full = env.render().cpu().numpy()
    t = torch.tensor(ids, dtype=torch.int32, device=DEV)
    for got in (env.render(t), env.render(ids)):  # a device tensor and a sequence
        got = got.cpu().numpy()
        assert got.shape[0] == len(ids)
        for i, e in enumerate(ids):
            assert np.array_equal(got[i], full[e]), (i, e)


@pytest.mark.parametrize("channels", [3, 1])
def test_an_env_id_out_of_range_gives_a_background_frame(env3, channels):
    env, _ = env3
    ids = torch.tensor([-1, 1, 3, 2 ** 31 - 1, -2 ** 31], dtype=torch.int32, device=DEV)
    nbytes = 5 * 150 * 600 * channels
    buf, out = _between_canaries(nbytes)
    got = env.render(ids, channels=channels, out=out).cpu().numpy()
    assert _canaries_hold(buf, nbytes)
    bg = np.array(rm.BACKGROUND if channels == 3 else [rm.luma(rm.BACKGROUND)], np.uint8)
    for i in (0, 2, 3, 4):
        assert (got[i] == bg).all(), i
    assert np.array_equal(got[1], env.render(channels=channels).cpu().numpy()[1])


# ------------------------------------------------------------------------------- 5. crafted edges
def test_crafted_edge_state_matches_the_model():
    env = _vec(2)
    try:
        for state in (rm.scene_edges(), rm.scene_road_start()):
            env.import_state(state)
            for channels in (3, 1):
                frames = env.render(channels=channels).cpu().numpy()
                check_frames(frames, state, [0, 1], 4, DEFAULT_VIEW, what="edges")
        rgb = env.render().cpu().numpy()  # scene_road_start: background beyond the road's ends
        assert (rgb[0, 5, :100] == np.array(rm.BACKGROUND, np.uint8)).all()
        assert (rgb[1, 5, -100:] == np.array(rm.BACKGROUND, np.uint8)).all()
    finally:
        env.close()


# ------------------------------------------------------------------------------- 6. shade
def test_shade_values_and_null_shade(env3):
    env, state = env3
    shade = rm.shade_values(3)
    for channels in (3, 1):
        got = env.render(channels=channels, shade=torch.as_tensor(shade, device=DEV))
        check_frames(got.cpu().numpy(), state, range(3), 4, DEFAULT_VIEW, shade=shade,
                     what="shade")
        zero = env.render(channels=channels, shade=torch.zeros(3, 64, device=DEV))
        assert torch.equal(zero, env.render(channels=channels))
    rgb = env.render(shade=torch.as_tensor(shade, device=DEV)).cpu().numpy()
    # the egos (the pixel at 0.3 / 0.5 of the frame): s = 1 gives HOT, 0.5 the midpoint, NaN the base
    for e, s in enumerate((1.0, 0.5, np.nan)):
        base = rm.CRASHED if state[rm.F_FLAGS, e, 0] & rm.FLAG_CRASHED else rm.EGO
        assert tuple(int(v) for v in rgb[e, 75, 180]) == rm.tint(base, s), (e, base)


# ------------------------------------------------------------------------------- 7. nothing else moves
def test_render_writes_nothing_but_the_frames():
    a, b = _vec(4, autoreset=True), _vec(4, autoreset=True)
    try:
        act = torch.as_tensor(np.random.default_rng(3).uniform(-0.3, 0.3, (2, 4, 2)).astype(np.float32),
                              device=DEV)
        outs = []
        for env, render in ((a, True), (b, False)):
            env.reset()
            env.step(act[0])
            if render:
                before = env.export_state().clone()
                env.render()
                env.render(channels=1, width=64, height=128)
                assert torch.equal(before, env.export_state())
            o = env.step(act[1])
            outs.append([t.clone() for t in o[:4]] + [env.export_state()])
        for x, y in zip(*outs):
            assert torch.equal(x, y)
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------- 8. graph capture
def test_captured_render_replays_on_the_later_state():
    from utils.graphs import capture

    env = _vec(4)
    try:
        _drive(env, rm.NATURAL[0])
        out = torch.zeros(4, 150, 600, 3, dtype=torch.uint8, device=DEV)
        env.render(out=out)  # eager first: the code object is loaded outside the capture
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            with capture(g, stream=s):
                env.render(out=out)
        torch.cuda.current_stream().wait_stream(s)
        first = out.clone()
        env.step(torch.full((4, 2), 0.2, device=DEV))
        out.zero_()
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, env.render())
        assert not torch.equal(out, first)
    finally:
        env.close()


# ------------------------------------------------------------------------------- 9. Python surface
def test_one_env_facade_render_modes():
    from experiments.config import Condition
    from experiments.wrappers import make_env
    from hwy.single_env import HighwayEnv

    env = make_env(Condition.SORTED, HIGHWAY_CONFIG, env_overrides={"render_mode": "rgb_array"})
    try:
        assert env.metadata["render_modes"] == ["rgb_array"] and env.render_mode == "rgb_array"
        env.reset(seed=5)
        env.step(np.array([0.1, 0.0], np.float32))
        frame = env.render()
        assert isinstance(frame, np.ndarray) and frame.shape == (150, 600, 3)
        assert frame.dtype == np.uint8
        assert np.array_equal(frame, env.vec_env.render()[0].cpu().numpy())
    finally:
        env.close()
    plain = HighwayEnv(HIGHWAY_CONFIG)
    try:
        plain.reset(seed=5)
        assert plain.render() is None
    finally:
        plain.close()
    with pytest.raises(ValueError):
        HighwayEnv(HIGHWAY_CONFIG, render_mode="human")


def test_bad_render_arguments_raise_value_error(env3):
    env, _ = env3
    for kw in (dict(width=0), dict(height=4097), dict(channels=2),
               dict(out=torch.zeros(7, dtype=torch.uint8, device=DEV)),
               dict(shade=torch.zeros(5, device=DEV)),
               dict(envs=torch.zeros(2, dtype=torch.int64, device=DEV))):
        with pytest.raises(ValueError):
            env.render(**kw)
    buf = torch.zeros(3 * 150 * 600 * 3 + 16, dtype=torch.uint8, device=DEV)
    with pytest.raises(ValueError):  # off the 16-byte alignment
        env.render(out=buf[1:1 + 3 * 150 * 600 * 3])


HORIZON, EXP_SEED = 6, 42


def _small_config():
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(max_episode_steps=HORIZON, screen_width=96, screen_height=32)
    return cfg


def _agent(seed=0):
    from ppo.agent import PPOAgent

    torch.manual_seed(seed)
    return PPOAgent(60, 2, hidden_dim=64, device=DEV)


def _eval_loop(cfg, agent, n, base_seed):
    """evaluate()'s loop, per episode: the float64 sums of the rewards and the lengths."""
    from hwy.vec_env import HighwayVecEnv

    ev = HighwayVecEnv(cfg, num_envs=n, device=DEV, autoreset=False)
    try:
        obs, _ = ev.reset(seeds=torch.arange(n, device=DEV, dtype=torch.int64) + base_seed)
        alive = torch.ones(n, dtype=torch.bool, device=DEV)
        total = torch.zeros(n, dtype=torch.float64, device=DEV)
        length = torch.zeros(n, dtype=torch.int64, device=DEV)
        for _ in range(ev.max_episode_steps + 1):
            a, _, _, _ = agent.select_action(obs.reshape(n, -1), deterministic=True)
            obs, r, te, tr, _ = ev.step(a.contiguous())
            total += torch.where(alive, r.double(), torch.zeros_like(total))
            length += alive.long()
            alive &= ~(te.bool() | tr.bool())
        return total.cpu().tolist(), length.cpu().tolist()
    finally:
        ev.close()


def test_visualize_agent_writes_each_episodes_frames(tmp_path):
    from hwy.vec_env import HighwayVecEnv
    from training.routine import visualize_agent

    cfg, agent, n = _small_config(), _agent(), 3
    env = HighwayVecEnv(cfg, num_envs=2, device=DEV)
    try:
        want, lengths = _eval_loop(cfg, agent, n, EXP_SEED + 2000)
        runs = []
        for k in range(2):
            out_dir = str(tmp_path / f"run{k}")
            rewards = visualize_agent(env, agent, num_episodes=n, exp_seed=EXP_SEED,
                                      out_dir=out_dir)
            assert rewards == want
            frames = [np.load(os.path.join(out_dir, f"viz_episode_{ep + 1}.npy"))
                      for ep in range(n)]
            for f, T in zip(frames, lengths):
                assert f.shape == (T + 1, 32, 96, 3) and f.dtype == np.uint8
                assert (f[0] != f[-1]).any()
            runs.append(frames)
        for x, y in zip(*runs):
            assert np.array_equal(x, y)
        assert visualize_agent(env, agent, num_episodes=n, exp_seed=EXP_SEED) == want
        assert not (tmp_path / "run2").exists()
    finally:
        env.close()


def test_visualize_cli_records_a_saved_checkpoint(tmp_path):
    import visualize

    agent = _agent(1)
    path = str(tmp_path / "ppo_highway_best_sorted_lr0.0003_hidden_dim64.pth")
    agent.save(path)
    out = tmp_path / "frames"
    assert visualize.main(["--model", path, "--episodes", "2", "--out", str(out)]) == 0
    dest = out / "ppo_highway_best_sorted_lr0.0003_hidden_dim64"
    for ep in (1, 2):
        f = np.load(dest / f"viz_episode_{ep}.npy")
        assert f.ndim == 4 and f.shape[1:] == (150, 600, 3) and f.shape[0] >= 2
