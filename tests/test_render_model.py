"""The render tests' float64 model (tests/render_model.py) against hand-counted scenes at scaling 8,
where pixel centres are odd multiples of 1/16 m and no edge ties with one: nothing is undecided.
Also the 1 % cap on undecided pixels for the crafted states the GPU tests feed the kernel, and the
facts the GPU tests rely on: the frame rule's table in include/hwy.h matches the model's
constants, and the feature exists in the library's Python surface."""

import os
import re

import numpy as np
import pytest

import render_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _render(state, env, W=64, H=32, **kw):
    view = dict(rm.SCENE_VIEW)
    view.update(kw)
    frame, und = rm.render(state, env, 4, W, H, **view)
    assert not und.any(), "a scaling-8 scene has no undecided pixel"
    return frame


def _is(frame, colour):
    return (frame == np.array(colour, dtype=np.uint8)).all(axis=-1)


def test_lone_car_at_heading_0_covers_40_by_16():
    f = _render(rm.scene_lone(), 0)
    ego = _is(f, rm.EGO)
    assert ego.sum() == 40 * 16
    rows, cols = np.where(ego)
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (8, 23, 12, 51)


def test_lone_car_at_half_pi_covers_16_by_40():
    f = _render(rm.scene_lone(), 1, W=64, H=48)
    ego = _is(f, rm.EGO)
    assert ego.sum() == 16 * 40
    rows, cols = np.where(ego)
    assert (rows.min(), rows.max(), cols.min(), cols.max()) == (4, 43, 24, 39)


def test_dashes_shift_by_8_px_per_metre():
    s = rm.scene_dash()
    a, b = _render(s, 0), _render(s, 1)
    # rows 0 and 31 are the dashed lines k = 1 and k = 2 (|py -+ 2| = 1/16 <= 0.15); row 1 is not
    for row in (0, 31):
        la, lb = _is(a, rm.LINE)[row], _is(b, rm.LINE)[row]
        assert la.any() and not la.all()
        assert np.array_equal(lb[:-8], la[8:])
        # xe = 100: phase 4, u = px + 4 in (0, 8): a dash where u < 3, i.e. px < -1: 24 columns
        assert la.sum() == 24 and la[:24].all()
    assert not _is(a, rm.LINE)[1].any()


def test_the_ego_paints_over_a_car_and_a_higher_index_over_a_lower():
    s = rm.scene_overlap()
    a, b = _render(s, 0), _render(s, 1)

    def at(f, px, py):  # the pixel whose centre is (px, py), both odd multiples of 1/16
        return tuple(int(v) for v in f[int(py * 8 + 16 - 0.5), int(px * 8 + 32 - 0.5)])

    mid = (1 / 16, 1 / 16)          # under the ego and both cars
    both = (3 + 1 / 16, 1 + 3 / 16)  # under cars 5 and 9, right of the ego
    only5 = (3 + 1 / 16, -5 / 16)    # under car 5 alone
    assert at(a, *mid) == rm.EGO and at(b, *mid) == rm.EGO
    assert at(a, *both) == rm.CRASHED  # env 0: 9 is the crashed one, and it is on top
    assert at(b, *both) == rm.VEHICLE  # env 1: 5 is crashed, 9 still on top
    assert at(a, *only5) == rm.VEHICLE and at(b, *only5) == rm.CRASHED


def test_crashed_absent_and_nan_vehicles():
    s = rm.scene_flags()
    a, b = _render(s, 0), _render(s, 1)
    assert _is(a, rm.CRASHED).sum() == 40 * 16          # the crashed ego
    assert _is(a, rm.VEHICLE).sum() == 0                # car 3 absent, car 4 at NaN
    # env 1: car 3 at +3 m covers px in [0.5, 4): 28 columns, 12 of them (px <= 2.5) under the ego
    assert _is(b, rm.VEHICLE).sum() == 12 * 16
    assert _is(b, rm.CRASHED).sum() == 40 * 16


def test_a_nan_ego_gives_an_all_background_frame():
    s = rm.scene_lone()
    rm.put(s, 0, 0, np.nan, 4.0)
    rm.put(s, 0, 7, 100.0, 4.0)
    assert _is(_render(s, 0), rm.BACKGROUND).all()
    assert _is(_render(s, 5), rm.BACKGROUND).all()  # an env id outside 0..E-1 as well


def test_luma_and_shade_endpoints():
    assert rm.luma((255, 255, 255)) == 255 and rm.luma((0, 0, 0)) == 0
    assert rm.luma(rm.EGO) == (77 * 50 + 150 * 200 + 128) >> 8
    for base in (rm.EGO, rm.VEHICLE, rm.CRASHED):
        assert rm.tint(base, 0.0) == base and rm.tint(base, 1.0) == rm.HOT
        assert rm.tint(base, -1.0) == base and rm.tint(base, 2.0) == rm.HOT
        assert rm.tint(base, np.nan) == base
        assert rm.tint(base, 0.5) == tuple((b * 128 + h * 128 + 128) >> 8
                                           for b, h in zip(base, rm.HOT))
    s = rm.scene_lone()
    shade = np.zeros((2, 64), dtype=np.float32)
    shade[0, 0] = 1.0
    f, _ = rm.render(s, 0, 4, 64, 32, shade=shade, **rm.SCENE_VIEW)
    assert _is(f, rm.HOT).sum() == 40 * 16
    g, _ = rm.render(s, 0, 4, 64, 32, channels=1, **rm.SCENE_VIEW)
    rgb = _render(s, 0)
    assert g.shape == (32, 64, 1)
    assert g[16, 32, 0] == rm.luma(rm.EGO) and g[0, 0, 0] == rm.luma(rgb[0, 0])


def test_ego_at_x_1_shows_background_left_of_the_road():
    s = rm.scene_road_start()
    a, b = _render(s, 0), _render(s, 1)
    # xe = 1: the road begins at px = -1, i.e. column 24; row 2 is clear of the ego and the lines
    assert _is(a, rm.BACKGROUND)[2, :24].all() and _is(a, rm.ROAD)[2, 24:].all()
    assert not _is(a, rm.LINE)[0, :24].any()  # lines only inside the road's x extent
    # xe = 9,999: the road ends at px = +1: columns 0..39
    assert _is(b, rm.ROAD)[2, :40].all() and _is(b, rm.BACKGROUND)[2, 40:].all()


@pytest.mark.parametrize("env", [0, 1])
def test_the_crafted_edge_state_keeps_the_undecided_share_under_1_percent(env):
    _, und = rm.render(rm.scene_edges(), env, 4, 600, 150)
    assert und.mean() <= 0.01


def _oracle_state(case):
    """The case's state on the CPU oracle (bit for bit the kernel's: tests/test_env_parity_gpu.py)."""
    import copy

    from config.base_config import HIGHWAY_CONFIG
    from hwy._abi import config_from_dict
    from oracle.oracle import OracleEnv

    _, E, _, overrides, _ = case
    cfg = copy.deepcopy(HIGHWAY_CONFIG)
    cfg.update(overrides)
    c = config_from_dict(cfg, num_envs=E, autoreset=False, seed_base=rm.SEED_BASE)
    ora = OracleEnv(c)
    ora.reset()
    for a in rm.natural_actions(case):
        ora.step(a)
    return ora.state.copy(), int(c.lanes_count)


@pytest.mark.parametrize("case", rm.NATURAL, ids=[c[0] for c in rm.NATURAL])
def test_the_natural_inputs_keep_the_undecided_share_under_1_percent(case):
    state, lanes = _oracle_state(case)
    for e in range(case[1]):
        _, und = rm.render(state, e, lanes, 600, 150)
        assert und.mean() <= 0.01, (case[0], e, und.sum())


def test_the_tail_inputs_keep_the_undecided_share_under_1_percent():
    state, lanes = _oracle_state(rm.TAILS)
    shade = rm.shade_values(3)
    for e in range(3):
        for W, H in rm.TAIL_SIZES:
            for cen in rm.TAIL_CENTERINGS:
                _, und = rm.render(state, e, lanes, W, H, centering=cen)
                assert und.mean() <= 0.01, (e, W, H, cen, und.sum())
        _, und = rm.render(state, e, lanes, 600, 150, shade=shade)
        assert und.mean() <= 0.01


def test_the_header_table_states_the_models_constants():
    text = open(os.path.join(ROOT, "include", "hwy.h")).read()
    for name in ("BACKGROUND", "ROAD", "LINE", "VEHICLE", "EGO", "CRASHED", "HOT"):
        m = re.search(r"\*\s+%s\s+\(\s*(\d+),\s*(\d+),\s*(\d+)\)" % name, text)
        assert m, name
        assert tuple(int(g) for g in m.groups()) == getattr(rm, name)
    assert re.search(r"LINE_HALF\s+0\.15 m", text) and re.search(r"DASH_ON\s+3 m of every 8", text)


def test_the_python_surface_names_the_feature():
    from experiments import wrappers
    from hwy.single_env import HighwayEnv
    from hwy.vec_env import HighwayVecEnv
    from training import routine

    assert HighwayEnv.metadata["render_modes"] == ["rgb_array"]
    assert callable(HighwayVecEnv.render) and callable(routine.visualize_agent)
    assert "render_mode" in wrappers._NATIVE_KEYS
    with pytest.raises(ValueError):
        HighwayEnv({}, render_mode="human")
