"""The shared base of the option records (SensorModel, GridSpec, LidarSpec, Shield) and the view
seam, without a device: what the four classes used to spell out one by one, the width a view's
rows have, and which run options are views."""

from __future__ import annotations

import json
import types

import pytest

from hwy import GridSpec, LidarSpec, SensorModel, Shield
from hwy.vec_env import VIEW_RECORDS, HighwayVecEnv
from ppo import options

# per class: a non-default value, its noun, whether True means the default
RECORDS = [
    (SensorModel(los=True, range=60.0, dropout=0.1, noise=(0.5, 0.25, 0.1), salt=3), "sensor",
     False),
    (GridSpec(layers=("presence", "vx", "on_road"), nx=7, ny=3, ranges={"vx": (-20, 30)},
              align=True, pad_to=8), "grid", True),
    (LidarSpec(cells=8, sub=2, p_drop=0.25, sigma_r=0.5, salt=9, ego_tail=False), "lidar", True),
    (Shield(horizon=5, fallbacks=((-1.0, 0.0), (0.5, -0.5)), lazy=False), "shield", False),
]
IDS = [type(r[0]).__name__ for r in RECORDS]


@pytest.mark.parametrize("x, noun, true_is_default", RECORDS, ids=IDS)
def test_a_record_survives_its_dict_and_json(x, noun, true_is_default):
    cls = type(x)
    back = cls.from_dict(json.loads(json.dumps(x.to_dict())))
    assert back == x and back is not x and hash(back) == hash(x)
    assert list(x.to_dict()) == list(cls.__slots__)
    assert cls.from_dict(x) is x
    assert cls.from_dict({}) == cls() != x
    assert x != x.to_dict() and x != object()
    assert eval(repr(x), {cls.__name__: cls}) == x  # Name(field=value, ...) over the slots
    assert cls.NOUN == noun and cls.TRUE_IS_DEFAULT is true_is_default


def test_repr_is_what_the_sensor_and_the_shield_printed_with_str():
    """their fields are bools, floats, None and tuples of floats, on which str and repr agree"""
    import sense_util as su

    for s in (SensorModel(), RECORDS[0][0], SensorModel(range=float("inf")), su.FULL, su.LOS):
        assert repr(s) == (f"SensorModel(los={s.los}, range={s.range}, dropout={s.dropout}, "
                           f"noise={s.noise}, salt={s.salt})")
    for sh in (Shield(), RECORDS[3][0], Shield(horizon=1, fallbacks=[(0, 1e-9)])):
        assert repr(sh) == f"Shield(horizon={sh.horizon}, fallbacks={sh.fallbacks}, lazy={sh.lazy})"


@pytest.mark.parametrize("x, noun, true_is_default", RECORDS, ids=IDS)
def test_a_record_is_immutable(x, noun, true_is_default):
    name = type(x).__name__
    for field in (type(x).__slots__[0], "anything"):
        with pytest.raises(AttributeError, match=f"^{name} is immutable$"):
            setattr(x, field, 1)
    assert not hasattr(x, "__dict__")


@pytest.mark.parametrize("x, noun, true_is_default", RECORDS, ids=IDS)
def test_what_from_dict_takes(x, noun, true_is_default):
    cls = type(x)
    if true_is_default:
        assert cls.from_dict(True) == cls()
        takes = f"a {noun} is a {cls.__name__}, True or a dict of its fields, got "
    else:
        takes = f"a {noun} is a {cls.__name__} or a dict of its fields, got "
        with pytest.raises(ValueError) as e:
            cls.from_dict(True)
        assert str(e.value) == takes + "True"
    for bad in (None, False, 1, "x", [("horizon", 3)]):
        with pytest.raises(ValueError) as e:
            cls.from_dict(bad)
        assert str(e.value) == takes + repr(bad)
    with pytest.raises(ValueError) as e:
        cls.from_dict({"zz": 1, cls.__slots__[0]: getattr(x, cls.__slots__[0]), "aa": 2})
    assert str(e.value) == f"unknown {noun} keys ['aa', 'zz']; known: {list(cls.__slots__)}"


def test_the_row_records_share_width_and_stride():
    for spec, payload in ((GridSpec(), 3 * 24 * 5), (LidarSpec(), 2 * 16),
                          (RECORDS[1][0], 3 * 7 * 3), (RECORDS[2][0], 2 * 8)):
        tail = 5 if spec.ego_tail else 0
        assert spec.payload == payload and spec.width(5) == payload + tail
        assert spec.stride(5) == -(-(payload + tail) // spec.pad_to) * spec.pad_to
    with pytest.raises(ValueError, match="^a grid row of 4100 floats is above hwy_grid's 4096$"):
        GridSpec(layers=("presence", "x", "y", "vx"), nx=32, ny=32).stride(1)
    assert LidarSpec(cells=1024).stride(8) == 2056  # the cap needs more features than an env has
    with pytest.raises(ValueError, match="^a lidar row of 4100 floats is above hwy_lidar's 4096$"):
        LidarSpec(cells=1024).stride(2049)


@pytest.mark.parametrize("N, F, Fo", [(5, 5, 5), (15, 7, 11)])
def test_view_width_is_the_stride_or_the_rows(N, F, Fo):
    env = types.SimpleNamespace(obs_rows=N, obs_features=Fo,
                                hwy_config=types.SimpleNamespace(n_features=F))
    for x, noun, _ in RECORDS[:3]:
        want = N * Fo if noun == "sensor" else x.stride(F)
        assert HighwayVecEnv.view_width(env, x) == want
        assert x.REPLACES_ROWS is (noun != "sensor")
    for not_a_view in (RECORDS[3][0], True, {}):
        with pytest.raises(ValueError, match="^a view is one of "):
            HighwayVecEnv.view_width(env, not_a_view)


def test_exactly_sensor_grid_and_lidar_are_views():
    assert options.VIEWS == ("sensor", "grid", "lidar") == tuple(VIEW_RECORDS)
    assert [o.name for o in options.OPTIONS if o.view] == list(options.VIEWS)
    for name, cls in VIEW_RECORDS.items():
        assert isinstance(options.BY_NAME[name].normalise({}), cls)


def test_the_given_view_of_every_single_option_value():
    values = {"episode_schedule": "reference", "episode_stats": True, "safety_stats": True,
              "truncation": "bootstrap", "attribution": True, "eval_orders": ["shuffled"],
              "eval_sensors": {"a": {}}, "sensor": {}, "eval_shields": {"a": None}, "shield": {},
              "grid": True, "lidar": True, "target_kl": 0.02, "lr_anneal_updates": 10}
    assert set(values) == set(options.BY_NAME)
    assert options.given_view({}) is None
    assert options.given_view({o.name: o.normalise(o.default) for o in options.OPTIONS}) is None
    for name, raw in values.items():
        v = options.BY_NAME[name].normalise(raw)
        got = options.given_view({name: v})
        if name in options.VIEWS:
            assert got == (name, v) and isinstance(v, VIEW_RECORDS[name])
        else:
            assert got is None
    for name in ("grid", "lidar"):
        assert options.given_view({name: options.BY_NAME[name].normalise(False)}) is None
