"""ctypes mirror of include/hwy.h and the HIGHWAY_CONFIG -> hwy_config translation.

The translation restates how highway-env 1.10.1 reads the reference's config dict
(config/base_config.py:5-39) after ``make_env``'s deep merge (experiments/wrappers.py:33-57):
the ``observation`` block configures KinematicObservation, the top-level keys configure
HighwayEnv / AbstractEnv.  This module holds no device code and is safe to import anywhere.
"""

from __future__ import annotations

import ctypes
import math
from typing import Any, Dict, Optional

HWY_ABI_VERSION = 1
HWY_MAX_VEHICLES = 64
HWY_MAX_FEATURES = 8
HWY_MAX_OBS_ROWS = 64
HWY_MAX_FOUT = 64

FEATURES = {
    "presence": 0,
    "x": 1,
    "y": 2,
    "vx": 3,
    "vy": 4,
    "cos_h": 5,
    "sin_h": 6,
    "heading": 7,
}
ORDER_SORTED, ORDER_SHUFFLED = 0, 1
PE_NONE, PE_RANK, PE_DIST, PE_ROPE, PE_DIST1 = 0, 1, 2, 3, 4
PE_APPENDS = (PE_RANK, PE_DIST, PE_DIST1)  # kinds that append d columns

# enum hwy_field / hwy_env_word
F_X, F_Y, F_HEADING, F_SPEED, F_TSPEED, F_DELTA, F_TIMER, F_IMPX, F_IMPY = range(9)
F_LANE, F_TLANE, F_FLAGS, F_ENV = 9, 10, 11, 12
NFIELDS = 13
E_STEP, E_EPISODE, E_SEED_LO, E_SEED_HI, E_EGO_ACC, E_EGO_STEER, E_RETURN = range(7)
FLAG_CRASHED, FLAG_IMPACT, FLAG_PRESENT = 1, 2, 4
FLAG_ORDER_SHIFT = 8  # bits 8-13: road-order position (include/hwy.h)
FLOAT_FIELDS = (F_X, F_Y, F_HEADING, F_SPEED, F_TSPEED, F_DELTA, F_TIMER, F_IMPX, F_IMPY)

# Episode horizon in policy steps.  highway-env 1.10.1 truncates on env.time >= duration; the
# reference's own artifacts show an untruncated episode is ~200 policy steps (SURVEY.md §6.4:
# 201-frame demo videos, ~170 mean steps/episode, eval returns up to 144 with per-step reward
# <= 1), which a 40-step reading of duration=40 @ 1 Hz cannot produce.  Default: 5 policy steps
# per second of "duration"; override with the "max_episode_steps" config key.
DEFAULT_STEPS_PER_DURATION = 5


# hwy_step_with_info (include/hwy.h): floats per env of the episode sums, their slots, and the
# keys of upstream's info["rewards"] (HighwayEnv._rewards) in the order of the rewards output
HWY_INFO_NACC = 8
(ACC_SPEED, ACC_COLLISION, ACC_RIGHT_LANE, ACC_HIGH_SPEED, ACC_ON_ROAD, ACC_LANE_CHANGES,
 ACC_CRASHED) = range(7)
REWARD_KEYS = ("collision_reward", "right_lane_reward", "high_speed_reward", "on_road_reward")


class HwyStepInfo(ctypes.Structure):
    """hwy_step_info: the info outputs of one handle's step (device pointers, all nullable)."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("speed", "crashed", "lane", "rewards", "acc",
                                               "ep_stats")]


class RenderArgs(ctypes.Structure):
    """hwy_render_args (include/hwy.h): one hwy_render launch's view, frame list and buffers."""
    _fields_ = [
        ("width", ctypes.c_int32),
        ("height", ctypes.c_int32),
        ("channels", ctypes.c_int32),
        ("n", ctypes.c_int32),
        ("scaling", ctypes.c_float),
        ("centering", ctypes.c_float * 2),
        ("env_ids", ctypes.c_void_p),
        ("shade", ctypes.c_void_p),
        ("frames", ctypes.c_void_p),
    ]


class ObserveArgs(ctypes.Structure):
    """hwy_observe_args (include/hwy.h): one hwy_observe launch's order override and outputs."""
    _fields_ = [
        ("order", ctypes.c_int32),
        ("obs", ctypes.c_void_p),
        ("row_vehicle", ctypes.c_void_p),
        ("row_values", ctypes.c_void_p),
        ("veh_values", ctypes.c_void_p),
    ]


# hwy_traffic (include/hwy.h): floats per env of the ego row and of the running reduction, their
# slots, and the defaults of the four thresholds (seconds, seconds, seconds, metres)
HWY_TRAFFIC_NEGO = 16
HWY_TRAFFIC_NACC = 8
(EGO_GAP, EGO_CLOSING, EGO_TTC, EGO_THW, EGO_REAR_GAP, EGO_REAR_CLOSING, EGO_REAR_TTC,
 EGO_LEFT_FRONT_GAP, EGO_LEFT_REAR_GAP, EGO_RIGHT_FRONT_GAP, EGO_RIGHT_REAR_GAP, EGO_MIN_DISTANCE,
 EGO_NEAR_COUNT, EGO_LANE_OFFSET, EGO_VX, EGO_RISK) = range(16)
(TACC_N, TACC_MIN_TTC, TACC_MIN_THW, TACC_MIN_GAP, TACC_MIN_DISTANCE, TACC_TTC_CRITICAL,
 TACC_TAILGATING, TACC_WITH_FRONT) = range(8)
TRAFFIC_VEHICLE_OUTPUTS = ("front", "rear", "gap", "closing", "ttc", "thw", "risk")
TRAFFIC_DEFAULTS = {"ttc_thresh": 2.0, "thw_thresh": 1.0, "risk_horizon": 4.0, "near_range": 50.0}


class TrafficArgs(ctypes.Structure):
    """hwy_traffic_args (include/hwy.h): one hwy_traffic launch's outputs, masks and thresholds."""
    _fields_ = [(n, ctypes.c_void_p) for n in TRAFFIC_VEHICLE_OUTPUTS + ("ego", "acc", "ep_stats")] + [
        ("restart", ctypes.c_void_p * 3),
        ("ttc_thresh", ctypes.c_float),
        ("thw_thresh", ctypes.c_float),
        ("risk_horizon", ctypes.c_float),
        ("near_range", ctypes.c_float),
    ]


# hwy_observe's `order`: None = the handle's own (-1)
OBSERVE_ORDERS = {None: -1, "sorted": 0, "shuffled": 1}


def observe_order(order) -> int:
    """hwy_observe_args.order of ``order`` (None, "sorted" or "shuffled")."""
    try:
        return OBSERVE_ORDERS[order]
    except (KeyError, TypeError):
        raise ValueError(f"order must be None, 'sorted' or 'shuffled', got {order!r}") from None


class _Record:
    """What the option records (SensorModel, GridSpec, LidarSpec, Shield) share: immutable,
    hashable values over the fields of ``__slots__``, JSON-ready through to_dict / from_dict.
    ``NOUN`` is what the messages call the record, and its run option's name in ppo/options.py;
    ``TRUE_IS_DEFAULT``: from_dict(True) is the default record; ``REPLACES_ROWS`` (of a view,
    HighwayVecEnv.view_into): what it writes stands in place of the step's Kinematics rows, with
    a width of its own, instead of overwriting them."""

    __slots__ = ()
    NOUN = ""
    TRUE_IS_DEFAULT = False
    REPLACES_ROWS = False

    def _init(self, **fields):
        for name, v in fields.items():
            object.__setattr__(self, name, v)

    def __setattr__(self, name, value):
        raise AttributeError(f"{type(self).__name__} is immutable")

    def _key(self):
        return tuple(getattr(self, n) for n in self.__slots__)

    def __eq__(self, other):
        return isinstance(other, type(self)) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        fields = ", ".join(f"{n}={getattr(self, n)!r}" for n in self.__slots__)
        return f"{type(self).__name__}({fields})"

    def _json_fields(self) -> Dict[str, Any]:
        """The fields whose JSON form is not the value itself (tuples as lists or dicts)."""
        return {}

    def to_dict(self) -> Dict[str, Any]:
        """JSON-ready (the metrics file)."""
        d = {n: getattr(self, n) for n in self.__slots__}
        d.update(self._json_fields())
        return d

    @classmethod
    def from_dict(cls, d):
        """A record from ``to_dict``'s form (missing keys: the defaults), ``d`` itself when it
        already is one, the default for True where the class takes it; unknown keys are a
        ValueError."""
        if isinstance(d, cls):
            return d
        if d is True and cls.TRUE_IS_DEFAULT:
            return cls()
        if not isinstance(d, dict):
            raise ValueError(f"a {cls.NOUN} is a {cls.__name__}"
                             f"{', True' if cls.TRUE_IS_DEFAULT else ''} or a dict of its fields, "
                             f"got {d!r}")
        unknown = set(d) - set(cls.__slots__)
        if unknown:
            raise ValueError(f"unknown {cls.NOUN} keys {sorted(unknown)}; known: "
                             f"{list(cls.__slots__)}")
        return cls(**d)


class _RowSpec(_Record):
    """A record of an observation that is one padded float32 row per env (GridSpec, LidarSpec):
    ``payload`` floats, the ego's own Kinematics row with ``ego_tail``, zeros up to a multiple of
    ``pad_to``, at most ``MAX_STRIDE`` floats (hwy_<NOUN>'s cap)."""

    __slots__ = ()
    TRUE_IS_DEFAULT = True
    REPLACES_ROWS = True
    MAX_STRIDE = 0

    def width(self, n_features: int) -> int:
        """Floats of a row that carry something: the payload and, with ``ego_tail``, the F values
        of the ego's Kinematics row."""
        return self.payload + (int(n_features) if self.ego_tail else 0)

    def stride(self, n_features: int) -> int:
        """Floats per env: ``width`` rounded up to a multiple of ``pad_to``."""
        w = self.width(n_features)
        s = -(-w // self.pad_to) * self.pad_to
        if s > self.MAX_STRIDE:
            raise ValueError(f"a {self.NOUN} row of {s} floats is above hwy_{self.NOUN}'s "
                             f"{self.MAX_STRIDE}")
        return s


class SenseArgs(ctypes.Structure):
    """hwy_sense_args (include/hwy.h): one hwy_sense launch's order, sensor and outputs."""
    _fields_ = [
        ("order", ctypes.c_int32),
        ("los", ctypes.c_int32),
        ("range_m", ctypes.c_float),
        ("p_drop", ctypes.c_float),
        ("sigma", ctypes.c_float * 3),
        ("salt", ctypes.c_int32),
        ("obs", ctypes.c_void_p),
        ("row_vehicle", ctypes.c_void_p),
        ("visible", ctypes.c_void_p),
        ("hidden", ctypes.c_void_p),
        ("counts", ctypes.c_void_p),
    ]


SENSE_OUTPUTS = ("obs", "row_vehicle", "visible", "hidden", "counts")
HWY_SENSE_SALT = 0x53454E53


class SensorModel(_Record):
    """The sensor of hwy_sense (include/hwy.h), an immutable, hashable value.

    ``los``: line-of-sight occlusion by the other vehicles' bodies; ``range``: sensing range in
    metres (None: unlimited); ``dropout``: probability of a missed detection per vehicle and
    step, in [0, 1]; ``noise``: the standard deviations of the perceived x (m), y (m) and speed
    (m/s); ``salt``: 0..65535, selects the stream of the draws.  Everything hwy_sense_check
    refuses is a ValueError here."""

    __slots__ = ("los", "range", "dropout", "noise", "salt")
    NOUN = "sensor"

    def __init__(self, los: bool = False, range: Optional[float] = None, dropout: float = 0.0,
                 noise=(0, 0, 0), salt: int = 0):
        try:
            rng = None if range is None else float(range)
            drop = float(dropout)
            sig = tuple(float(s) for s in noise)
            slt = int(salt)
        except (TypeError, ValueError):
            raise ValueError(f"bad sensor fields: range={range!r} dropout={dropout!r} "
                             f"noise={noise!r} salt={salt!r}") from None
        if rng is not None and math.isinf(rng) and rng > 0:
            rng = None
        if rng is not None and not (rng > 0.0 and math.isfinite(rng)):
            raise ValueError(f"range must be None (unlimited) or finite and > 0, got {range!r}")
        if not 0.0 <= drop <= 1.0:
            raise ValueError(f"dropout must lie in [0, 1], got {dropout!r}")
        if len(sig) != 3 or not all(s >= 0.0 and math.isfinite(s) for s in sig):
            raise ValueError(f"noise must be three finite values >= 0 (x, y, speed), got {noise!r}")
        if slt != salt or not 0 <= slt <= 65535:
            raise ValueError(f"salt must be an integer in 0..65535, got {salt!r}")
        self._init(los=bool(los), range=rng, dropout=drop, noise=sig, salt=slt)

    @property
    def is_null(self) -> bool:
        """No occlusion, no range limit, no dropout and no noise: hwy_sense is hwy_observe."""
        return (not self.los and self.range is None and self.dropout == 0.0
                and self.noise == (0.0, 0.0, 0.0))

    def _json_fields(self):  # range None = unlimited
        return {"noise": list(self.noise)}

    def fill(self, a: SenseArgs) -> SenseArgs:
        """Write the sensor's fields into hwy_sense_args ``a``."""
        a.los = int(self.los)
        a.range_m = math.inf if self.range is None else self.range
        a.p_drop = self.dropout
        for c in range(3):
            a.sigma[c] = self.noise[c]
        a.salt = self.salt
        return a


class GridArgs(ctypes.Structure):
    """hwy_grid_args (include/hwy.h): one hwy_grid launch's geometry, layers and outputs."""
    _fields_ = [
        ("nx", ctypes.c_int32),
        ("ny", ctypes.c_int32),
        ("x0", ctypes.c_float),
        ("y0", ctypes.c_float),
        ("step_x", ctypes.c_float),
        ("step_y", ctypes.c_float),
        ("align", ctypes.c_int32),
        ("n_layers", ctypes.c_int32),
        ("layer_ids", ctypes.c_int32 * 8),
        ("has_range", ctypes.c_int32 * 8),
        ("range", (ctypes.c_float * 2) * 8),
        ("clip", ctypes.c_int32),
        ("ego_tail", ctypes.c_int32),
        ("row_stride", ctypes.c_int32),
        ("grid", ctypes.c_void_p),
        ("cell_vehicle", ctypes.c_void_p),
        ("veh_cell", ctypes.c_void_p),
        ("counts", ctypes.c_void_p),
    ]


GRID_OUTPUTS = ("grid", "cell_vehicle", "veh_cell", "counts")
GRID_ON_ROAD = 8
GRID_MAX_LAYERS = 8
GRID_MAX_CELLS = 1024
GRID_MAX_STRIDE = 4096
GRID_LAYERS = dict(FEATURES, on_road=GRID_ON_ROAD)
(GCOUNT_PRESENT, GCOUNT_INSIDE, GCOUNT_LOST, GCOUNT_OUTSIDE) = range(4)


class GridSpec(_RowSpec):
    """The occupancy grid of hwy_grid (include/hwy.h), an immutable, hashable value.

    ``layers``: names out of FEATURES and "on_road", distinct; ``nx`` x ``ny`` cells of
    ``step_x`` x ``step_y`` metres whose cell 0 has its lower edge at (``x0``, ``y0``) from the
    ego; ``ranges``: {layer: (lo, hi)} mapped to [-1, 1]; ``clip``: clip the ranged layers;
    ``align``: the ego's axes instead of the road's; ``ego_tail``: append the ego's own
    Kinematics row; ``pad_to``: the row stride is the width rounded up to a multiple of it.  The
    defaults are upstream's OccupancyGrid features over the road ahead: presence, vx and vy on
    24 x 5 cells of 5 m x 4 m from 32.5 m behind to 87.5 m ahead and 10 m to either side.
    Everything hwy_grid_check refuses is a ValueError here."""

    __slots__ = ("layers", "nx", "ny", "x0", "y0", "step_x", "step_y", "ranges", "clip", "align",
                 "ego_tail", "pad_to")
    NOUN = "grid"
    MAX_STRIDE = GRID_MAX_STRIDE

    def __init__(self, layers=("presence", "vx", "vy"), nx: int = 24, ny: int = 5,
                 x0: float = -32.5, y0: float = -10.0, step_x: float = 5.0, step_y: float = 4.0,
                 ranges=None, clip: bool = True, align: bool = False, ego_tail: bool = True,
                 pad_to: int = 4):
        if ranges is None:  # upstream's, of the layers asked for
            ranges = {k: (-2 * MAX_SPEED, 2 * MAX_SPEED) for k in ("vx", "vy")
                      if not isinstance(layers, str) and k in layers}
        try:
            lay = tuple(str(n) for n in layers)
            gx, gy, pad = int(nx), int(ny), int(pad_to)
            geo = tuple(float(v) for v in (x0, y0, step_x, step_y))
            items = ranges.items() if isinstance(ranges, dict) else ranges
            rng = tuple(sorted((str(k), (float(lo), float(hi))) for k, (lo, hi) in items))
        except (TypeError, ValueError):
            raise ValueError(f"bad grid fields: layers={layers!r} nx={nx!r} ny={ny!r} x0={x0!r} "
                             f"y0={y0!r} step_x={step_x!r} step_y={step_y!r} ranges={ranges!r} "
                             f"pad_to={pad_to!r}") from None
        if isinstance(layers, str) or not 1 <= len(lay) <= GRID_MAX_LAYERS:
            raise ValueError(f"a grid takes 1..{GRID_MAX_LAYERS} layers, got {layers!r}")
        for n in lay:
            if n not in GRID_LAYERS:
                raise ValueError(f"unknown grid layer {n!r}; known: {list(GRID_LAYERS)}")
        if len(set(lay)) != len(lay):
            raise ValueError(f"a grid layer is given twice: {list(lay)}")
        if gx != nx or gy != ny or gx < 1 or gy < 1 or gx * gy > GRID_MAX_CELLS:
            raise ValueError(f"nx and ny must be integers >= 1 with nx * ny <= {GRID_MAX_CELLS}, "
                             f"got {nx!r} x {ny!r}")
        if not (math.isfinite(geo[0]) and math.isfinite(geo[1])):
            raise ValueError(f"x0 and y0 must be finite, got {x0!r}, {y0!r}")
        if not all(math.isfinite(s) and s > 0.0 for s in geo[2:]):
            raise ValueError(f"step_x and step_y must be finite and > 0, got {step_x!r}, {step_y!r}")
        for k, (lo, hi) in rng:
            if k not in lay or k == "on_road":
                raise ValueError(f"a range for {k!r}: not a vehicle layer of this grid {list(lay)}")
            if not (math.isfinite(lo) and math.isfinite(hi)) or lo == hi:
                raise ValueError(f"range of {k!r} must be finite with lo != hi, got {(lo, hi)!r}")
        if len(set(k for k, _ in rng)) != len(rng):
            raise ValueError(f"a range is given twice: {[k for k, _ in rng]}")
        if pad != pad_to or pad < 1:
            raise ValueError(f"pad_to must be an integer >= 1, got {pad_to!r}")
        self._init(layers=lay, nx=gx, ny=gy, x0=geo[0], y0=geo[1], step_x=geo[2], step_y=geo[3],
                   ranges=rng, clip=bool(clip), align=bool(align), ego_tail=bool(ego_tail),
                   pad_to=pad)

    @property
    def shape(self):
        """(C, W, H) of the layers: layer, cell along x, cell along y."""
        return (len(self.layers), self.nx, self.ny)

    @property
    def payload(self) -> int:
        """Floats of the layers."""
        return len(self.layers) * self.nx * self.ny

    def _json_fields(self):
        return {"layers": list(self.layers),
                "ranges": {k: [lo, hi] for k, (lo, hi) in self.ranges}}

    @classmethod
    def from_observation_config(cls, obs: Dict[str, Any], *, ego_tail: bool = True,
                                pad_to: int = 4) -> "GridSpec":
        """A GridSpec from the keys of upstream's OccupancyGrid observation config: ``features``
        (with "on_road"), ``grid_size`` [[x lo, x hi], [y lo, y hi]], ``grid_step`` [sx, sy],
        ``features_range``, ``align_to_vehicle_axes`` and ``clip``, each defaulting as upstream's
        does; the cell counts are floor((hi - lo) / step) in float64, as upstream takes them.
        ``absolute`` and ``as_image`` are refused, and so is any other key but ``type``."""
        if not isinstance(obs, dict):
            raise ValueError(f"an observation config is a dict, got {obs!r}")
        known = ("type", "features", "grid_size", "grid_step", "features_range",
                 "align_to_vehicle_axes", "clip", "absolute", "as_image")
        unknown = set(obs) - set(known)
        if unknown:
            raise ValueError(f"unknown OccupancyGrid keys {sorted(unknown)}; known: {list(known)}")
        if obs.get("type", "OccupancyGrid") != "OccupancyGrid":
            raise ValueError(f"not an OccupancyGrid observation config: type {obs.get('type')!r}")
        if obs.get("absolute"):
            raise ValueError("an absolute OccupancyGrid is not built: the grid is ego-centred")
        if obs.get("as_image"):
            raise ValueError("as_image is not built: the grid is float32")
        feats = list(obs.get("features") or ["presence", "vx", "vy"])
        size = obs.get("grid_size") or [[-27.5, 27.5], [-27.5, 27.5]]
        step = obs.get("grid_step") or [5, 5]
        try:
            (xlo, xhi), (ylo, yhi) = ((float(a), float(b)) for a, b in size)
            sx, sy = (float(s) for s in step)
        except (TypeError, ValueError):
            raise ValueError(f"bad grid_size {size!r} or grid_step {step!r}") from None
        if not (sx > 0.0 and sy > 0.0 and math.isfinite(sx) and math.isfinite(sy)):
            raise ValueError(f"grid_step must be finite and > 0, got {step!r}")
        if not all(math.isfinite(v) for v in (xlo, xhi, ylo, yhi)):
            raise ValueError(f"grid_size must be finite, got {size!r}")
        franges = obs.get("features_range")
        if franges is None:  # upstream's defaults, of the layers asked for
            franges = {"vx": [-2 * MAX_SPEED, 2 * MAX_SPEED], "vy": [-2 * MAX_SPEED, 2 * MAX_SPEED]}
        ranges = {k: v for k, v in dict(franges).items() if k in feats and k != "on_road"}
        return cls(layers=feats, nx=int(math.floor((xhi - xlo) / sx)),
                   ny=int(math.floor((yhi - ylo) / sy)), x0=xlo, y0=ylo, step_x=sx, step_y=sy,
                   ranges=ranges, clip=bool(obs.get("clip", True)),
                   align=bool(obs.get("align_to_vehicle_axes", False)), ego_tail=ego_tail,
                   pad_to=pad_to)

    def fill(self, a: GridArgs, n_features: int) -> GridArgs:
        """Write the grid's fields into hwy_grid_args ``a`` for a handle of ``n_features``."""
        a.nx, a.ny = self.nx, self.ny
        a.x0, a.y0, a.step_x, a.step_y = self.x0, self.y0, self.step_x, self.step_y
        a.align = int(self.align)
        a.n_layers = len(self.layers)
        rng = dict(self.ranges)
        for i, name in enumerate(self.layers):
            a.layer_ids[i] = GRID_LAYERS[name]
            if name in rng:
                a.has_range[i] = 1
                a.range[i][0], a.range[i][1] = rng[name]
        a.clip = int(self.clip)
        a.ego_tail = int(self.ego_tail)
        a.row_stride = self.stride(n_features)
        return a


class LidarArgs(ctypes.Structure):
    """hwy_lidar_args (include/hwy.h): one hwy_lidar launch's rays, sensor errors and outputs."""
    _fields_ = [
        ("cells", ctypes.c_int32),
        ("sub", ctypes.c_int32),
        ("range_m", ctypes.c_float),
        ("align", ctypes.c_int32),
        ("normalize", ctypes.c_int32),
        ("speed_scale", ctypes.c_float),
        ("p_drop", ctypes.c_float),
        ("sigma_r", ctypes.c_float),
        ("salt", ctypes.c_int32),
        ("ego_tail", ctypes.c_int32),
        ("row_stride", ctypes.c_int32),
        ("obs", ctypes.c_void_p),
        ("hit_vehicle", ctypes.c_void_p),
        ("seen", ctypes.c_void_p),
        ("counts", ctypes.c_void_p),
    ]


LIDAR_OUTPUTS = ("obs", "hit_vehicle", "seen", "counts")
HWY_LIDAR_SALT = 0x4C494441
LIDAR_MAX_CELLS = 1024
LIDAR_MAX_SUB = 16
LIDAR_MAX_RAYS = 4096
LIDAR_MAX_STRIDE = 4096
(LCOUNT_BODIES, LCOUNT_SEEN, LCOUNT_RETURNS, LCOUNT_DROPPED) = range(4)


class LidarSpec(_RowSpec):
    """The ray-cast range observation of hwy_lidar (include/hwy.h), an immutable, hashable value.

    ``cells`` directions around the ego, cell i centred on i * 2 pi / cells, each the nearest
    return of its ``sub`` sub-rays within ``range_m`` metres as (distance, relative radial speed);
    ``align``: cell 0 points along the ego's heading instead of the road's x; ``normalize``:
    distance / ``range_m`` and speed / ``speed_scale`` (None: ``range_m``, as upstream divides
    both columns by the range); ``p_drop``, ``sigma_r``, ``salt``: per-cell dropout probability,
    range noise in metres and the salt of their draws; ``ego_tail``: append the ego's own
    Kinematics row; ``pad_to``: the row stride is the width rounded up to a multiple of it.  The
    defaults are upstream's LidarObservation: 16 cells, 60 m, normalised.  Everything
    hwy_lidar_check refuses is a ValueError here."""

    __slots__ = ("cells", "sub", "range_m", "align", "normalize", "speed_scale", "p_drop",
                 "sigma_r", "salt", "ego_tail", "pad_to")
    NOUN = "lidar"
    MAX_STRIDE = LIDAR_MAX_STRIDE

    def __init__(self, cells: int = 16, sub: int = 1, range_m: float = 60.0, align: bool = False,
                 normalize: bool = True, speed_scale: Optional[float] = None, p_drop: float = 0.0,
                 sigma_r: float = 0.0, salt: int = 0, ego_tail: bool = True, pad_to: int = 4):
        if speed_scale is None:
            speed_scale = range_m
        try:
            n, s, slt, pad = int(cells), int(sub), int(salt), int(pad_to)
            rng, scale, drop, sig = (float(v) for v in (range_m, speed_scale, p_drop, sigma_r))
        except (TypeError, ValueError):
            raise ValueError(f"bad lidar fields: cells={cells!r} sub={sub!r} range_m={range_m!r} "
                             f"speed_scale={speed_scale!r} p_drop={p_drop!r} sigma_r={sigma_r!r} "
                             f"salt={salt!r} pad_to={pad_to!r}") from None
        if n != cells or not 1 <= n <= LIDAR_MAX_CELLS:
            raise ValueError(f"cells must be an integer in 1..{LIDAR_MAX_CELLS}, got {cells!r}")
        if s != sub or not 1 <= s <= LIDAR_MAX_SUB:
            raise ValueError(f"sub must be an integer in 1..{LIDAR_MAX_SUB}, got {sub!r}")
        if n * s > LIDAR_MAX_RAYS:
            raise ValueError(f"cells * sub must be <= {LIDAR_MAX_RAYS}, got {n} x {s}")
        if not (math.isfinite(rng) and rng > 0.0):
            raise ValueError(f"range_m must be finite and > 0, got {range_m!r}")
        if not (math.isfinite(scale) and scale > 0.0):
            raise ValueError(f"speed_scale must be finite and > 0, got {speed_scale!r}")
        if not 0.0 <= drop <= 1.0:
            raise ValueError(f"p_drop must lie in [0, 1], got {p_drop!r}")
        if not (math.isfinite(sig) and sig >= 0.0):
            raise ValueError(f"sigma_r must be finite and >= 0, got {sigma_r!r}")
        if slt != salt or not 0 <= slt <= 65535:
            raise ValueError(f"salt must be an integer in 0..65535, got {salt!r}")
        if pad != pad_to or pad < 1:
            raise ValueError(f"pad_to must be an integer >= 1, got {pad_to!r}")
        self._init(cells=n, sub=s, range_m=rng, align=bool(align), normalize=bool(normalize),
                   speed_scale=scale, p_drop=drop, sigma_r=sig, salt=slt, ego_tail=bool(ego_tail),
                   pad_to=pad)

    @property
    def shape(self):
        """(cells, 2): per cell the distance and the relative radial speed."""
        return (self.cells, 2)

    @property
    def payload(self) -> int:
        """Floats of the cells' pairs."""
        return 2 * self.cells

    @classmethod
    def from_observation_config(cls, obs: Dict[str, Any], *, ego_tail: bool = True,
                                pad_to: int = 4, **more) -> "LidarSpec":
        """A LidarSpec from the keys of upstream's LidarObservation config: ``cells``,
        ``maximum_range`` and ``normalize``, each defaulting as upstream's does; any other key but
        ``type`` is refused.  ``more``: this project's own fields (``sub``, ``align``, ...)."""
        if not isinstance(obs, dict):
            raise ValueError(f"an observation config is a dict, got {obs!r}")
        known = ("type", "cells", "maximum_range", "normalize")
        unknown = set(obs) - set(known)
        if unknown:
            raise ValueError(f"unknown LidarObservation keys {sorted(unknown)}; known: "
                             f"{list(known)}")
        if obs.get("type", "LidarObservation") != "LidarObservation":
            raise ValueError(f"not a LidarObservation config: type {obs.get('type')!r}")
        return cls(cells=obs.get("cells", 16), range_m=obs.get("maximum_range", 60),
                   normalize=obs.get("normalize", True), ego_tail=ego_tail, pad_to=pad_to, **more)

    def fill(self, a: LidarArgs, n_features: int) -> LidarArgs:
        """Write the spec's fields into hwy_lidar_args ``a`` for a handle of ``n_features``."""
        a.cells, a.sub = self.cells, self.sub
        a.range_m, a.speed_scale = self.range_m, self.speed_scale
        a.align, a.normalize = int(self.align), int(self.normalize)
        a.p_drop, a.sigma_r, a.salt = self.p_drop, self.sigma_r, self.salt
        a.ego_tail = int(self.ego_tail)
        a.row_stride = self.stride(n_features)
        return a


class LookaheadArgs(ctypes.Structure):
    """hwy_lookahead_args (include/hwy.h): one hwy_lookahead call's candidates and outputs."""
    _fields_ = [
        ("k", ctypes.c_int32),
        ("horizon", ctypes.c_int32),
        ("hold", ctypes.c_int32),
        ("lazy", ctypes.c_int32),
        ("gamma", ctypes.c_float),
        ("actions", ctypes.c_void_p),
        ("steps", ctypes.c_void_p),
        ("terminated", ctypes.c_void_p),
        ("truncated", ctypes.c_void_p),
        ("rewards", ctypes.c_void_p),
        ("ret", ctypes.c_void_p),
        ("ego_final", ctypes.c_void_p),
        ("obs", ctypes.c_void_p),
        ("chosen", ctypes.c_void_p),
        ("chosen_action", ctypes.c_void_p),
    ]


LOOKAHEAD_OUTPUTS = ("steps", "terminated", "truncated", "rewards", "ret", "ego_final", "obs",
                     "chosen", "chosen_action")
LOOKAHEAD_MAX_K = 64
LOOKAHEAD_MAX_H = 64
LOOKAHEAD_MAX_BRANCHES = 1 << 22


class Shield(_Record):
    """The action shield on top of hwy_lookahead (include/hwy.h), an immutable, hashable value.

    The policy's action, held for ``horizon`` policy steps, is candidate 0; the ``fallbacks``
    (pairs of raw actions, each held likewise) are candidates 1, 2, ...  The env executes the
    first candidate that does not terminate within the horizon, or, if all do, the one that
    survives longest.  ``lazy``: the fallbacks are rolled out only for envs whose candidate 0
    terminates (the choice is the same either way)."""

    __slots__ = ("horizon", "fallbacks", "lazy")
    NOUN = "shield"

    def __init__(self, horizon: int = 3, fallbacks=((-1.0, 0.0), (0.0, 0.0), (1.0, 0.0)),
                 lazy: bool = True):
        try:
            hz = int(horizon)
            fb = tuple((float(a), float(b)) for a, b in fallbacks)
        except (TypeError, ValueError):
            raise ValueError(f"bad shield fields: horizon={horizon!r} "
                             f"fallbacks={fallbacks!r}") from None
        if hz != horizon or not 1 <= hz <= LOOKAHEAD_MAX_H:
            raise ValueError(f"horizon must be an integer in 1..{LOOKAHEAD_MAX_H}, got {horizon!r}")
        if not 1 <= len(fb) <= LOOKAHEAD_MAX_K - 1:
            raise ValueError(f"a shield takes 1..{LOOKAHEAD_MAX_K - 1} fallbacks, got {len(fb)}")
        if not all(math.isfinite(x) for pair in fb for x in pair):
            raise ValueError(f"fallback actions must be finite, got {fallbacks!r}")
        self._init(horizon=hz, fallbacks=fb, lazy=bool(lazy))

    @property
    def k(self) -> int:
        """Candidates per env: the policy's action and the fallbacks."""
        return 1 + len(self.fallbacks)

    def _json_fields(self):
        return {"fallbacks": [list(p) for p in self.fallbacks]}


# the view hwy_render draws by default: upstream's AbstractEnv.default_config screen_width,
# screen_height, scaling and centering_position [highway-env 1.10.1]
RENDER_DEFAULTS = {"screen_width": 600, "screen_height": 150, "scaling": 5.5,
                   "centering_position": [0.3, 0.5]}


def render_view(cfg: Dict[str, Any]) -> Dict[str, Any]:
    """The config's view keys over RENDER_DEFAULTS, as (width, height, scaling, centering)."""
    v = dict(RENDER_DEFAULTS)
    v.update({k: cfg[k] for k in RENDER_DEFAULTS if cfg.get(k) is not None})
    cen = list(v["centering_position"])
    if len(cen) != 2:
        raise ValueError(f"centering_position must have two entries, got {cen!r}")
    return {"width": int(v["screen_width"]), "height": int(v["screen_height"]),
            "scaling": float(v["scaling"]), "centering": (float(cen[0]), float(cen[1]))}


class HwyConfig(ctypes.Structure):
    _fields_ = [
        ("num_envs", ctypes.c_int32),
        ("lanes_count", ctypes.c_int32),
        ("vehicles_count", ctypes.c_int32),
        ("obs_vehicles", ctypes.c_int32),
        ("n_features", ctypes.c_int32),
        ("feature_ids", ctypes.c_int32 * HWY_MAX_FEATURES),
        ("has_range", ctypes.c_int32 * HWY_MAX_FEATURES),
        ("features_range", (ctypes.c_float * 2) * HWY_MAX_FEATURES),
        ("order", ctypes.c_int32),
        ("absolute", ctypes.c_int32),
        ("normalize", ctypes.c_int32),
        ("clip", ctypes.c_int32),
        ("see_behind", ctypes.c_int32),
        ("sim_freq", ctypes.c_int32),
        ("policy_freq", ctypes.c_int32),
        ("max_steps", ctypes.c_int32),
        ("initial_lane_id", ctypes.c_int32),
        ("vehicles_density", ctypes.c_float),
        ("ego_spacing", ctypes.c_float),
        ("speed_limit", ctypes.c_float),
        ("collision_reward", ctypes.c_float),
        ("right_lane_reward", ctypes.c_float),
        ("high_speed_reward", ctypes.c_float),
        ("lane_change_reward", ctypes.c_float),
        ("on_road_reward", ctypes.c_float),
        ("reward_speed_range", ctypes.c_float * 2),
        ("normalize_reward", ctypes.c_int32),
        ("offroad_terminal", ctypes.c_int32),
        ("pe_kind", ctypes.c_int32),
        ("d_embed", ctypes.c_int32),
        ("ego_idx", ctypes.c_int32),
        ("pe_max_dist", ctypes.c_float),
        ("autoreset", ctypes.c_int32),
        ("env_offset", ctypes.c_int32),
        ("seed_base", ctypes.c_int64),
        ("seed_stride", ctypes.c_int64),
    ]

    def obs_features(self) -> int:
        extra = self.d_embed if self.pe_kind in PE_APPENDS else 0
        return int(self.n_features + extra)

    def as_dict(self) -> Dict[str, Any]:
        out = {}
        for name, _ in self._fields_:
            v = getattr(self, name)
            if isinstance(v, ctypes.Array):
                v = [list(x) if isinstance(x, ctypes.Array) else x for x in v]
            out[name] = v
        return out


# highway-env 1.10.1 defaults for keys the reference config may omit (HighwayEnv.default_config,
# AbstractEnv.default_config, KinematicObservation.__init__) [upstream, unverified offline].
_ENV_DEFAULTS = {
    "simulation_frequency": 15,
    "policy_frequency": 1,
    "duration": 40,
    "lanes_count": 4,
    "vehicles_count": 50,
    "initial_lane_id": None,
    "ego_spacing": 2,
    "vehicles_density": 1,
    "collision_reward": -1,
    "right_lane_reward": 0.1,
    "high_speed_reward": 0.4,
    "lane_change_reward": 0,
    "reward_speed_range": [20, 30],
    "normalize_reward": True,
    "offroad_terminal": False,
}
_OBS_DEFAULTS = {
    "vehicles_count": 5,
    "features": ["presence", "x", "y", "vx", "vy"],
    "features_range": None,
    "absolute": False,
    "order": "sorted",
    "normalize": True,
    "clip": True,
    "see_behind": False,
}
MAX_SPEED = 40.0
LANE_WIDTH = 4.0


def default_features_range(lanes_count: int) -> Dict[str, list]:
    """KinematicObservation.normalize_obs defaults when features_range is empty."""
    return {
        "x": [-5.0 * MAX_SPEED, 5.0 * MAX_SPEED],
        "y": [-LANE_WIDTH * lanes_count, LANE_WIDTH * lanes_count],
        "vx": [-2 * MAX_SPEED, 2 * MAX_SPEED],
        "vy": [-2 * MAX_SPEED, 2 * MAX_SPEED],
    }


def config_from_dict(
    cfg: Dict[str, Any],
    num_envs: int = 1,
    pe_kind: int = PE_NONE,
    d_embed: int = 0,
    ego_idx: int = 0,
    pe_max_dist: float = 100.0,
    autoreset: bool = False,
    env_offset: int = 0,
    seed_base: int = 0,
    seed_stride: Optional[int] = None,
) -> HwyConfig:
    """Translate a highway-env config dict (after make_env's merge) into hwy_config.

    Raises ValueError for settings the native env does not implement.
    """
    env = dict(_ENV_DEFAULTS)
    env.update({k: v for k, v in cfg.items() if k not in ("observation", "action")})
    obs = dict(_OBS_DEFAULTS)
    obs.update(cfg.get("observation", {}) or {})
    act = cfg.get("action", {"type": "ContinuousAction"}) or {}

    if obs.get("type", "Kinematics") != "Kinematics":
        raise ValueError(f"observation type {obs.get('type')!r} is not supported (Kinematics only)")
    if act.get("type", "ContinuousAction") != "ContinuousAction":
        raise ValueError(f"action type {act.get('type')!r} is not supported (ContinuousAction only)")
    if not (act.get("longitudinal", True) and act.get("lateral", True)):
        raise ValueError("ContinuousAction must control both longitudinal and lateral")

    c = HwyConfig()
    c.num_envs = int(num_envs)
    c.lanes_count = int(env["lanes_count"])
    c.vehicles_count = int(env["vehicles_count"])
    c.obs_vehicles = int(obs["vehicles_count"])
    feats = list(obs["features"])
    if not 1 <= len(feats) <= HWY_MAX_FEATURES:
        raise ValueError(f"between 1 and {HWY_MAX_FEATURES} features are supported, got {len(feats)}")
    c.n_features = len(feats)
    franges = obs.get("features_range") or default_features_range(c.lanes_count)
    for i, f in enumerate(feats):
        if f not in FEATURES:
            raise ValueError(f"unsupported Kinematics feature {f!r}")
        c.feature_ids[i] = FEATURES[f]
        if f in franges:
            c.has_range[i] = 1
            c.features_range[i][0] = float(franges[f][0])
            c.features_range[i][1] = float(franges[f][1])
    order = obs.get("order", "sorted")
    if order not in ("sorted", "shuffled"):
        raise ValueError(f"observation order must be 'sorted' or 'shuffled', got {order!r}")
    c.order = ORDER_SORTED if order == "sorted" else ORDER_SHUFFLED
    c.absolute = int(bool(obs.get("absolute", False)))
    c.normalize = int(bool(obs.get("normalize", True)))
    c.clip = int(bool(obs.get("clip", True)))
    c.see_behind = int(bool(obs.get("see_behind", False)))
    c.sim_freq = int(env["simulation_frequency"])
    c.policy_freq = int(env["policy_frequency"])
    if "max_episode_steps" in cfg:
        c.max_steps = int(cfg["max_episode_steps"])
    else:
        c.max_steps = int(math.ceil(float(env["duration"]) * DEFAULT_STEPS_PER_DURATION))
    lid = env.get("initial_lane_id")
    c.initial_lane_id = -1 if lid is None else int(lid)
    c.vehicles_density = float(env["vehicles_density"])
    c.ego_spacing = float(env["ego_spacing"])
    c.speed_limit = float(cfg.get("speed_limit", 30.0))
    c.collision_reward = float(env["collision_reward"])
    c.right_lane_reward = float(env["right_lane_reward"])
    c.high_speed_reward = float(env["high_speed_reward"])
    c.lane_change_reward = float(env["lane_change_reward"])
    c.on_road_reward = float(env.get("on_road_reward", 0.0))
    c.reward_speed_range[0] = float(env["reward_speed_range"][0])
    c.reward_speed_range[1] = float(env["reward_speed_range"][1])
    c.normalize_reward = int(bool(env["normalize_reward"]))
    c.offroad_terminal = int(bool(env["offroad_terminal"]))
    c.pe_kind = int(pe_kind)
    c.d_embed = int(d_embed)
    c.ego_idx = int(ego_idx)
    c.pe_max_dist = float(pe_max_dist)
    c.autoreset = int(bool(autoreset))
    c.env_offset = int(env_offset)
    c.seed_base = int(seed_base)
    c.seed_stride = int(num_envs if seed_stride is None else seed_stride)
    return c


def schedule_seed(cfg: HwyConfig, env: int, episode: int) -> int:
    """seed(env e, episode k) of include/hwy.h (= exp_seed + episode_num for one env)."""
    return int(cfg.seed_base + cfg.env_offset + env + 1 + cfg.seed_stride * episode)
