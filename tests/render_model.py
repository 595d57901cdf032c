"""A float64 numpy model of hwy_render's frame rule (include/hwy.h), for the render tests.

It works from the binary32 state words and shares no code with the kernel.  ``render`` returns
the frame and a boolean ``undecided`` mask: a pixel is undecided when a comparison that can
change its colour has a margin below DELTA = 1e-3 m, and only the decided pixels are compared
with the kernel, exactly.

Why 1e-3 m.  The kernel evaluates the rule in binary32; this model evaluates it in float64 on
the same binary32 inputs, so the two can disagree only where a comparison's two sides are closer
than the kernel's rounding error:
  * every binary32 quantity in a margin is below 256 m, so its ulp is <= 1.5e-5 m;
  * fewer than 16 roundings enter a margin (a pixel centre: 3, an ego-relative vehicle centre:
    1, the rotated offsets: 2 differences, 2 products and 1 sum each);
  * hm_sincosf's absolute error is <= 1e-7 (pinned by tests/test_oracle_golden.py) and it
    multiplies lengths <= 256 m: <= 5.2e-5 m for the two terms.
Together that is < 3e-4 m; DELTA is about 3 times that.

Layers compose from the bottom: where a layer decisively covers a pixel, what lies below no
longer matters (the pixel becomes decided again); where a layer's coverage is within DELTA of
flipping, the pixel is undecided.

hm_sincosf returns (0, 0) for a finite |heading| > 16777215 (Cephes' total loss of precision) and
NaN for a non-finite one; the model does the same, since the rule is stated on hm_sincosf.
"""

import numpy as np

DELTA = 1e-3

F_X, F_Y, F_HEADING, F_FLAGS = 0, 1, 2, 11
NFIELDS, NVEH = 13, 64
FLAG_CRASHED, FLAG_PRESENT = 1, 4

BACKGROUND = (60, 60, 60)
ROAD = (100, 100, 100)
LINE = (255, 255, 255)
VEHICLE = (100, 200, 255)
EGO = (50, 200, 0)
CRASHED = (255, 100, 100)
HOT = (255, 220, 0)
LINE_HALF = 0.15
DASH_ON, DASH_PERIOD = 3.0, 8.0
HALF_LENGTH, HALF_WIDTH = 2.5, 1.0
ROAD_LENGTH = 10000.0


def luma(rgb):
    r, g, b = (int(v) for v in rgb)
    return (77 * r + 150 * g + 29 * b + 128) >> 8


def tint(base, s):
    """base tinted toward HOT by shade s (a binary32 value), in integer arithmetic."""
    s = float(np.float32(s))
    t = 0.0 if not s > 0.0 else min(s, 1.0)
    s8 = int(t * 256.0)
    return tuple((b * (256 - s8) + h * s8 + 128) >> 8 for b, h in zip(base, HOT))


def empty_state(num_envs):
    return np.zeros((NFIELDS, num_envs, NVEH), dtype=np.uint32)


def put(state, env, v, x, y, heading=0.0, flags=FLAG_PRESENT):
    """Write vehicle v of env into a state array (positions and heading as binary32 bits)."""
    for f, val in ((F_X, x), (F_Y, y), (F_HEADING, heading)):
        state[f, env, v] = np.array([val], dtype=np.float32).view(np.uint32)[0]
    state[F_FLAGS, env, v] = flags


def _and(conds):
    """Conjunction of (value, small-margin) pairs: (covered, ambiguous).  Ambiguous: some
    condition is within DELTA of flipping and no decisive condition is false."""
    cov = np.ones_like(conds[0][0], dtype=bool)
    any_small = np.zeros_like(cov)
    dec_false = np.zeros_like(cov)
    for val, small in conds:
        cov &= val
        any_small |= small
        dec_false |= ~val & ~small
    return cov, any_small & ~dec_false


def _le(a, b):
    with np.errstate(invalid="ignore"):
        return a <= b, np.abs(a - b) < DELTA


def _lt(a, b):
    with np.errstate(invalid="ignore"):
        return a < b, np.abs(a - b) < DELTA


def _sincos(h):
    h = float(h)
    if not np.isfinite(h):
        return np.nan, np.nan
    if abs(h) > 16777215.0:
        return 0.0, 0.0
    return float(np.sin(h)), float(np.cos(h))


def render(state, env, lanes, width, height, channels=3, scaling=5.5, centering=(0.3, 0.5),
           shade=None):
    """Frame [height, width, channels] uint8 of env ``env`` of ``state`` (uint32 [13, E, 64])
    and its undecided mask [height, width].  ``env`` outside 0..E-1: all background.
    ``shade``: None or float [E, 64]."""
    W, H = int(width), int(height)
    scaling = float(np.float32(scaling))
    c0, c1 = (float(np.float32(c)) for c in centering)
    frame = np.empty((H, W, 3), dtype=np.uint8)
    frame[:] = BACKGROUND
    und = np.zeros((H, W), dtype=bool)

    def paint(cov, amb, colour):
        frame[cov] = colour
        und[cov & ~amb] = False
        und[amb] = True

    E = state.shape[1]
    if 0 <= env < E:
        f32 = lambda f: state[f, env].view(np.float32).astype(np.float64)  # noqa: E731
        xs, ys, hs = f32(F_X), f32(F_Y), f32(F_HEADING)
        flags = state[F_FLAGS, env]
        xe, ye = xs[0], ys[0]
        px = np.broadcast_to((((np.arange(W) + 0.5) - c0 * W) / scaling)[None, :], (H, W))
        py = np.broadcast_to((((np.arange(H) + 0.5) - c1 * H) / scaling)[:, None], (H, W))
        in_x = [_le(-xe + 0 * px, px), _le(px, ROAD_LENGTH - xe + 0 * px)]
        yk = [(4.0 * k - 2.0) - ye for k in range(lanes + 1)]
        paint(*_and(in_x + [_le(yk[0] + 0 * py, py), _lt(py, yk[lanes] + 0 * py)]), ROAD)
        with np.errstate(invalid="ignore"):
            ph = xe - DASH_PERIOD * np.floor(xe / DASH_PERIOD)
            m = (px + ph) - DASH_PERIOD * np.floor((px + ph) / DASH_PERIOD)
            dash = (m < DASH_ON, (np.abs(m - DASH_ON) < DELTA) | (m < DELTA)
                    | (m > DASH_PERIOD - DELTA))
        for k in range(lanes + 1):
            conds = in_x + [_le(np.abs(py - yk[k]), LINE_HALF + 0 * py)]
            if 0 < k < lanes:
                conds = conds + [dash]
            paint(*_and(conds), LINE)
        for v in list(range(1, NVEH)) + [0]:
            if v != 0 and not flags[v] & FLAG_PRESENT:
                continue
            base = CRASHED if flags[v] & FLAG_CRASHED else (EGO if v == 0 else VEHICLE)
            colour = base if shade is None else tint(base, shade[env][v])
            sh, ch = _sincos(hs[v])
            with np.errstate(invalid="ignore"):
                dx, dy = px - (xs[v] - xe), py - (ys[v] - ye)
                lon, lat = dx * ch + dy * sh, dy * ch - dx * sh
            paint(*_and([_le(np.abs(lon), HALF_LENGTH + 0 * px),
                         _le(np.abs(lat), HALF_WIDTH + 0 * px)]), colour)
    if channels == 1:
        r, g, b = (frame[..., i].astype(np.int64) for i in range(3))
        frame = ((77 * r + 150 * g + 29 * b + 128) >> 8).astype(np.uint8)[..., None]
    return frame, und


# ------------------------------------------------------------------------------------------------
# Crafted scenes at scaling 8 (E = 2, lanes_count 4, the ego in lane 1's centre): pixel centres
# are odd multiples of 1/16 m, every edge below is a multiple of 1/2 m away from the ego, the
# line edge 0.15 lies 0.0375 m from the nearest centre and the dash edges are whole metres from
# whole-metre ego positions, so no pixel is undecided.
PI = float(np.float32(np.pi))


def scene_lone(headings=(0.0, PI / 2)):
    s = empty_state(2)
    for e, h in enumerate(headings):
        put(s, e, 0, 100.0, 4.0, h)
    return s


def scene_dash(xes=(100.0, 101.0)):
    s = empty_state(2)
    for e, x in enumerate(xes):
        put(s, e, 0, x, 4.0)
    return s


def scene_overlap():
    """The ego under two overlapping cars, 5 and 9; the crashed one is 9 in env 0, 5 in env 1."""
    s = empty_state(2)
    for e in range(2):
        put(s, e, 0, 100.0, 4.0)
        put(s, e, 5, 101.0, 4.5, flags=FLAG_PRESENT | (FLAG_CRASHED if e == 1 else 0))
        put(s, e, 9, 102.0, 5.0, flags=FLAG_PRESENT | (FLAG_CRASHED if e == 0 else 0))
    return s


def scene_flags():
    """A crashed ego; car 3 to its right absent in env 0 and present in env 1; car 4, present,
    at a NaN position on top of it."""
    s = empty_state(2)
    for e in range(2):
        put(s, e, 0, 100.0, 4.0, flags=FLAG_PRESENT | FLAG_CRASHED)
        put(s, e, 3, 103.0, 4.0, flags=FLAG_PRESENT if e == 1 else 0)
        put(s, e, 4, np.nan, 4.0)
    return s


def scene_road_start():
    """The ego at x = 1 (the road begins 1 m behind it) and at x = 9,999 (it ends 1 m ahead)."""
    s = empty_state(2)
    put(s, 0, 0, 1.0, 4.0)
    put(s, 1, 0, 9999.0, 4.0)
    return s


SCENES = {"lone": scene_lone, "dash": scene_dash, "overlap": scene_overlap,
          "flags": scene_flags, "road_start": scene_road_start}
SCENE_VIEW = dict(scaling=8.0, centering=(0.5, 0.5))


def scene_edges():
    """The GPU tests' crafted state (E = 2, default view 600x150 at 5.5): headings 0, pi/4, pi/2,
    -3 and +-pi -+ 1e-3, two overlapping cars, a car half outside the view, a car exactly at the
    view's cull distance (its centre 2.7 m past the right edge), an absent slot, a crashed ego;
    env 1: an ego at x = 1 with the same cars ahead; the ego at x = 9,999 is scene_road_start."""
    s = empty_state(2)
    right = (600 - 0.5 - 0.3 * 600) / 5.5  # the last pixel centre's x
    cars = [(10.0, 0.0, 0.0), (20.0, 4.0, PI / 4), (30.0, -4.0, PI / 2), (40.0, 4.0, -3.0),
            (50.0, 0.0, PI - 1e-3), (60.0, -4.0, -PI + 1e-3),
            (12.0, 1.0, 0.1),               # overlaps the first
            (right, 8.0, 0.0),              # half outside the view
            (right + 2.7, 0.0, 0.0),        # at the cull distance
            (-31.0, 4.0, 0.0)]              # half outside on the left
    for e, xe in enumerate((500.0, 1.0)):
        put(s, e, 0, xe, 4.0, 0.02, flags=FLAG_PRESENT | (FLAG_CRASHED if e == 0 else 0))
        for i, (dx, dy, h) in enumerate(cars):
            put(s, e, 1 + 2 * i, xe + dx, 4.0 + dy, h)
        put(s, e, 2, xe + 5.0, 4.0, flags=0)  # absent: on top of the ego's nose if drawn
    return s


# ------------------------------------------------------------------------------------------------
# Natural inputs of the GPU tests: (name, envs, steps, config overrides, seed of the actions).
# Each is the default config with the overrides, schedule seed base 11, reset and then stepped
# with uniform +-0.3 actions.  The CPU oracle reaches the same states bit for bit, so
# tests/test_render_model.py checks the 1 % cap on undecided pixels for every one of them without
# a GPU.  ("63-others" takes action seed 1: with seed 0 a lane-line edge of env 1 falls within
# DELTA of two pixel rows' centres, 1.7 % of the frame.)
NATURAL = [
    ("default", 4, 5, {}, 0),
    ("lanes-1", 2, 2, dict(lanes_count=1), 0),
    ("lanes-8", 2, 2, dict(lanes_count=8), 0),
    ("63-others", 2, 2, dict(vehicles_count=63, lanes_count=16), 1),
]
TAILS = ("tails", 3, 2, {}, 1)  # the state of the store-tail, env_ids and shade tests
TAIL_SIZES = [(37, 13), (1, 1), (16, 1), (17, 3), (600, 150)]
TAIL_CENTERINGS = [(0.5, 0.5), (0.0, 1.0)]
SEED_BASE = 11


def natural_actions(case):
    """The case's actions, one float32 [E, 2] array per step."""
    _, E, steps, _, seed = case
    rng = np.random.default_rng(seed)
    return [rng.uniform(-0.3, 0.3, size=(E, 2)).astype(np.float32) for _ in range(steps)]


def shade_values(E):
    """The shade test's input: 0, 1, 0.5, -1, 2 and NaN spread over the vehicles, and 1, 0.5 and
    NaN on the first three egos."""
    vals = np.array([0.0, 1.0, 0.5, -1.0, 2.0, np.nan], dtype=np.float32)
    i = np.arange(E * NVEH)
    shade = vals[(i * 5 + i // NVEH) % 6].reshape(E, NVEH)
    shade[:3, 0] = [1.0, 0.5, np.nan][:E]
    return shade
