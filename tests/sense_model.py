"""A numpy model of hwy_sense's front end (include/hwy.h): which vehicles the sensor sees and the
x, y and speed it perceives.  It shares no code with the kernel; Philox comes from
tests/rng_model.py.

Dropout and noise are float32 numpy, operation by operation as the contract writes them, and
are exact: the kernel's bits must equal them.

Range and line of sight are float64 with a bound on what binary32 can make of each compared
quantity.  The bound follows the contract's operations one by one: a binary32 operation returns
the nearest binary32 value to its real result, so a result whose operands carry no error and
whose real value binary32 holds is exact, and any other is off by at most U = 2^-24 of its
magnitude on top of what its operands carried:
    err(a + b) = err(a) + err(b) + round        err(a * b) = |a| err(b) + |b| err(a) + round
    round = 0 where err(a) = err(b) = 0 and the result is a binary32 value, else U (|v| + err)
    err(a + 0) = err(a) for an exact 0 (nothing is rounded)
(sin, cos) of a heading of exactly 0 are exactly (0, 1) in hm_sincosf; of any other heading they
are within SINCOS_ABS = 2e-7: tests/test_kernels_gpu.py::test_device_math_accuracy_against_libm
pins the device's sin and cos over [-20, 20] to libm within 2e-7 relative or 1e-7 absolute,
whichever is wider, and |sin|, |cos| <= 1 makes either at most 2e-7 absolute (headings stay
within +-pi).  |x|, min and max round nothing and keep the larger bound.  A comparison l <= r with bounds el, er is
*undecided* where el + er > 0 and |l - r| <= TOL * (el + er), TOL = 2; with el + er = 0 it is
decided exactly, equality included.  "blocked by j" (five comparisons, all must hold) is decided
false by one decided-false comparison, decided true by five decided-true ones and undecided
otherwise; "blocked" (some j) is decided true by one decided-true j, else undecided with one
undecided j.  An entry (env, present other vehicle) is undecided where its range test is, or
where it is not decidedly out of range and its blocked bit is undecided."""

from __future__ import annotations

import numpy as np

import rng_model as rm
from hwy import _abi

U = 2.0 ** -24
SINCOS_ABS = 2e-7
TOL = 2.0
SALT = 0x53454E53
HALF_LENGTH, HALF_WIDTH = 2.5, 1.0
DROP_CHANNEL = 3

MUTATIONS = (
    "half-length-2",           # the blocker's rectangle 4.0 long
    "blockers-visible-only",   # a hidden vehicle blocks nothing
    "ego-body-blocks",         # j runs from 0
    "channels-swapped",        # x takes channel 1's draw, y channel 0's
    "salt-ignored",            # SALT without the call's salt
    "range-on-perceived",      # the range test on the noisy positions
)


class B:
    """a real value and a bound on its distance from the binary32 evaluation, elementwise"""

    __slots__ = ("v", "e")

    def __init__(self, v, e=0.0):
        self.v = np.asarray(v, np.float64)
        self.e = np.broadcast_to(np.asarray(e, np.float64), self.v.shape)

    @staticmethod
    def _rounded(v, e):
        with np.errstate(over="ignore", invalid="ignore"):
            held = v.astype(np.float32).astype(np.float64) == v
        return B(v, np.where((e == 0.0) & held, 0.0, e + U * (np.abs(v) + e)))

    def __add__(self, o):
        r = B._rounded(self.v + o.v, self.e + o.e)
        for a, b in ((self, o), (o, self)):   # x + 0 is x: nothing is rounded
            r.e = np.where((a.v == 0.0) & (a.e == 0.0), b.e, r.e)
        return r

    def __sub__(self, o):
        return B._rounded(self.v - o.v, self.e + o.e)

    def __mul__(self, o):
        return B._rounded(self.v * o.v, np.abs(self.v) * o.e + np.abs(o.v) * self.e + self.e * o.e)

    def abs(self):
        return B(np.abs(self.v), self.e)

    def min(self, o):
        return B(np.minimum(self.v, o.v), np.maximum(self.e, o.e))

    def max(self, o):
        return B(np.maximum(self.v, o.v), np.maximum(self.e, o.e))


def le(l: B, r: B):
    """(l <= r, undecided) elementwise; a NaN compares false and decided"""
    with np.errstate(invalid="ignore"):
        d, t = l.v - r.v, l.e + r.e
        und = (t > 0.0) & (np.abs(d) <= TOL * t)
        return (d <= 0.0) & ~und, und


def const(c):
    return B(np.float64(c))


# ----------------------------------------------------------------------------- the state's words
def fields(cfg, state):
    """x, y, heading, speed [E, 64] float32, present [E, 64] bool, step [E], seed [E] uint64"""
    st = np.ascontiguousarray(state).view(np.uint32)
    V = cfg.vehicles_count + 1
    f = {n: st[i].view(np.float32) for n, i in (("x", _abi.F_X), ("y", _abi.F_Y),
                                                ("h", _abi.F_HEADING), ("spd", _abi.F_SPEED))}
    f["present"] = ((st[_abi.F_FLAGS] & _abi.FLAG_PRESENT) != 0) & (np.arange(64)[None, :] < V)
    f["step"] = st[_abi.F_ENV][:, _abi.E_STEP].astype(np.uint64)
    f["seed"] = rm.state_seeds(st)
    return f


def words(f, channel, salt, mut=""):
    """[E, 64, 4] Philox words of `channel`: counter (vehicle, step, channel, SALT + salt), key
    (seed low, seed high)"""
    E = f["step"].shape[0]
    s = np.uint64(SALT if mut == "salt-ignored" else (SALT + int(salt)) & 0xFFFFFFFF)
    ctr = np.empty((E, 64, 4), np.uint64)
    ctr[..., 0] = np.arange(64, dtype=np.uint64)[None, :]
    ctr[..., 1] = f["step"][:, None]
    ctr[..., 2] = np.uint64(channel)
    ctr[..., 3] = s
    key = np.stack([f["seed"] & np.uint64(0xFFFFFFFF), f["seed"] >> np.uint64(32)], -1)[:, None, :]
    return rm.philox4x32_10(ctr, key)


def u01(w):
    """hm_u01: the word's top 24 bits times 2^-24, exact in float32"""
    return (np.asarray(w, np.uint64) >> np.uint64(8)).astype(np.float32) * np.float32(2.0 ** -24)


def z_of(w):
    """the unit-variance draw of four words [..., 4], float32 operation by operation"""
    u = u01(w)
    return (((u[..., 0] + u[..., 1]) + (u[..., 2] + u[..., 3])) - np.float32(2.0)) * np.float32(1.7320508)


def perceive(f, sensor, mut=""):
    """x', y', speed' [E, 64] float32: vehicle 0 and a zero sigma leave the bits as they are"""
    chan = {"x": 0, "y": 1, "spd": 2}
    if mut == "channels-swapped":
        chan = {"x": 1, "y": 0, "spd": 2}
    out = {}
    for i, name in enumerate(("x", "y", "spd")):
        sig = np.float32(sensor.noise[i])
        val = f[name].copy()
        if sig != 0:
            with np.errstate(over="ignore", invalid="ignore"):
                moved = f[name] + sig * z_of(words(f, chan[name], sensor.salt, mut))
            val[:, 1:] = moved[:, 1:]
        out[name] = val
    return out


# ----------------------------------------------------------------------------- visibility
def _range(f, sensor, pos):
    """(in range, undecided) [E, 64]"""
    E = f["x"].shape[0]
    if sensor.range is None:
        return np.ones((E, 64), bool), np.zeros((E, 64), bool)
    r = np.float32(sensor.range)
    r2 = B(np.float64(np.float32(r * r)))          # the call squares it once, in binary32
    x, y = B(pos["x"]), B(pos["y"])
    dx, dy = x - B(pos["x"][:, :1]), y - B(pos["y"][:, :1])
    return le(dx * dx + dy * dy, r2)


def _blocked(f, bodies, first, mut=""):
    """(blocked, undecided) [E, 64] over the blockers `bodies` [E, 64] bool with index >= first"""
    hl = const(2.0 if mut == "half-length-2" else HALF_LENGTH)
    hw = const(HALF_WIDTH)
    x, y, h = (f[n].astype(np.float64) for n in ("x", "y", "h"))
    with np.errstate(invalid="ignore"):
        trig_e = np.where(h == 0.0, 0.0, SINCOS_ABS)
        c, s = B(np.cos(h)[:, None, :], trig_e[:, None, :]), B(np.sin(h)[:, None, :], trig_e[:, None, :])
    # axes: [E, k, j]
    xj, yj = B(x[:, None, :]), B(y[:, None, :])
    xe, ye = B(x[:, :1, None]), B(y[:, :1, None])
    xk, yk = B(x[:, :, None]), B(y[:, :, None])
    ax, ay, bx, by = xe - xj, ye - yj, xk - xj, yk - yj
    u0, w0 = ax * c + ay * s, ay * c - ax * s
    u1, w1 = bx * c + by * s, by * c - bx * s
    tests = (le(u0.min(u1), hl), le(const(-1.0) * hl, u0.max(u1)),
             le(w0.min(w1), hw), le(const(-1.0) * hw, w0.max(w1)),
             le((u0 * w1 - u1 * w0).abs(), hl * (w1 - w0).abs() + hw * (u1 - u0).abs()))
    false_ = np.zeros_like(tests[0][0])
    true_ = np.ones_like(false_)
    for ok, und in tests:
        false_ |= ~ok & ~und
        true_ &= ok
    jj = np.arange(64)
    pair = bodies[:, None, :] & (jj[None, None, :] >= first) & (jj[None, :, None] != jj[None, None, :])
    hit = true_ & pair
    maybe = ~true_ & ~false_ & pair
    blocked = hit.any(-1)
    return blocked, ~blocked & maybe.any(-1)


def sense(cfg, state, sensor, mut=""):
    """The sensor's view of `state`: a dict of [E, 64] arrays -- visible (bool; trustworthy where
    undecided is False), undecided, present, in_range, blocked, dropped (exact), hidden (float32),
    x, y, spd (float32, the perceived values, exact) -- and counts [E, 4] (trustworthy for the
    envs without an undecided entry, `counts_ok` [E])."""
    assert mut == "" or mut in MUTATIONS, mut
    sensor = _abi.SensorModel.from_dict(sensor)
    f = fields(cfg, state)
    other = f["present"].copy()
    other[:, 0] = False
    seen = perceive(f, sensor, mut)
    in_range, r_und = _range(f, sensor, seen if mut == "range-on-perceived" else f)
    if sensor.dropout > 0.0:
        dropped = u01(words(f, DROP_CHANNEL, sensor.salt, mut)[..., 0]) < np.float32(sensor.dropout)
    else:
        dropped = np.zeros_like(other)
    E = other.shape[0]
    blocked, b_und = np.zeros((E, 64), bool), np.zeros((E, 64), bool)
    if sensor.los:
        first = 0 if mut == "ego-body-blocks" else 1
        bodies = f["present"] if mut == "ego-body-blocks" else other
        blocked, b_und = _blocked(f, bodies, first, mut)
        if mut == "blockers-visible-only":
            blocked, b_und = _blocked(f, other & in_range & ~blocked & ~dropped, first, mut)
    visible = other & in_range & ~blocked & ~dropped
    visible[:, 0] = f["present"][:, 0]
    und = other & (r_und | ((in_range | r_und) & b_und))
    counts = np.stack([other.sum(1), (other & ~in_range).sum(1), (other & in_range & blocked).sum(1),
                       (other & in_range & ~blocked & dropped).sum(1)], 1).astype(np.int32)
    return dict(visible=visible, undecided=und, present=f["present"], in_range=in_range,
                blocked=blocked, dropped=dropped,
                hidden=(f["present"] & ~visible).astype(np.float32),
                counts=counts, counts_ok=~und.any(1), **seen)


def perceived_state(cfg, state, visible, seen):
    """`state` as the sensor hands it to the observation: the perceived x, y and speed in the
    words of vehicles 1.., and the present flag cleared where `visible` is 0"""
    st = np.ascontiguousarray(state).view(np.uint32).copy()
    for name, i in (("x", _abi.F_X), ("y", _abi.F_Y), ("spd", _abi.F_SPEED)):
        st[i][:, 1:] = np.ascontiguousarray(seen[name], np.float32).view(np.uint32)[:, 1:]
    gone = ~np.asarray(visible, bool)
    gone[:, 0] = False
    st[_abi.F_FLAGS][gone] &= np.uint32(~_abi.FLAG_PRESENT & 0xFFFFFFFF)
    return st
