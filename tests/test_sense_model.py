"""tests/sense_model.py on its own (no GPU): the hand-stated cases, the draws' moments and
streams, how much of the natural states it leaves undecided, and that each of six deliberate
mistakes in it makes a case fail."""

from __future__ import annotations

import math

import numpy as np
import pytest

import rng_model as rm
import sense_model as sm
import sense_util as su
from hwy import _abi
from hwy._abi import SensorModel


# ------------------------------------------------------------------------------ the cases
def case_hand(mut=""):
    cfg = su.hand_cfg()
    st = su.hand_state(cfg)

    def visible_of(sensor):
        out = sm.sense(cfg, st, sensor, mut)
        if not mut:
            assert not out["undecided"].any(), \
                f"a hand case is undecided: {np.argwhere(out['undecided']).tolist()}"
        return out["visible"]

    su.check_hand(visible_of, "model: ")


def _philox_scalar(c, k):
    """Philox4x32-10 on Python integers: counter c[4], key k[2] -> four words"""
    c, k = list(c), list(k)
    for r in range(10):
        if r:
            k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xFFFFFFFF, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xFFFFFFFF]
    return c


def _z_scalar(vehicle, step, channel, salt, seed):
    w = _philox_scalar([vehicle, step, channel, (sm.SALT + salt) & 0xFFFFFFFF],
                       [seed & 0xFFFFFFFF, seed >> 32])
    u = [np.float32(x >> 8) * np.float32(2.0 ** -24) for x in w]
    return np.float32(np.float32(np.float32(u[0] + u[1]) + np.float32(u[2] + u[3])) - np.float32(2.0)) \
        * np.float32(1.7320508)


def case_channels(mut=""):
    """x', y' and speed' of a hand state against draws computed one by one on Python integers"""
    cfg = su.hand_cfg()
    st = su.hand_state(cfg)
    sensor = SensorModel(noise=(0.5, 0.25, 2.0), salt=9)
    out = sm.sense(cfg, st, sensor, mut)
    f = sm.fields(cfg, st)
    e = su.HAND_NAMES.index("leader")
    seed, step = int(f["seed"][e]), int(f["step"][e])
    for k in (1, 2, 3, 4):
        for c, (name, sig) in enumerate((("x", 0.5), ("y", 0.25), ("spd", 2.0))):
            want = np.float32(f[name][e, k] + np.float32(np.float32(sig) * _z_scalar(k, step, c, 9, seed)))
            assert out[name][e, k].view(np.uint32) == want.view(np.uint32), (name, k)
    for name in ("x", "y", "spd"):
        assert out[name][e, 0].view(np.uint32) == f[name][e, 0].view(np.uint32), "the ego moved"


def case_salt(mut=""):
    """the same (state, salt) gives the same bits, another salt other draws"""
    cfg, st = su.natural_state("E6-N15-50cars")
    a = sm.sense(cfg, st, SensorModel(dropout=0.5, noise=(1.0, 1.0, 1.0), salt=1), mut)
    b = sm.sense(cfg, st, SensorModel(dropout=0.5, noise=(1.0, 1.0, 1.0), salt=1), mut)
    c = sm.sense(cfg, st, SensorModel(dropout=0.5, noise=(1.0, 1.0, 1.0), salt=2), mut)
    others = a["present"][:, 1:]
    for name in ("x", "y", "spd", "dropped"):
        assert np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
        same = (a[name] == c[name])[:, 1:][others].mean()
        assert same < (0.6 if name == "dropped" else 0.01), f"{name}: salt 2 repeats salt 1 ({same:.2f})"


def case_ring(mut=""):
    """vehicles at exactly the range stay in range whatever noise their perceived position has"""
    cfg = make_ring_cfg()
    out = sm.sense(cfg, su.ring_state(cfg), su.RING_SENSOR, mut)
    n = len(su.RING)
    assert out["visible"][:, 1:n + 1].all() and not out["undecided"].any()
    assert (out["x"][:, 1:n + 1] != sm.fields(cfg, su.ring_state(cfg))["x"][:, 1:n + 1]).any()


def make_ring_cfg():
    return su.make_cfg(E=4, vehicles_count=len(su.RING), N=5)


CASES = {"hand": case_hand, "channels": case_channels, "salt": case_salt, "ring": case_ring}
# the case that refuses each mistake
REFUSED_BY = {"half-length-2": "hand", "blockers-visible-only": "hand", "ego-body-blocks": "hand",
              "channels-swapped": "channels", "salt-ignored": "salt", "range-on-perceived": "ring"}


@pytest.mark.parametrize("name", list(CASES))
def test_case(name):
    CASES[name]()


@pytest.mark.parametrize("mut", sm.MUTATIONS)
def test_each_mistake_fails_a_case(mut):
    assert set(REFUSED_BY) == set(sm.MUTATIONS)
    with pytest.raises(AssertionError):
        CASES[REFUSED_BY[mut]](mut)


def test_the_mistakes_fail_for_the_stated_reason():
    cfg = su.hand_cfg()
    st = su.hand_state(cfg)
    vis = {m: sm.sense(cfg, st, su.LOS, m)["visible"] for m in ("", "half-length-2",
                                                                "blockers-visible-only",
                                                                "ego-body-blocks")}
    e = su.HAND_NAMES.index
    assert not vis[""][e("u-min-at"), 2] and vis["half-length-2"][e("u-min-at"), 2]
    assert not vis[""][e("chain"), 3] and vis["blockers-visible-only"][e("chain"), 3]
    assert not vis["ego-body-blocks"][:, 1:].any()


# ------------------------------------------------------------------------------ the draws
def test_moments_of_a_million_draws():
    n = 1_000_000
    ctr = np.zeros((n, 4), np.uint64)
    ctr[:, 0] = np.arange(n) % 64
    ctr[:, 1] = np.arange(n) // 64
    ctr[:, 2] = 1
    ctr[:, 3] = sm.SALT + 5
    z = sm.z_of(rm.philox4x32_10(ctr, np.array([[0xDEADBEEF, 0x1234]], np.uint64))).astype(np.float64)
    assert z.dtype == np.float64 and z.shape == (n,)
    assert abs(z.mean()) <= 5.0 / math.sqrt(n), z.mean()
    assert abs(z.var() - 1.0) <= 5.0 * math.sqrt(1.7 / n), z.var()
    assert np.abs(z).max() <= 2.0 * math.sqrt(3.0)


def test_u01_and_z_are_float32_and_bounded():
    w = np.array([[0, 0, 0, 0], [0xFFFFFFFF] * 4, [0x80000000] * 4], np.uint64)
    z = sm.z_of(w)
    assert z.dtype == np.float32
    assert z[0] == np.float32(-2.0) * np.float32(1.7320508)
    assert z[2] == 0.0 and abs(float(z[1])) <= 2.0 * math.sqrt(3.0)


def test_dropout_edges():
    cfg, st = su.natural_state("E6-N15-50cars")
    others = sm.sense(cfg, st, su.NULL)["present"][:, 1:]
    assert not sm.sense(cfg, st, SensorModel(dropout=0.0))["dropped"].any()
    all_ = sm.sense(cfg, st, SensorModel(dropout=1.0))
    assert all_["dropped"].all() and not all_["visible"][:, 1:].any()
    assert np.array_equal(all_["counts"][:, 3], others.sum(1))
    half = sm.sense(cfg, st, SensorModel(dropout=0.5))["dropped"][:, 1:][others].mean()
    assert 0.35 < half < 0.65, half


def test_zero_sigma_keeps_the_bits():
    cfg = su.hand_cfg()
    st = su.hand_state(cfg)
    st[_abi.F_Y].view(np.float32)[0, 2] = -0.0
    out = sm.sense(cfg, st, SensorModel(noise=(1.0, 0.0, 0.0)))
    assert out["y"].view(np.uint32)[0, 2] == 0x80000000
    assert np.array_equal(out["spd"].view(np.uint32), st[_abi.F_SPEED])


# ------------------------------------------------------------------------------ natural states
@pytest.mark.parametrize("name", list(su.NATURAL))
def test_undecided_share_of_natural_states(name):
    cfg, st = su.natural_state(name)
    out = sm.sense(cfg, st, SensorModel(los=True, range=120.0))
    others = out["present"].copy()
    others[:, 0] = False
    share = out["undecided"].sum() / max(1, others.sum())
    print(f"{name}: {out['undecided'].sum()} of {others.sum()} entries undecided; "
          f"{(others & ~out['in_range']).sum()} out of range, {(others & out['blocked']).sum()} blocked")
    assert share <= 0.01, share
    if cfg.vehicles_count >= 50:
        assert (others & out["blocked"]).any() and (others & ~out["in_range"]).any()
    c = out["counts"]
    assert np.array_equal(c[:, 1] + c[:, 2] + c[:, 3] + out["visible"][:, 1:].sum(1), c[:, 0])


def test_perceived_state_clears_flags_and_moves_words():
    cfg, st = su.natural_state("E6-N15-50cars")
    out = sm.sense(cfg, st, su.FULL)
    ps = sm.perceived_state(cfg, st, out["visible"], out)
    f = sm.fields(cfg, ps)
    assert np.array_equal(f["present"][:, 1:], out["visible"][:, 1:])
    assert np.array_equal(f["x"].view(np.uint32), out["x"].view(np.uint32))
    assert np.array_equal(ps[_abi.F_HEADING], st[_abi.F_HEADING])
    assert np.array_equal(ps[_abi.F_X][:, 0], st[_abi.F_X][:, 0])
