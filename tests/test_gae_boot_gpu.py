"""hwy_gae_boot (include/hwy.h, ops.gae_boot) on the GPU: with no bootstrapped row it is hwy_gae bit
for bit, and in general it equals a numpy restatement of the formula in the header -- float64
arithmetic, float32 rounding at the same places (the library is built with -ffp-contract=off, so
no product is fused into a sum).

Shapes: T in {1, 8, 9, 19} (below, at and past the kernel's 8-step look-ahead, and two full
groups plus a remainder), E = 70 (two 64-thread blocks, the second partial); flags drawn with
p = 0.2 each, so rows with both flags set occur (p = 0.04)."""

import functools

import numpy as np
import pytest
import torch

from hwy import ops

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
E = 70
GAMMA, LAM = 0.99, 0.95
TS = [1, 8, 9, 19]


@functools.lru_cache(maxsize=None)
def _inputs(T):
    rng = np.random.default_rng(100 + T)
    rew = rng.normal(size=(T, E)).astype(np.float32)
    val = rng.normal(size=(T, E)).astype(np.float32)
    val[val == 0] = 1.0
    last = rng.normal(size=E).astype(np.float32)
    boot = rng.normal(size=(T, E)).astype(np.float32)
    term = (rng.random((T, E)) < 0.2).astype(np.uint8)
    trunc = (rng.random((T, E)) < 0.2).astype(np.uint8)
    return rew, term, trunc, val, last, boot


def _dev(*xs):
    return [torch.as_tensor(x, device=DEV) for x in xs]


def _restated(rew, term, trunc, val, last, boot, gamma, lam):
    """The header's formula, one env per array lane."""
    T = rew.shape[0]
    f64, f32 = np.float64, np.float32
    gamma, gl = f64(gamma), f64(gamma) * f64(lam)
    adv = np.zeros_like(rew)
    ret = np.zeros_like(rew)
    last_adv = np.zeros(rew.shape[1], f32)
    v1 = last.astype(f64)
    for t in range(T - 1, -1, -1):
        v0 = val[t]
        done = (term[t] | trunc[t]) != 0
        boot_row = (trunc[t] != 0) & (term[t] == 0)
        vsel = np.where(boot_row, boot[t].astype(f64), v1)
        m = np.where(done & ~boot_row, f64(0), f64(1))
        nd = np.where(done, f64(0), f64(1))
        delta = (rew[t].astype(f64) + (gamma * vsel) * m) - v0.astype(f64)
        a = (delta + (gl * nd) * last_adv.astype(f64)).astype(f32)
        adv[t] = a
        ret[t] = a + v0  # float32 + float32
        last_adv = a
        v1 = v0.astype(f64)
    assert adv.dtype == f32 and ret.dtype == f32
    return adv, ret


def _bits(x):
    return x.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("T", TS)
def test_no_truncation_is_gae_on_terminated(T):
    rew, term, _, val, last, boot = _inputs(T)
    r, te, v, l, b = _dev(rew, term, val, last, boot)
    tr = torch.zeros_like(te)
    adv, ret = ops.gae_boot(r, te, tr, v, l, b, GAMMA, LAM)
    adv0, ret0 = ops.gae(r, te, v, l, GAMMA, LAM)
    np.testing.assert_array_equal(_bits(adv), _bits(adv0))
    np.testing.assert_array_equal(_bits(ret), _bits(ret0))
    assert int(te.sum()) >= 1 or T == 1


@pytest.mark.parametrize("T", TS)
def test_zero_boot_values_is_gae_on_done(T):
    rew, term, trunc, val, last, _ = _inputs(T)
    assert (val != 0).all()
    r, te, tr, v, l = _dev(rew, term, trunc, val, last)
    adv, ret = ops.gae_boot(r, te, tr, v, l, torch.zeros_like(v), GAMMA, LAM)
    adv0, ret0 = ops.gae(r, te | tr, v, l, GAMMA, LAM)
    np.testing.assert_array_equal(_bits(adv), _bits(adv0))
    np.testing.assert_array_equal(_bits(ret), _bits(ret0))


@pytest.mark.parametrize("T", TS)
def test_general_case_equals_the_restated_formula(T):
    rew, term, trunc, val, last, boot = _inputs(T)
    both = int((term & trunc).sum())
    boots = int((trunc & ~term & 1).sum())
    print(f"T {T}: bootstrapped rows {boots}, rows with both flags {both}")
    assert boots >= 1
    if T >= 8:
        assert both >= 1
    out = (torch.full((T, E), float("nan"), device=DEV), torch.full((T, E), float("nan"),
                                                                   device=DEV))
    adv, ret = ops.gae_boot(*_dev(rew, term, trunc, val, last, boot), GAMMA, LAM, out=out)
    assert adv is out[0] and ret is out[1]
    want_adv, want_ret = _restated(rew, term, trunc, val, last, boot, GAMMA, LAM)
    np.testing.assert_array_equal(_bits(adv), want_adv.view(np.uint32))
    np.testing.assert_array_equal(_bits(ret), want_ret.view(np.uint32))
    # the bootstrap changes something: the same flags booked as terminal give other advantages
    adv0, _ = ops.gae(*_dev(rew, term | trunc, val, last), GAMMA, LAM)
    assert not np.array_equal(_bits(adv), _bits(adv0))


def test_shape_mismatch_is_refused():
    rew, term, trunc, val, last, boot = _inputs(8)
    r, te, tr, v, l, b = _dev(rew, term, trunc, val, last, boot)
    with pytest.raises(ValueError, match="boot_values"):
        ops.gae_boot(r, te, tr, v, l, b[:4], GAMMA, LAM)
