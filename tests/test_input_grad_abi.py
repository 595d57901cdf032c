"""hwy_ppo_input_grad without a GPU: the symbol and its argument struct's layout, and the argument
checks, which return -1 before any device call."""

import ctypes

import pytest


def _lib():
    from hwy.ppo_native import _bind_input_grad, lib

    return _bind_input_grad(lib())


def _args(B=17, S=60, H=256, A=2, K=3, null=None):
    """A hwy_ppo_input_grad_args whose pointers are non-NULL (never dereferenced: every call of
    these tests must be refused before a launch), with `null` cleared."""
    from hwy.ppo_native import PpoDims, PpoInputGradArgs

    a = PpoInputGradArgs()
    a.dims = PpoDims(B, S, H, A)
    a.K = K
    for f in ("states", "params", "cot", "dstates"):
        setattr(a, f, 0x1000)
    if null:
        setattr(a, null, None)
    return a


def test_symbol_and_struct_layout():
    from hwy.ppo_native import PpoDims, PpoInputGradArgs

    L = _lib()
    assert L.hwy_ppo_input_grad_args_size() == ctypes.sizeof(PpoInputGradArgs)
    # hwy_ppo.h's field order on an LP64 ABI: dims, two pointers, K (padded), five pointers
    assert ctypes.sizeof(PpoInputGradArgs) == ctypes.sizeof(PpoDims) + 8 * 8
    assert PpoInputGradArgs.K.offset == ctypes.sizeof(PpoDims) + 16
    assert PpoInputGradArgs.relu_bits.offset == ctypes.sizeof(PpoDims) + 7 * 8


def test_null_struct_is_refused():
    assert _lib().hwy_ppo_input_grad(None, None) == -1


@pytest.mark.parametrize("field", ["states", "params", "cot", "dstates"])
def test_null_required_pointer_is_refused(field):
    assert _lib().hwy_ppo_input_grad(ctypes.byref(_args(null=field)), None) == -1


@pytest.mark.parametrize("K", [0, 5, -1])
def test_cotangent_count_outside_1_to_4_is_refused(K):
    assert _lib().hwy_ppo_input_grad(ctypes.byref(_args(K=K)), None) == -1


@pytest.mark.parametrize("dims", [
    dict(B=0), dict(B=-3), dict(S=0), dict(S=-4), dict(S=62), dict(S=1028), dict(H=0), dict(H=32),
    dict(H=96), dict(H=576), dict(A=1), dict(A=3)])
def test_dims_outside_the_range_are_refused(dims):
    assert _lib().hwy_ppo_input_grad(ctypes.byref(_args(**dims)), None) == -1
