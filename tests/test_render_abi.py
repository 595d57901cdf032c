"""hwy_render without a GPU: the three symbols, the argument struct's layout, and the argument
checks, which return before any device call."""

import ctypes
import math

import pytest


def _lib():
    from hwy.native import lib

    return lib()


def _args(**kw):
    """A hwy_render_args that passes every check (its pointers are never dereferenced here)."""
    from hwy._abi import RenderArgs

    a = RenderArgs()
    a.width, a.height, a.channels, a.n = 600, 150, 3, 16
    a.scaling = 5.5
    a.centering[0], a.centering[1] = 0.3, 0.5
    a.frames = 0x1000
    for k, v in kw.items():
        if k == "centering":
            a.centering[0], a.centering[1] = v
        else:
            setattr(a, k, v)
    return a


def test_symbols_and_struct_layout():
    from hwy._abi import RenderArgs

    L = _lib()
    for name in ("hwy_render_args_size", "hwy_render_frame_bytes", "hwy_render"):
        assert hasattr(L, name)
    assert L.hwy_render_args_size() == ctypes.sizeof(RenderArgs)
    # hwy.h's field order on an LP64 ABI: four ints, three floats, padding, three pointers
    assert ctypes.sizeof(RenderArgs) == 56
    assert RenderArgs.scaling.offset == 16 and RenderArgs.centering.offset == 20
    assert RenderArgs.env_ids.offset == 32 and RenderArgs.frames.offset == 48


@pytest.mark.parametrize("kw, want", [
    (dict(), 16 * 150 * 600 * 3),
    (dict(channels=1, width=64, height=128, n=4096), 4096 * 128 * 64),
    (dict(width=1, height=1, n=1), 3),
    (dict(width=4096, height=4096, n=64), 64 * 4096 * 4096 * 3),  # past 2^31
])
def test_frame_bytes_of_good_arguments(kw, want):
    assert _lib().hwy_render_frame_bytes(ctypes.byref(_args(**kw))) == want


@pytest.mark.parametrize("kw", [
    dict(width=0), dict(width=-5), dict(width=4097), dict(height=0), dict(height=-1),
    dict(height=4097), dict(channels=2), dict(channels=0), dict(channels=4), dict(n=0), dict(n=-1),
    dict(scaling=0.0), dict(scaling=-1.0), dict(scaling=math.inf), dict(scaling=math.nan),
    dict(centering=(math.nan, 0.5)), dict(centering=(0.3, math.nan)),
    dict(centering=(math.inf, 0.5)), dict(frames=None), dict(frames=0x1008), dict(frames=0x1001)])
def test_each_bad_field_is_refused(kw):
    L = _lib()
    a = _args(**kw)
    assert L.hwy_render_frame_bytes(ctypes.byref(a)) == -1
    assert L.hwy_last_error().decode().startswith("hwy_render:")
    # hwy_render makes the same checks before it touches the handle (a fake one, never read)
    assert L.hwy_render(ctypes.c_void_p(0x1000), ctypes.byref(a), None) == -1


def test_null_handle_and_null_args_are_refused():
    L = _lib()
    assert L.hwy_render(None, ctypes.byref(_args()), None) == -1
    assert L.hwy_render(ctypes.c_void_p(0x1000), None, None) == -1
    assert L.hwy_render_frame_bytes(None) == -1
