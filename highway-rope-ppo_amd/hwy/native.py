"""Loader for libhwy.so (the HIP/gfx950 C ABI of include/hwy.h).

The product path always runs through this library: there is no CPU fallback.  If the library is
missing or cannot be loaded, every compute entry point raises ``HwyNativeError``.
torch is imported first so that libhwy.so binds to the HIP runtime torch already loaded
(same soname, libamdhip64.so.7) and shares its streams.
"""

from __future__ import annotations

import ctypes
import os
import subprocess
from typing import Optional

from ._abi import (HWY_ABI_VERSION, GridArgs, HwyConfig, HwyStepInfo, LidarArgs, LookaheadArgs,
                   ObserveArgs, RenderArgs, SenseArgs, TrafficArgs)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libhwy.so")
CSRC = os.path.join(os.path.dirname(_HERE), "csrc")

HWY_OK, HWY_EINVAL, HWY_EDEVICE, HWY_ENOMEM = 0, -1, -2, -3


class HwyNativeError(RuntimeError):
    """libhwy.so is unavailable or a device call failed."""


_lib = None


class HwyStepIO(ctypes.Structure):
    """hwy_step_io (include/hwy.h): one handle's buffers for a grouped step."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("actions", "obs", "reward", "terminated",
                                               "truncated", "ep_return", "ep_length")]


class HwyStepGroupPlan(ctypes.Structure):
    _fields_ = [("n", ctypes.c_int32), ("blocks", ctypes.c_int32), ("big", ctypes.c_int32)]


def build(jobs: int = 4) -> str:
    """Compile libhwy.so for gfx950 (hipcc cross-compiles without a GPU)."""
    subprocess.run(["make", "-s", f"-j{jobs}", "-C", CSRC], check=True)
    return LIB_PATH


def _signatures() -> dict:
    """include/hwy.h as ctypes: name -> argtypes, or (argtypes, restype) where the function does
    not return an int."""
    vp, i32, i64, f32, f64 = (ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float,
                              ctypes.c_double)
    P = ctypes.POINTER
    plan, info = P(HwyStepGroupPlan), P(HwyStepInfo)
    return {
        "hwy_abi_version": [],
        "hwy_last_error": ([], ctypes.c_char_p),
        "hwy_create": [P(HwyConfig), i32, P(vp)],
        "hwy_destroy": ([vp], None),
        "hwy_obs_features": [vp],
        "hwy_set_pe_table": [vp, vp, i32],
        "hwy_set_seed_schedule": [vp, i64, ctypes.c_int32, i64],
        "hwy_set_seed_groups": [vp, vp, i32, i32],
        "hwy_reset": [vp] * 5,
        "hwy_step": [vp] * 9,
        "hwy_cut_episodes": [vp] * 6,
        "hwy_step_group_table_bytes": ([i32], i64),
        "hwy_step_group_prepare": [vp, vp, i32, vp, plan, vp],
        "hwy_step_group": [plan, vp, vp],
        "hwy_step_info_size": [],
        "hwy_step_with_info": [vp] * 8 + [info, vp],
        "hwy_step_group_info_table_bytes": ([i32], i64),
        "hwy_step_group_info_prepare": [vp, vp, vp, i32, vp, vp, plan, vp],
        "hwy_step_group_info": [plan, vp, vp, vp],
        "hwy_step_with_final": [vp] * 8 + [info, vp, vp],
        "hwy_step_group_final_table_bytes": ([i32], i64),
        "hwy_step_group_final_prepare": [vp, vp, vp, vp, i32, vp, vp, plan, vp],
        "hwy_step_group_final": [plan, vp, vp, vp],
        "hwy_gae": [vp, vp, vp, vp, f64, f64, i32, i32, vp, vp, vp],
        "hwy_gae_boot": [vp] * 6 + [f64, f64, i32, i32, vp, vp, vp],
        "hwy_render_args_size": [],
        "hwy_render_frame_bytes": ([P(RenderArgs)], i64),
        "hwy_render": [vp, P(RenderArgs), vp],
        "hwy_observe_args_size": [],
        "hwy_observe_check": [P(ObserveArgs)],
        "hwy_observe": [vp, P(ObserveArgs), vp],
        "hwy_traffic_args_size": [],
        "hwy_traffic_check": [P(TrafficArgs)],
        "hwy_traffic": [vp, P(TrafficArgs), vp],
        "hwy_sense_args_size": [],
        "hwy_sense_check": [P(SenseArgs)],
        "hwy_sense": [vp, P(SenseArgs), vp],
        "hwy_lookahead_args_size": [],
        "hwy_lookahead_check": [P(LookaheadArgs)],
        "hwy_lookahead": [vp, P(LookaheadArgs), vp],
        "hwy_grid_args_size": [],
        "hwy_grid_check": [P(GridArgs)],
        "hwy_grid": [vp, P(GridArgs), vp],
        "hwy_lidar_args_size": [],
        "hwy_lidar_check": [P(LidarArgs)],
        "hwy_lidar": [vp, P(LidarArgs), vp],
        "hwy_export_state": [vp, vp, vp],
        "hwy_import_state": [vp, vp, vp],
        "hwy_obs_pe": [vp, vp, i32, i32, i32, i32, i32, i32, f32, vp, vp, vp],
        "hwy_math_selftest": [i32, vp, vp, vp, i32, vp],
    }


def lib():
    """The loaded libhwy.so (raises HwyNativeError when it is missing)."""
    global _lib
    if _lib is not None:
        return _lib
    import torch  # noqa: F401  (load torch's HIP runtime first; see module docstring)

    if not os.path.exists(LIB_PATH):
        raise HwyNativeError(
            f"{LIB_PATH} not found: build it with `make -C {CSRC}` "
            "(or __graft_entry__.build()); there is no CPU fallback"
        )
    try:
        L = ctypes.CDLL(LIB_PATH, mode=ctypes.RTLD_GLOBAL)
    except OSError as e:  # pragma: no cover - depends on the box
        raise HwyNativeError(f"cannot load {LIB_PATH}: {e}") from e
    for name, sig in _signatures().items():
        fn = getattr(L, name)
        fn.argtypes, fn.restype = sig if isinstance(sig, tuple) else (sig, ctypes.c_int)
    for size, mirror, cname in (("hwy_step_info_size", HwyStepInfo, "hwy_step_info"),
                                ("hwy_render_args_size", RenderArgs, "hwy_render_args"),
                                ("hwy_observe_args_size", ObserveArgs, "hwy_observe_args"),
                                ("hwy_traffic_args_size", TrafficArgs, "hwy_traffic_args"),
                                ("hwy_sense_args_size", SenseArgs, "hwy_sense_args"),
                                ("hwy_lookahead_args_size", LookaheadArgs,
                                 "hwy_lookahead_args"),
                                ("hwy_grid_args_size", GridArgs, "hwy_grid_args"),
                                ("hwy_lidar_args_size", LidarArgs, "hwy_lidar_args")):
        if getattr(L, size)() != ctypes.sizeof(mirror):
            raise HwyNativeError(f"libhwy.so's {cname} differs from the python mirror; rebuild")
    if L.hwy_abi_version() != HWY_ABI_VERSION:
        raise HwyNativeError(
            f"libhwy.so ABI {L.hwy_abi_version()} != python ABI {HWY_ABI_VERSION}; rebuild"
        )
    _lib = L
    return L


def last_error() -> str:
    msg = lib().hwy_last_error()
    return msg.decode() if msg else ""


def check(rc: int, what: str) -> None:
    if rc == HWY_OK:
        return
    msg = f"{what}: {last_error()}"
    if rc == HWY_EINVAL:
        raise ValueError(msg)
    raise HwyNativeError(msg)


def ptr(t) -> Optional[int]:
    """Device pointer of a torch tensor (None passes NULL)."""
    if t is None:
        return None
    return t.data_ptr()


def stream_ptr(stream=None) -> Optional[int]:
    import torch

    s = torch.cuda.current_stream() if stream is None else stream
    return s.cuda_stream


def require_device(t, name: str) -> None:
    if not t.is_cuda:
        raise HwyNativeError(f"{name} must be a HIP device tensor (got {t.device}); no CPU path")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
