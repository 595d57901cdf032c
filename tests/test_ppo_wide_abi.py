"""The fused PPO path for state rows wider than 256 floats (S % 4 == 0, S <= 1,024), without a
GPU: the ABI calls that decide which shapes take it compute on the host only -- the tile image
offset, the workspace size, act_supported, the grouped table sizes -- and the parameter layout,
which does not depend on the path."""

import ctypes

import pytest

WIDE = [(260, 64), (300, 256), (600, 384), (1024, 512)]
# past the bound, and a width that is no multiple of 4 floats: the general path, torch acting
REFUSED = [(1028, 256), (302, 256)]


def _lib():
    from hwy.ppo_native import _bind, _bind_group, lib

    return _bind_group(_bind(lib()))


def _layout(S, H):
    """make_layout of csrc/ppo_kernels.hip: nn.Module.parameters() order, weights [out, in]."""
    sizes = [H * S, H, H * H, H, H * H, H, 2 * H, 2, 2, H * H, H, H, 1]
    offs, o = [], 0
    for n in sizes:
        offs.append(o)
        o += n
    return offs, o


@pytest.mark.parametrize("S,H", WIDE)
def test_wide_shapes_take_the_fused_path(S, H):
    from hwy.ppo_native import PpoDims, act_supported

    L = _lib()
    for B in (64, 8200):
        d = PpoDims(B, S, H, 2)
        assert L.hwy_ppo_tile_image_offset(ctypes.byref(d)) >= 0, (S, H, B)
        assert L.hwy_ppo_workspace_bytes(ctypes.byref(d)) > 0, (S, H, B)
    assert act_supported(S, H, 2)


@pytest.mark.parametrize("S,H", REFUSED)
def test_shapes_outside_the_range_keep_the_general_path(S, H):
    from hwy.ppo_native import PpoDims, act_supported

    L = _lib()
    d = PpoDims(64, S, H, 2)
    assert L.hwy_ppo_tile_image_offset(ctypes.byref(d)) == -1
    assert L.hwy_ppo_workspace_bytes(ctypes.byref(d)) > 0  # the general path still runs them
    assert not act_supported(S, H, 2)
    assert L.hwy_ppo_group_table_bytes(ctypes.byref(d), 2) == -1


@pytest.mark.parametrize("S,H", WIDE + REFUSED)
def test_param_layout_does_not_depend_on_the_path(S, H):
    from hwy.ppo_native import param_layout

    assert param_layout(S, H) == _layout(S, H)


def test_tile_image_holds_whole_k_blocks_of_w1():
    """The image is the workspace's last sub-buffer: W1's forward tiles (H / 16 column groups x
    the state blocks, zero-padded to whole ring groups of 16-deep blocks) and six H x H images."""
    from hwy.ppo_native import PpoDims

    L = _lib()
    for S, H in WIDE + [(256, 256), (60, 64)]:
        d = PpoDims(64, S, H, 2)
        nw = 8 if (H // 64) % 2 == 0 else 4
        depth = 4 if H // nw // 16 <= 4 else 2
        hb = -(-(H // 16) // depth) * depth
        sb = -(-(-(-S // 16)) // depth) * depth
        floats = (H // 16) * 256 * (sb + 6 * hb)
        ws = L.hwy_ppo_workspace_bytes(ctypes.byref(d))
        off = L.hwy_ppo_tile_image_offset(ctypes.byref(d))
        assert ws - off == -(-floats // 64) * 64 * 4, (S, H)


def test_wide_learners_join_grouped_tables():
    """The grouped table sizes accept wide learners, alone and beside narrow ones."""
    from hwy.ppo_native import PpoDims

    L = _lib()
    assert L.hwy_ppo_group_table_bytes(ctypes.byref(PpoDims(64, 360, 256, 2)), 3) > 0
    dims = [(64, 300, 128, 2), (64, 600, 256, 2), (64, 120, 320, 2)]
    arr = (PpoDims * 3)(*[PpoDims(*d) for d in dims])
    assert L.hwy_ppo_mixed_table_bytes(arr, 3) > 0
    sd = [(32, 300, 256, 2), (40, 600, 128, 2)]
    arr = (PpoDims * 2)(*[PpoDims(*d) for d in sd])
    nmb = (ctypes.c_int32 * 2)(2, 2)
    assert L.hwy_ppo_sched_table_bytes(arr, nmb, 2) > 0
