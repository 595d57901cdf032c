"""The shapes of the PPO memory tests (ppo_ref_util.MEMORY_*; the kernels run in
test_ppo_memory_gpu.py), without a GPU: that the host plan restated in ppo_ref_util (rows_tile,
fused_ok, rows_blocks, wgrad_plan, workspace_sizes) is the library's -- it must add up to
hwy_ppo_workspace_bytes and hwy_ppo_tile_image_offset, host queries that need no device and size
the partitions for the full MI355X (256 CUs, 8 XCDs) without one -- and that the set reaches every
addressing path named in ppo_ref_util.MEMORY_PATHS, each shape the paths it is there for."""

import ctypes

import pytest

from ppo_ref_util import (FULL_CHIP, GRAD_CASES, MEMORY_FUSED, MEMORY_GENERAL, MEMORY_PATHS,
                          WORK_REGIONS, act_kernel, fused_ok, general_plan, memory_act,
                          memory_large, memory_paths, ring_depth, rows_blocks, rows_tile,
                          tile_image_floats, wgrad_plan, workspace_floats, workspace_sizes)

CUS, XCDS = FULL_CHIP
ALL = MEMORY_FUSED + MEMORY_GENERAL + memory_large(CUS)


def _id(c):
    return "-".join(str(x) for x in c[0])


def _lib():
    from hwy.ppo_native import _bind, lib

    return _bind(lib())


def _queries(B, S, H):
    from hwy.ppo_native import PpoDims

    d = PpoDims(B, S, H, 2)
    L = _lib()
    return (int(L.hwy_ppo_workspace_bytes(ctypes.byref(d))),
            int(L.hwy_ppo_tile_image_offset(ctypes.byref(d))))


@pytest.mark.parametrize("c", ALL, ids=_id)
def test_shape_reaches_its_paths(c):
    (B, S, H), want = c
    got = memory_paths(S, H, B, CUS, XCDS)
    assert want <= got, (want - got, got)
    assert want <= MEMORY_PATHS and got <= MEMORY_PATHS


def test_the_set_reaches_every_path():
    reached = set()
    for (B, S, H), _ in ALL:
        reached |= memory_paths(S, H, B, CUS, XCDS)
    assert reached == MEMORY_PATHS, MEMORY_PATHS - reached


def test_what_the_tags_mean_at_these_shapes():
    """The plan figures behind the tags, written out for the shapes the issue names."""
    assert rows_tile(100, 128, 60, CUS) == 16 and 100 % 16 == 4 and 100 % 64 == 36
    # (129, 200, 320): 5 column tiles per wave -> a two-deep ring; 13 live W1 blocks in a
    # 14-block image, the 14th wholly past S
    assert ring_depth(320) == 2 and rows_blocks(200, 320) == (14, 20) and 14 * 16 - 200 >= 16
    assert ring_depth(448) == 2 and ring_depth(192) == 4 and ring_depth(512) == 4
    assert rows_tile(72, 256, 260, CUS) == 16 and rows_tile(1 << 20, 256, 260, CUS) == 16
    (b32, _), (b64, _) = memory_large(CUS)
    assert rows_tile(*[b32[i] for i in (0, 2, 1)], CUS) == 32
    assert rows_tile(b32[0] - 6, 128, 60, CUS) == 16          # just below the threshold
    assert rows_tile(*[b64[i] for i in (0, 2, 1)], CUS) == 64
    w = wgrad_plan(60, 256, b64[0], CUS, XCDS)
    # 26 tiles on 8 slices of 32 workgroups: 6 extras take 5 tiles' tails each; two slots
    assert (w["ntile"], w["split"], w["bal"], w["tpe"], w["nslot"]) == (26, 8, 1, 5, 2)
    assert w["wm"] < (-(-b64[0] // 8) + 63) // 64 and w["grid"] == CUS
    assert wgrad_plan(60, 128, b32[0], CUS, XCDS)["bal"] == 0
    # the general shapes: split-K slabs at (33, 30, 64) and (64, 75, 128), one slab at 16 rows
    assert [general_plan(30, 64, 33)[k]["slabs"] for k in ("ac", "2", "1")] == [2, 2, 2]
    assert general_plan(30, 64, 33)["1"]["lens"] == [32, 1]
    assert [general_plan(75, 128, 64)[k]["slabs"] for k in ("ac", "2", "1")] == [2, 2, 2]
    assert [general_plan(1028, 64, 16)[k]["slabs"] for k in ("ac", "2", "1")] == [1, 1, 1]
    assert not fused_ok(30, 64) and not fused_ok(1028, 64) and fused_ok(1024, 512)


def test_act_shapes_reach_every_act_kernel():
    got = {act_kernel(S, H, B, tiles, CUS) for B, S, H in memory_act(CUS) for tiles in (0, 1)}
    assert got == {("ppo_act_params", 16), ("ppo_act_tiles", 16), ("ppo_act_c", 16),
                   ("ppo_act_c", 32)}
    # the compact kernel at a ragged B in both tile heights; wide states keep 16-row tiles
    assert act_kernel(120, 256, 1000, 1, CUS) == ("ppo_act_c", 16) and 1000 % 16
    assert act_kernel(60, 256, 64 * CUS + 5, 1, CUS) == ("ppo_act_c", 32) and (64 * CUS + 5) % 32
    assert act_kernel(260, 256, 1 << 20, 1, CUS) == ("ppo_act_c", 16)
    assert any(B % 16 for B, _, _ in memory_act(CUS)) and any(S > 256 for _, S, _ in memory_act(CUS))


@pytest.mark.parametrize("c", ALL + tuple(((c[2], c[0], c[1]), None) for c in GRAD_CASES),
                         ids=_id)
def test_restated_workspace_is_the_librarys(c):
    """workspace_sizes (17 regions, each rounded to 64 floats) adds up to
    hwy_ppo_workspace_bytes; the tile image is the last region and starts where
    hwy_ppo_tile_image_offset says.  Also at every GRAD_CASES shape, so the restatement is pinned
    beyond the shapes it was written for."""
    (B, S, H), _ = c
    nbytes, off = _queries(B, S, H)
    sizes = workspace_sizes(S, H, B, CUS, XCDS)
    assert len(sizes) == len(WORK_REGIONS) == 17
    assert 4 * workspace_floats(S, H, B, CUS, XCDS) == nbytes
    if fused_ok(S, H):
        assert sizes[-1] == tile_image_floats(S, H) and sizes[-1] % 256 == 0
        assert off + 4 * sizes[-1] == nbytes
        assert all(n == 0 for n in sizes[7:13])  # no split-K slabs on the fused path
    else:
        assert off == -1 and sizes[-1] == sizes[-2] == sizes[-3] == 0


def test_tile_image_floats_is_the_fused_tests_formula():
    """test_ppo_fused_gpu._tile_image_floats (which the GPU tests use for the image's size),
    restated here without importing a GPU module."""
    for H in range(64, 513, 64):
        for S in (4, 60, 200, 256, 260, 1024):
            qh = H // 64
            nw = 8 if qh % 2 == 0 else 4
            d = 4 if H // nw // 16 <= 4 else 2
            hb = -(-(H // 16) // d) * d
            sb = -(-(-(-S // 16)) // d) * d
            assert tile_image_floats(S, H) == (H // 16) * sb * 256 + 6 * (H // 16) * hb * 256
