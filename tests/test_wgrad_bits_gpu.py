"""ppo_wgrad's chunk loop (csrc/ppo_kernels.hip, wgrad_tile_dma) reproduces, bit for bit, what
the build before the issue-slot / partner-stagger changes computed: tests/golden/
wgrad_parent_bits.json holds that build's SHA-256 of the flat gradient, the norm partials and
the metrics row after one hwy_ppo_forward_backward per shape (tools/record_wgrad_bits.py, seeded
CPU-drawn inputs).  Each case also passes the float64-autograd criterion of
test_edge_gradient_matches_autograd, so a stale fixture cannot hide an error.

The H = 64 shapes (three tiles) cover one ragged chunk, one whole chunk, whole + 1-row masked,
a ragged third chunk and three whole chunks per slice: at these counts the stagger's head and
tail and the buffer-reuse rule carry the whole result.  H = 256 runs the bench shape and the
balanced partition (two partial slots, extras walking several tiles in one workgroup)."""

import pytest

from wgrad_bits_util import SHAPES, load_golden, run_case, shape_id

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("c", SHAPES, ids=shape_id)
def test_wgrad_bits_match_parent_build(c):
    want = load_golden()[shape_id(c)]
    got = run_case(c)
    assert got == want, (shape_id(c), got, want)
