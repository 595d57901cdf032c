"""Conditions on the inputs of test_ppo_general_gpu.py and what its cases reach, checked without
a GPU: test_ppo_edge_inputs.check_grad_inputs, unchanged, on every ppo_ref_util.GENERAL_CASES row
(|z| <= 3, no rounding-level ReLU flip between torch fp32 and float64, clip margin > 1e-4,
20-80 % of the rows clipped with every (advantage sign, clip side) cell non-empty where B >= 32);
the split-K plan of each row (ppo_ref_util.general_plan, a restatement of split_for / chunk_for /
carve in csrc/ppo_kernels.hip), so that the set cannot quietly stop reaching the K loops if the
split rule changes; and that the library routes every row to the general path."""

import ctypes

import pytest
import torch

from ppo_ref_util import (COEFS, GENERAL_CASES, GENERAL_EXACT_CASES, GENERAL_NORM_CASES, GRAD_CASES,
                          GRAD_GENERAL_SHAPES, K_STEP, LOG_STDS, V_K, _grad64, case_id, case_kwargs,
                          dead_columns, edge_case, general_plan)
from test_ppo_edge_inputs import check_grad_inputs

CPU = torch.device("cpu")
PLANS = {c[:3]: general_plan(*c[:3]) for c in GENERAL_CASES}

# (slabs, kchunk) of d[Wa1;Wc1], dW2, dW1 that each row is there for, worked out by hand from
# split_for / chunk_for (256 workgroups over the output tiles, whole 32-row K-steps)
EXPECTED_PLAN = {
    (1, 64, 17): ((1, 32), (1, 32), (1, 32)),
    (33, 128, 40): ((2, 32), (2, 32), (2, 32)),
    (63, 192, 72): ((3, 32), (3, 32), (3, 32)),
    (65, 256, 130): ((5, 32), (5, 32), (5, 32)),
    (130, 320, 72): ((3, 32), (3, 32), (3, 32)),
    (25, 64, 1000): ((32, 32), (32, 32), (32, 32)),
    (258, 512, 300): ((2, 160), (4, 96), (5, 64)),
    (75, 512, 300): ((2, 160), (4, 96), (10, 32)),
    (130, 512, 1000): ((2, 512), (4, 256), (8, 128)),
    (1028, 64, 17): ((1, 32), (1, 32), (1, 32)),
    (1028, 256, 72): ((3, 32), (3, 32), (3, 32)),
    (1088, 128, 130): ((5, 32), (5, 32), (5, 32)),
    (1100, 512, 130): ((2, 96), (3, 64), (1, 160)),
    (1028, 512, 300): ((2, 160), (4, 96), (1, 320)),
    (1028, 384, 520): ((3, 192), (6, 96), (2, 288)),
}


def _lib():
    from hwy.ppo_native import _bind, lib

    return _bind(lib())


def test_settings_and_shapes_are_spread():
    """Distinct shapes, none shared with GRAD_CASES; every log_std and every (eps_clip,
    value_coef, entropy_coef) setting on a scalar (S % 4 != 0) and on a vector (S > 1,024) row;
    the exact and norm cases hold both kernels' rows and (258, 512, 300)."""
    shapes = [c[:3] for c in GENERAL_CASES]
    assert len(set(shapes)) == len(shapes)
    assert not set(shapes) & {c[:3] for c in GRAD_CASES}
    for rows in ([c for c in GENERAL_CASES if c[0] % 4], [c for c in GENERAL_CASES if c[0] > 1024]):
        assert {c[3] for c in rows} == set(range(len(LOG_STDS)))
        assert {c[4] for c in rows} == set(range(len(COEFS)))
    assert all(c[0] % 4 != 0 or c[0] > 1024 for c in GENERAL_CASES)
    for group in (GENERAL_EXACT_CASES, GENERAL_NORM_CASES):
        assert (258, 512, 300) in {c[:3] for c in group}
        assert any(c[0] > 1024 for c in group) and any(c[0] % 4 for c in group)


@pytest.mark.parametrize("c", GENERAL_CASES, ids=case_id)
def test_general_case_inputs(c):
    f = check_grad_inputs(c)
    # the in-kernel norm test runs at exactly the rows whose clipped step really clips
    assert (f["norm"] > 0.5) == (c in GENERAL_NORM_CASES), f["norm"]


@pytest.mark.parametrize("c", GENERAL_EXACT_CASES, ids=case_id)
def test_general_dead_unit_case_inputs(c):
    """As test_ppo_edge_inputs.test_dead_unit_case_inputs: the dead-unit variant is a case of its
    own and meets the same conditions; in float64 the dead units' gradients are exactly zero."""
    S, H, B = c[:3]
    dead = dead_columns(H)
    check_grad_inputs(c, dead=dead)
    a, _, s, z, lp, adv, ret, idx = edge_case(S, H, B, device=CPU, dead=dead, **case_kwargs(c))
    g64 = _grad64(a, s, z, lp, adv, ret, idx)
    for j in dead:
        assert not g64["shared.0.weight"][j].any() and g64["shared.0.bias"][j] == 0
        assert not g64["shared.2.weight"][:, j].any()


@pytest.mark.parametrize("c", GENERAL_CASES, ids=case_id)
def test_general_case_split_plan(c):
    """The row's split-K plan is the one it was chosen for, and the kernel of its dW1."""
    S, H, B = c[:3]
    p = PLANS[c[:3]]
    got = tuple((p[k]["slabs"], p[k]["kchunk"]) for k in ("ac", "2", "1"))
    assert got == EXPECTED_PLAN[c[:3]], got
    assert p["ac"]["vector"] and p["2"]["vector"] and p["1"]["vector"] == (S % 4 == 0)
    for q in p.values():  # the chunks partition the B rows, none empty
        assert sum(q["lens"]) == B and min(q["lens"]) >= 1 and max(q["lens"]) <= q["kchunk"]


def test_cases_reach_the_k_loops():
    """Over GENERAL_CASES, for each weight-gradient GEMM and each kernel that can run it (the
    H x H ones always gemm64v: their M and N are multiples of 64; dW1 gemm64v when S % 4 == 0,
    else scalar gemm64): a chunk of more than one K-tile (the prefetch branch), a chunk that ends
    inside a K-tile after a full one, and, somewhere, more than 16 slabs."""
    reach = {}
    for shape, p in PLANS.items():
        for name, q in p.items():
            r = reach.setdefault((name, q["vector"]), dict(multi=[], inside=[], slabs=0))
            assert q["ktile"] == (V_K if q["vector"] else K_STEP)
            if any(n > q["ktile"] for n in q["lens"]):
                r["multi"].append(shape)
            if any(n > q["ktile"] and n % q["ktile"] for n in q["lens"]):
                r["inside"].append(shape)
            r["slabs"] = max(r["slabs"], q["slabs"])
    assert set(reach) == {("ac", True), ("2", True), ("1", True), ("1", False)}
    for key, r in reach.items():
        assert r["multi"], key
        assert r["inside"], key
    assert all(reach[k]["slabs"] > 16 for k in (("ac", True), ("2", True), ("1", False)))
    # the scalar dW1 with two K-steps per workgroup, and the bias column sum over several tiles
    assert PLANS[(258, 512, 300)]["1"]["kchunk"] == 2 * K_STEP
    # gathered state rows behind gemm64v's prefetch: one chunk of five K-tiles
    assert PLANS[(1028, 512, 300)]["1"]["lens"] == [300]
    # the first layer's K loop (K = S): a single k, one k into the second K-step, and K-tiles of
    # the vector kernel followed by one float4
    assert {1, K_STEP + 1} <= {c[0] for c in GENERAL_CASES}
    assert any(c[0] > 1024 and c[0] % V_K == 4 for c in GENERAL_CASES)
    assert any(c[0] > 1024 and c[0] % V_K == 0 for c in GENERAL_CASES)


def test_existing_general_cases_run_their_k_loop_once():
    """Why GENERAL_CASES exists: every split-K chunk of GRAD_CASES' general shapes is one K-step."""
    for shape in GRAD_GENERAL_SHAPES:
        assert all(q["kchunk"] == K_STEP for q in general_plan(*shape).values()), shape


@pytest.mark.parametrize("c", GENERAL_CASES + tuple(c for c in GRAD_CASES
                                                    if c[:3] in GRAD_GENERAL_SHAPES), ids=case_id)
def test_library_routes_the_case_to_the_general_path(c):
    from hwy.ppo_native import PpoDims

    L = _lib()
    S, H, B = c[:3]
    d = PpoDims(B, S, H, 2)
    assert L.hwy_ppo_tile_image_offset(ctypes.byref(d)) == -1
    assert L.hwy_ppo_workspace_bytes(ctypes.byref(d)) > 0


def test_labels_of_grad_cases_match_the_library():
    """GRAD_CASES' shapes labelled general are exactly those without a tile image."""
    from hwy.ppo_native import PpoDims

    L = _lib()
    for c in GRAD_CASES:
        S, H, B = c[:3]
        off = L.hwy_ppo_tile_image_offset(ctypes.byref(PpoDims(B, S, H, 2)))
        assert (off == -1) == (c[:3] in GRAD_GENERAL_SHAPES), c[:3]
