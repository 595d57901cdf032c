"""tests/traffic_model.py on the CPU, on states stepped by the oracle: its neighbour search
against dyn_model's, the crafted states against values stated by hand, the share of entries a
rounding edge leaves undecided per natural case (at most 1 %), the fold, and that the cases tell
each deliberate mistake from the rule -- with the model's own float32 values standing in for the
kernel's, which tests/test_traffic_gpu.py puts in their place."""

from __future__ import annotations

import numpy as np
import pytest

import dyn_model as dm
import traffic_model as tm
import traffic_util as tu
from hwy import _abi

MAX_UNDECIDED = 0.01


@pytest.fixture(scope="module")
def natural():
    return {name: tu.oracle_states(name) for name in tu.NATURAL}


def as_outputs(m):
    """the model's values as the float32 arrays a kernel would hand back"""
    out = {k: m[k] for k in ("front", "rear", "gap")}
    with np.errstate(over="ignore"):
        out.update({k: m[k].v.astype(np.float32) for k in ("closing", "ttc", "thw", "risk")})
        ego = np.zeros((m["gap"].shape[0], tm.NEGO), np.float32)
        for s, v in m["ego_exact"].items():
            ego[:, s] = v
        for s, q in m["ego"].items():
            ego[:, s] = q.v.astype(np.float32)
    out["ego"] = ego
    return out


def test_slot_constants_match_the_abi():
    assert (tm.NEGO, tm.NACC) == (_abi.HWY_TRAFFIC_NEGO, _abi.HWY_TRAFFIC_NACC)
    assert tm.DEFAULTS == _abi.TRAFFIC_DEFAULTS
    assert sorted(tm.EXACT_EGO + tm.BOUND_EGO) == list(range(tm.NEGO))
    assert (_abi.EGO_GAP, _abi.EGO_TTC, _abi.EGO_THW, _abi.EGO_MIN_DISTANCE, _abi.EGO_RISK) == \
        (0, 2, 3, 11, 15)
    assert (_abi.TACC_N, _abi.TACC_MIN_TTC, _abi.TACC_TTC_CRITICAL, _abi.TACC_WITH_FRONT) == \
        (0, 1, 5, 7)


def test_neighbour_search_is_dyn_models(natural):
    n = 0
    for name, (cfg, states) in natural.items():
        for st in states[::8]:
            s = dm.unpack(cfg, st)
            L = int(cfg.lanes_count)
            lat = s["y"][:, :, None] - 4.0 * np.arange(L)
            onl = (np.abs(lat) <= 3.0) & (s["present"] & (s["x"] >= -5) & (s["x"] < 10005))[:, :, None]
            for got, want in zip(tm.neighbours(s["x"], onl), dm.neighbours(s["x"], onl)):
                assert np.array_equal(got, want), name
            n += 1
    assert n >= 40


def test_crafted_states_by_hand():
    cfg = tu.craft_cfg()
    m = tm.traffic_model(cfg, tu.craft(cfg))
    out = as_outputs(m)
    tu.check_crafted(out["front"], out["rear"], out["gap"], out["ego"])
    assert not tm.compare(m, out)
    for k in ("ttc", "thw", "risk"):
        assert not m["und"][k].any(), f"a crafted entry's {k} is undecided"


@pytest.mark.parametrize("name", list(tu.NATURAL))
def test_undecided_share_per_natural_case(natural, name):
    cfg, states = natural[name]
    und = present = fronts = 0
    for st in states:
        m = tm.traffic_model(cfg, st)
        assert not tm.compare(m, as_outputs(m)), "the model does not agree with itself"
        u = m["und"]["ttc"] | m["und"]["thw"] | m["und"]["risk"]
        und += int((u & m["present"]).sum())
        present += int(m["present"].sum())
        fronts += int((m["front"] >= 0).sum())
    print(f"{name}: {und} of {present} present entries undecided, {fronts} with a front")
    assert present >= len(states) * cfg.num_envs
    assert und <= MAX_UNDECIDED * present
    if cfg.vehicles_count >= 50:
        assert fronts > present // 4, "hardly a vehicle has a front: the case checks little"


def test_natural_cases_restart_episodes(natural):
    cfg, states = natural["E16-default"]
    assert (states[-1][_abi.F_ENV][:, _abi.E_EPISODE] > 0).all()


@pytest.mark.parametrize("mistake", list(tu.MISTAKES))
def test_cases_notice_each_deliberate_mistake(natural, mistake):
    kw = tu.MISTAKES[mistake]
    cases = [("crafted", tu.craft_cfg(), [tu.craft(tu.craft_cfg())])]
    cases += [(n, cfg, states[::4]) for n, (cfg, states) in natural.items()]
    noticed = []
    for name, cfg, states in cases:
        for st in states:
            right = as_outputs(tm.traffic_model(cfg, st))
            wrong = tm.traffic_model(cfg, st, kw.get("consts"),
                                     **{k: v for k, v in kw.items() if k != "consts"})
            if tm.compare(wrong, right):
                noticed.append(name)
                break
    assert noticed, f"no case tells '{mistake}' from the rule"
    print(f"{mistake}: noticed by {noticed}")


def test_fold_by_hand():
    F = np.float32
    inf = F(np.inf)
    acc = np.zeros((3, 8), F)
    acc[1] = [2, 3.0, 1.5, 30.0, 9.0, 0, 0, 2]
    acc[2] = [4, inf, inf, inf, 50.0, 0, 0, 0]
    ego = np.zeros((3, 16), F)
    ego[:, 2], ego[:, 3], ego[:, 0], ego[:, 11] = [1.0, 5.0, inf], [0.5, 1.2, inf], [10, 40, inf], [6, 7, 8]
    row = tm.state_row(ego, np.array([True, True, False]))
    assert row.tolist() == [[1, 1.0, 0.5, 10, 6, 1, 1, 1], [1, 5.0, F(1.2), 40, 7, 0, 0, 1],
                            [1, inf, inf, inf, 8, 0, 0, 0]]
    new, ep = tm.fold(acc, row, [False, False, True])
    assert new[0].tolist() == row[0].tolist()                       # n = 0: starts, no flush
    assert new[1].tolist() == [3, 3.0, F(1.2), 30.0, 7.0, 0, 0, 3]  # folded
    assert new[2].tolist() == row[2].tolist() and ep[2].tolist() == acc[2].tolist()
    assert not ep[:2].any()
