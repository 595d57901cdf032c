"""hwy_lookahead on the GPU against the CPU oracle, bit for bit: every output of the cases of
tests/lookahead_util.py in both action forms and with subsets of the outputs, a shuffled handle
with per-group RankPE tables, a part-filled last workgroup, one step against a clone handle, an
ego that has already crashed, the untouched handle, lazy, the shield's choice, a captured graph,
and five deliberate mistakes of the expected-value driver, each refused by the case that can see it."""

from __future__ import annotations

import ctypes

import numpy as np
import pytest

import lookahead_util as lu
from env_util import HipEnv
from hwy import _abi
from parity_util import make_cfg, pe_table_for, policy_actions

pytestmark = pytest.mark.gpu

SUBSETS = (("ret",), ("obs",), ("steps", "terminated"), ("rewards", "ego_final"), ("truncated",))


def compare(got, want, what, names=None):
    for n in names or got:
        lu.same_bits(got[n], want[n], f"{what}: {n}")


# ------------------------------------------------------------------- 1. the three cases
@pytest.mark.parametrize("name", list(lu.CASES))
def test_every_output_equals_the_oracle(name):
    cfg, states = lu.snapshots(name)
    _, E, H, *_ = lu.CASES[name]
    refused = set()
    hip = HipEnv(cfg)
    try:
        hip.reset()
        for i, ((st, acts, want), (_, _, want9)) in enumerate(zip(lu.expected(name),
                                                                 lu.expected(name, 0.9))):
            what = f"{name} snapshot {i}"
            hip.set_state(st)
            got = lu.hip_lookahead(hip, acts, H)
            compare(got, want, what)
            got9 = lu.hip_lookahead(hip, acts, H, gamma=0.9)
            compare(got9, want9, what + " gamma 0.9")
            # the held form of the five held candidates is the sequence form's
            held = lu.hip_lookahead(hip, acts[:, :5, 0], H, hold=True, gamma=0.9)
            compare(held, {k: v[:, :5] for k, v in want9.items()}, what + " hold")
            for names in SUBSETS:
                compare(lu.hip_lookahead(hip, acts, H, gamma=0.9, outputs=names), want9,
                        what + f" outputs {names}")
            assert np.array_equal(hip.state(), st.view(np.uint32)), f"{what}: the state was written"
            if name == "default":
                for m in ("past_done", "discount_first"):
                    wrong = lu.oracle_lookahead(cfg, st, acts, gamma=0.9, mistake=m)
                    if lu.differs(got9, wrong, lu.OUTPUTS):
                        refused.add(m)
        if name == "default":  # the mistaken drivers' values are not the kernel's
            assert refused == {"past_done", "discount_first"}, refused
    finally:
        hip.close()


# ------------------------------------------------------------------- 2. shuffled, RankPE, groups
def test_shuffled_rank_pe_with_two_seed_groups():
    from hwy.native import check, lib

    E, H, d = 8, 3, 8
    cfg = make_cfg(E=E, order="shuffled", pe=_abi.PE_RANK, d=d, max_episode_steps=5)
    tables = np.stack([pe_table_for(_abi.PE_RANK, d, cfg.obs_vehicles, seed=s) for s in (1, 2)])
    assert not np.array_equal(tables[0], tables[1])
    hip = HipEnv(cfg, tables[0])
    try:
        hip.set_seed_groups([100, 2000], 4)
        t = np.ascontiguousarray(tables, np.float32)
        check(lib().hwy_set_pe_table(hip.h, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
              "hwy_set_pe_table")
        hip.reset()
        rng = np.random.default_rng(1)
        acts = lu.candidates(E, H)[:, [0, 2, 5]]
        per_env = [tables[e // 4] for e in range(E)]
        by_branch_refused = False
        for t_ in range(4):
            st = hip.state()
            got = lu.hip_lookahead(hip, acts, H, gamma=0.9)
            want = lu.oracle_lookahead(cfg, st, acts, gamma=0.9, tables=per_env)
            compare(got, want, f"groups, step {t_}")
            wrong = lu.oracle_lookahead(cfg, st, acts, gamma=0.9, tables=per_env,
                                        mistake="table_by_branch")
            by_branch_refused |= lu.differs(got, wrong, ("obs",))
            assert np.array_equal(hip.state(), st)
            hip.step(policy_actions(rng, E, t_))
        assert by_branch_refused, "the group table indexed by branch gives the same obs"
    finally:
        hip.close()


# ------------------------------------------------------------------- 3. shapes
def stepped(cfg, steps, seed=2, table=None):
    hip = HipEnv(cfg, table)
    hip.reset()
    rng = np.random.default_rng(seed)
    for t in range(steps):
        hip.step(policy_actions(rng, cfg.num_envs, t))
    return hip


def test_part_filled_last_workgroup():
    cfg = make_cfg(E=5, max_episode_steps=6)
    hip = stepped(cfg, 2)
    try:
        st = hip.state()
        acts = lu.candidates(5, 4)[:, [1, 3, 5]]  # 15 waves: the fourth workgroup holds three
        compare(lu.hip_lookahead(hip, acts, 4, gamma=0.9),
                lu.oracle_lookahead(cfg, st, acts, gamma=0.9), "E 5, K 3")
    finally:
        hip.close()


def test_one_branch_of_one_step_is_a_step_of_a_clone_handle():
    """the route include/hwy.h documents: export, import into an autoreset-off handle, hwy_step"""
    cfg = make_cfg(E=1, order="shuffled", max_episode_steps=6)
    off = make_cfg(E=1, order="shuffled", max_episode_steps=6, autoreset=False)
    hip, clone = stepped(cfg, 3), HipEnv(off)
    try:
        st = hip.state()
        a = np.array([[[[0.4, -0.2]]]], np.float32)
        got = lu.hip_lookahead(hip, a, 1)
        clone.reset()
        clone.set_state(st)
        obs, rew, term, trunc, _, _ = clone.step(a[0, 0])
        after = clone.state()
        lu.same_bits(got["obs"][:, 0], obs, "obs")
        lu.same_bits(got["rewards"][:, 0, 0], rew, "reward")
        lu.same_bits(got["ret"][:, 0], rew, "ret")
        assert got["steps"].tolist() == [[1]]
        assert got["terminated"][:, 0].tolist() == term.tolist()
        assert got["truncated"][:, 0].tolist() == trunc.tolist()
        ego = np.stack([after[f].view(np.float32)[:, 0] for f in
                        (_abi.F_X, _abi.F_Y, _abi.F_HEADING, _abi.F_SPEED)], 1)
        lu.same_bits(got["ego_final"][:, 0], ego, "ego_final")
        compare(got, lu.oracle_lookahead(cfg, st, a), "E 1, K 1, H 1")
    finally:
        hip.close()
        clone.close()


def test_an_ego_that_has_already_crashed_ends_every_branch_at_once():
    cfg = make_cfg(E=4, max_episode_steps=20, autoreset=False)
    hip = stepped(cfg, 2)
    try:
        st = hip.state()
        st[_abi.F_FLAGS][:, 0] |= _abi.FLAG_CRASHED
        hip.set_state(st)
        acts = lu.candidates(4, 3)
        got = lu.hip_lookahead(hip, acts, 3)
        assert (got["steps"] == 1).all() and (got["terminated"] == 1).all()
        assert not got["truncated"].any()
        compare(got, lu.oracle_lookahead(cfg, st, acts), "crashed ego")
    finally:
        hip.close()


# ------------------------------------------------------------------- 4. the handle is untouched
def test_the_next_steps_are_those_of_a_twin_that_never_looked_ahead():
    cfg = make_cfg(E=6, max_episode_steps=5)
    hip, twin = stepped(cfg, 2), stepped(cfg, 2)
    try:
        before = hip.state()
        lu.hip_lookahead(hip, lu.candidates(6, 4), 4)
        lu.hip_lookahead(hip, lu.candidates(6, 4), 4, lazy=True)
        assert np.array_equal(hip.state(), before)
        rng = np.random.default_rng(9)
        for t in range(3):
            a = policy_actions(rng, 6, t)
            for x, y, n in zip(hip.step(a), twin.step(a), HipEnv.STEP_KEYS):
                lu.same_bits(x, y, f"step {t} {n}")
            assert np.array_equal(hip.state(), twin.state())
    finally:
        hip.close()
        twin.close()


# ------------------------------------------------------------------- 5. lazy and the choice
def reordered():
    """the last snapshot of the default case with (0.3, +0.5) held as candidate 0, which crashes
    two egos, one of them on the very step that also truncates every other candidate of its env;
    a third env's ego is crashed by hand, so that none of its candidates is safe"""
    cfg, states = lu.snapshots("default")
    _, E, H, *_ = lu.CASES["default"]
    acts = np.ascontiguousarray(lu.candidates(E, H)[:, [4, 0, 1, 2, 3, 5]])
    st = states[3].copy()
    st[_abi.F_FLAGS][2, 0] |= _abi.FLAG_CRASHED
    return cfg, st, acts, H


def test_lazy_skips_what_a_safe_candidate_0_makes_needless():
    cfg, st, acts, H = reordered()
    full = lu.oracle_lookahead(cfg, st, acts, gamma=0.9)
    skip = lu.not_run_mask(full["terminated"])
    t0 = full["terminated"][:, 0] != 0
    assert t0.any() and not t0.all(), "the case needs both kinds of env"
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(st)
        got = lu.hip_lookahead(hip, acts, H, gamma=0.9, lazy=True)
        compare(got, lu.lazy_expected(full), "lazy")
        assert (got["steps"][skip] == 0).all() and (got["steps"][~skip] >= 1).all()
        one = lu.hip_lookahead(hip, acts[:, :1], H, gamma=0.9, lazy=True)  # K 1: nothing to skip
        compare(one, {k: v[:, :1] for k, v in full.items()}, "lazy, K 1")
    finally:
        hip.close()


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("hold", [False, True])
def test_the_shields_choice(lazy, hold):
    cfg, st, acts, H = reordered()
    if hold:
        acts = np.ascontiguousarray(acts[:, :, 0])
    full = lu.oracle_lookahead(cfg, st, acts, hold=hold, horizon=H)
    want = lu.choose(full["steps"], full["terminated"], lazy=lazy)
    term = full["terminated"] != 0
    assert term.all(1).any(), "no env without a safe candidate"
    assert (want > 0).any() and (want == 0).any()
    hip = HipEnv(cfg)
    try:
        hip.reset()
        hip.set_state(st)
        got = lu.hip_lookahead(hip, acts, H, hold=hold, lazy=lazy,
                               outputs=("steps", "terminated", "truncated", "chosen", "chosen_action"))
        assert got["chosen"].tolist() == want.tolist()
        first = lu.first_actions(acts, hold)
        lu.same_bits(got["chosen_action"], first[np.arange(len(want)), want], "chosen_action")
        only = lu.hip_lookahead(hip, acts, H, hold=hold, lazy=lazy,
                                outputs=("steps", "terminated", "chosen"))
        assert only["chosen"].tolist() == want.tolist()
        for m in ("truncated_unsafe", "last_safe"):
            wrong = lu.choose(full["steps"], full["terminated"], full["truncated"], lazy=lazy,
                              mistake=m)
            assert wrong.tolist() != got["chosen"].tolist(), f"the mistake {m} is not refused"
    finally:
        hip.close()


# ------------------------------------------------------------------- 6. captured
def test_a_captured_call_replayed_after_the_env_stepped_on():
    import torch

    from hwy.native import check, lib

    cfg = make_cfg(E=6, max_episode_steps=6)
    hip = stepped(cfg, 1)
    try:
        acts = lu.candidates(6, 3)
        keep = {}
        lu.hip_lookahead(hip, acts, 3, gamma=0.9, lazy=True, keep=keep,
                         outputs=lu.OUTPUTS + ("chosen", "chosen_action"))
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            check(lib().hwy_lookahead(hip.h, ctypes.byref(keep["args"]),
                                      torch.cuda.current_stream().cuda_stream), "hwy_lookahead")
        rng = np.random.default_rng(4)
        for t in range(2):
            hip.step(policy_actions(rng, 6, t))
            st = hip.state()
            g.replay()
            got = lu.read(keep)
            want = lu.lazy_expected(lu.oracle_lookahead(cfg, st, acts, gamma=0.9))
            compare(got, want, f"replay {t}", lu.OUTPUTS)
            full = lu.oracle_lookahead(cfg, st, acts)
            assert got["chosen"].tolist() == lu.choose(full["steps"], full["terminated"]).tolist()
            assert np.array_equal(hip.state(), st)
    finally:
        hip.close()


# ------------------------------------------------------------------- 7. refusals with a handle
def test_refusals_that_need_a_handle():
    import torch

    from hwy.native import HWY_EINVAL, check, last_error, lib

    cfg = make_cfg(E=4, pe=_abi.PE_RANK, d=4)
    hip = HipEnv(cfg, pe_table_for(_abi.PE_RANK, 4, cfg.obs_vehicles))
    try:
        buf = torch.zeros(4096, device=hip.dev)
        a = _abi.LookaheadArgs()
        a.k, a.horizon, a.gamma, a.actions, a.ret = 2, 2, 1.0, buf.data_ptr(), buf.data_ptr()
        assert lib().hwy_lookahead(hip.h, None, None) == HWY_EINVAL
        a.k = 65
        assert lib().hwy_lookahead(hip.h, ctypes.byref(a), None) == HWY_EINVAL
        a.k = 2
        # seed groups of another geometry leave the per-group tables without meaning: obs is refused,
        # the outputs that read no table are not
        hip.set_seed_groups([1, 2], 2)
        t = np.zeros((2, cfg.obs_vehicles, 4), np.float32)
        check(lib().hwy_set_pe_table(hip.h, t.ctypes.data_as(ctypes.c_void_p), int(t.size)),
              "hwy_set_pe_table")
        hip.set_seed_groups([1, 2, 3, 4], 1)
        assert lib().hwy_lookahead(hip.h, ctypes.byref(a), None) == 0, last_error()
        a.obs = buf.data_ptr()
        assert lib().hwy_lookahead(hip.h, ctypes.byref(a), None) == HWY_EINVAL
        assert "PE tables" in last_error()
        torch.cuda.synchronize()
    finally:
        hip.close()


def test_branch_count_limit():
    from hwy.native import HWY_EINVAL, last_error, lib
    import torch

    cfg = make_cfg(E=(1 << 16) + 1)
    hip = HipEnv(cfg)
    try:
        buf = torch.zeros(16, device=hip.dev)
        a = _abi.LookaheadArgs()
        a.k, a.horizon, a.gamma, a.actions, a.ret = 64, 1, 1.0, buf.data_ptr(), buf.data_ptr()
        assert lib().hwy_lookahead(hip.h, ctypes.byref(a), None) == HWY_EINVAL
        assert "num_envs * k" in last_error()
    finally:
        hip.close()
