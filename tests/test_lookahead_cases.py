"""hwy_lookahead's cases on the CPU oracle alone: the shield's choice rule against an exhaustive
restatement, the binary32 return, the lazy image, and the coverage the GPU tests rely on (how many
branches end terminated, truncated, or run the full horizon).

The oracle's figures for the cases of tests/lookahead_util.py (printed by the coverage test):
default 27 terminated / 76 truncated / 89 full horizon of 192, 38 done on their first step;
policy_frequency-5 7 / 44 / 93 of 144; lanes2-V31 31 / 24 / 89 of 144."""

from __future__ import annotations

import itertools

import numpy as np
import pytest

import lookahead_util as lu
from hwy import _abi


def brute_choice(steps, term, lazy):
    """the rule of include/hwy.h, word for word, for one env"""
    K = len(steps)
    if lazy and term[0] == 0:
        return 0
    safe = [k for k in range(K) if term[k] == 0]
    if safe:
        return min(safe)
    most = max(steps)
    return min(k for k in range(K) if steps[k] == most)


@pytest.mark.parametrize("lazy", [False, True])
@pytest.mark.parametrize("K", [1, 2, 3, 4])
def test_choice_rule_on_exhaustive_tables(K, lazy):
    rows = []
    for steps in itertools.product((1, 2, 3), repeat=K):
        for term in itertools.product((0, 1), repeat=K):
            s, t = list(steps), list(term)
            if lazy and t[0] == 0:  # what a lazy call writes for the skipped candidates
                s[1:], t[1:] = [0] * (K - 1), [0] * (K - 1)
            rows.append((s, t))
    steps = np.array([r[0] for r in rows], np.int32)
    term = np.array([r[1] for r in rows], np.uint8)
    got = lu.choose(steps, term, lazy=lazy)
    want = [brute_choice(s, t, lazy) for s, t in rows]
    assert got.tolist() == want
    # lazy or not, the choice over the full tables is the same
    if lazy:
        full_steps = np.array(list(itertools.product((1, 2, 3), repeat=K)), np.int32)
        for term_row in itertools.product((0, 1), repeat=K):
            t = np.tile(np.array(term_row, np.uint8), (len(full_steps), 1))
            lz = lu.lazy_expected(dict(steps=full_steps, terminated=t))
            assert np.array_equal(lu.choose(lz["steps"], lz["terminated"], lazy=True),
                                  lu.choose(full_steps, t))


def test_choice_mistakes_differ_from_the_rule():
    steps = np.array([[3, 3, 3], [1, 2, 2]], np.int32)
    term = np.array([[1, 0, 0], [1, 1, 1]], np.uint8)
    trunc = np.array([[0, 1, 0], [0, 0, 0]], np.uint8)
    assert lu.choose(steps, term, trunc).tolist() == [1, 1]
    assert lu.choose(steps, term, trunc, mistake="last_safe").tolist() == [2, 1]
    assert lu.choose(steps, term, trunc, mistake="truncated_unsafe").tolist() == [2, 1]


def test_binary32_return():
    r = np.array([0.7, 0.8, 0.9, 0.1], np.float32)
    acc = np.float32(0)
    for x in r[:3]:
        acc = np.float32(acc + x)
    assert lu.f32_return(r, 3, 1.0) == acc          # gamma 1: the step's own running return
    assert lu.f32_return(r, 3, 0.0) == r[0]         # 0^0 = 1: the first reward is not discounted
    g = np.float32(0.9)
    want = np.float32(np.float32(r[0] + np.float32(g * r[1])) + np.float32(np.float32(g * g) * r[2]))
    assert lu.f32_return(r, 3, 0.9) == want
    assert lu.f32_return(r, 0, 0.9) == 0.0


@pytest.mark.parametrize("name", list(lu.CASES))
def test_coverage_of_the_gpu_cases(name):
    kw, E, H, snaps, least_term, least_trunc, least_full = lu.CASES[name]
    term, trunc, full, first, total = lu.coverage(name)
    print(f"{name}: {term} terminated, {trunc} truncated, {full} full horizon of {total}; "
          f"{first} done on their first step")
    assert total == E * 6 * len(snaps) and term + trunc + full == total
    assert term >= least_term and trunc >= least_trunc and full >= least_full
    if name == "default":
        assert total == 192 and min(term, trunc, full) >= 10 and first >= 10
    for st, acts, out in lu.expected(name):
        steps = out["steps"]
        assert steps.min() >= 1 and steps.max() <= H
        done = (out["terminated"] != 0) | (out["truncated"] != 0)
        assert (steps[~done] == H).all()
        # rewards past `steps` are +0.0 and the return at gamma 1 is the running sum
        for e, k in np.ndindex(*steps.shape):
            assert not out["rewards"][e, k, steps[e, k]:].view(np.uint32).any()
            assert out["ret"][e, k] == lu.f32_return(out["rewards"][e, k], steps[e, k], 1.0)
        # truncation is the step count's: the env's step word plus the steps run
        step0 = st[_abi.F_ENV][:, _abi.E_STEP].astype(np.int64)[:, None]
        max_steps = kw["max_episode_steps"]
        assert np.array_equal(out["truncated"] != 0, step0 + steps >= max_steps)


def test_the_default_case_has_an_env_without_a_safe_candidate_or_needs_crafting():
    """the shield test needs one env whose candidates all terminate; say whether the natural run
    has one (the GPU test crafts one with import_state otherwise)"""
    none_safe = sum(int((out["terminated"] != 0).all(1).sum()) for _, _, out in lu.expected("default"))
    some_unsafe = sum(int(((out["terminated"] != 0).any(1)).sum()) for _, _, out in lu.expected("default"))
    print(f"envs with no safe candidate: {none_safe}; with an unsafe one: {some_unsafe}")
    assert some_unsafe >= 1


def test_mistaken_drivers_differ_on_the_oracle():
    """each deliberate mistake changes some expected value of the default case, so a kernel that
    agrees with the right driver refuses the mistaken one"""
    cfg, states = lu.snapshots("default")
    _, E, H, *_ = lu.CASES["default"]
    acts = lu.candidates(E, H)
    changed = {m: False for m in ("past_done", "discount_first")}
    for st in states:
        right = lu.oracle_lookahead(cfg, st, acts, gamma=0.9)
        for m in changed:
            wrong = lu.oracle_lookahead(cfg, st, acts, gamma=0.9, mistake=m)
            changed[m] |= lu.differs(right, wrong, lu.OUTPUTS)
    assert all(changed.values()), changed
