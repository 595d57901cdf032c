"""The env step across hwy_config's switches, not just HIGHWAY_CONFIG as shipped.

Every case of tests/env_util.py::CASES runs through run_parity: kernel against oracle, every
state word and output bit-equal, as tests/test_env_parity_gpu.py does at the default config.  A
hook also compares the kernel's outputs directly with tests/env_model.py, a float64 numpy
restatement that shares no code with hwy_math.h or the oracle, within the bound derived there
-- so that check does not pass through the oracle.  tests/test_env_model.py runs the same
cases with the same actions on the CPU oracle, where each case's "must occur" count and the
5 % cap on what `uncertain` leaves out are shown to hold without a GPU; they are asserted
again here from the kernel's run.

Two more tests carry a non-default config through the paths that hold a copy of it: the grouped
launch's device table and the info / final variants of the step kernel.
"""

import ctypes

import numpy as np
import pytest

from env_util import ALL8, CASES, Case, Checker, HipEnv, run_parity, swerve, wild
from hwy import _abi
from parity_util import diff_state, policy_actions

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_config_case_kernel_equals_oracle_and_model(case):
    cfg, table = case.make()
    ck = Checker(case, cfg, table)
    run_parity(cfg, case.steps, table=table, seed=case.seed, action_fn=case.actions,
               hook=lambda cfg_, hip_out, hip_state, ora_out: ck.check(hip_out, hip_state))
    ck.finish()


def test_grouped_step_of_unlike_configs_equals_each_handles_own():
    """Three handles of unlike configs (see_behind with 8 features; off-road termination on 2
    lanes; 5 policy steps a second with DIST1) in one hwy_step_group launch against the same
    three stepped by hwy_step: the grouped table's copy of each config is the handle's."""
    import torch

    from hwy.native import HwyStepGroupPlan, HwyStepIO, check, lib, ptr

    specs = [Case("g-see_behind-8", dict(order="shuffled", observation=dict(see_behind=True, features=ALL8),
                                         max_episode_steps=6), E=5, actions=wild, autoreset=True),
             Case("g-off-road", dict(offroad_terminal=True, lanes_count=2, max_episode_steps=6),
                  E=7, actions=swerve, autoreset=True),
             Case("g-frames-dist1", dict(policy_frequency=5, pe=_abi.PE_DIST1, d=4,
                                         max_episode_steps=6), E=3, actions=policy_actions,
                  autoreset=True)]
    made = [s.make() for s in specs]
    solo = [HipEnv(cfg, table) for cfg, table in made]
    grouped = [HipEnv(cfg, table) for cfg, table in made]
    n = len(specs)
    try:
        for h in solo + grouped:
            h.reset()
        dev = grouped[0].dev
        acts = [torch.zeros(h.E, 2, device=dev) for h in grouped]
        io = (HwyStepIO * n)(*[HwyStepIO(ptr(a), ptr(h.obs), ptr(h.rew), ptr(h.term), ptr(h.trunc),
                                         ptr(h.er), ptr(h.el)) for a, h in zip(acts, grouped)])
        hs = (ctypes.c_void_p * n)(*[h.h.value for h in grouped])
        table = torch.empty(int(lib().hwy_step_group_table_bytes(n)), dtype=torch.uint8, device=dev)
        plan = HwyStepGroupPlan()
        check(lib().hwy_step_group_prepare(hs, io, n, table.data_ptr(), ctypes.byref(plan), None),
              "hwy_step_group_prepare")
        rng = np.random.default_rng(0)
        dones = [0] * n
        for t in range(10):
            a_np = [s.actions(rng, h.E, t) for s, h in zip(specs, grouped)]
            for a, x in zip(acts, a_np):
                a.copy_(torch.as_tensor(x))
            check(lib().hwy_step_group(ctypes.byref(plan), table.data_ptr(), None), "hwy_step_group")
            torch.cuda.synchronize()
            for i, (s, g, x) in enumerate(zip(solo, grouped, a_np)):
                want, got = s.step(x), g._out()
                for k, w, v in zip(HipEnv.STEP_KEYS, want, got):
                    np.testing.assert_array_equal(v, w, err_msg=f"handle {i} {k} at step {t}")
                d = diff_state(g.state(), s.state(), s.cfg.vehicles_count + 1)
                assert d is None, f"handle {i} step {t}: {d}"
                dones[i] += int((want[2] | want[3]).sum())
        assert all(d >= h.E for d, h in zip(dones, solo)), dones  # every env was autoreset
    finally:
        for h in solo + grouped:
            h.close()


def test_info_and_final_variants_under_a_non_default_config():
    """hwy_step_with_final with info under see_behind, absolute, shuffled, an unnormalised
    reward and 5-step episodes: the step is hwy_step's, the four reward terms are the model's,
    and each final_obs row is what a handle with autoreset off writes to obs from that state."""
    kw = dict(order="shuffled", observation=dict(see_behind=True, absolute=True),
              normalize_reward=False, max_episode_steps=5, vehicles_density=3)
    case = Case("info-final", kw, E=16, actions=wild, autoreset=True)
    cfg, table = case.make()
    twin_cfg, _ = Case("twin", kw, E=16, autoreset=False).make()
    plain, final, twin = HipEnv(cfg), HipEnv(cfg), HipEnv(twin_cfg)
    ck = Checker(case, twin_cfg, table)
    V = cfg.vehicles_count + 1
    rng = np.random.default_rng(5)
    crashes = truncations = 0
    try:
        plain.reset()
        final.reset()
        for t in range(12):
            a = case.actions(rng, cfg.num_envs, t)
            twin.set_state(final.state())  # the twin steps from the same state, without the reset
            want = plain.step(a)
            out = final.step_final(a)
            tw = twin.step(a)
            for k, w in zip(HipEnv.STEP_KEYS, want):
                np.testing.assert_array_equal(out[k], w, err_msg=f"{k} at step {t}")
            d = diff_state(final.state(), plain.state(), V)
            assert d is None, f"step {t}: {d}"
            # the terms are of the state before the autoreset, which the twin still holds
            twin_state = twin.state()
            ck.check_terms(out["rewards"], twin_state)
            ck.check(tw, twin_state)
            np.testing.assert_array_equal(out["rew"], tw[1])
            done = (out["term"] | out["trunc"]).astype(bool)
            np.testing.assert_array_equal(out["final_obs"][done], tw[0][done],
                                          err_msg=f"final_obs at step {t}")
            assert np.isnan(out["final_obs"][~done]).all(), "a row of an env that is not done was written"
            np.testing.assert_array_equal(out["obs"][~done], tw[0][~done])
            final.final_obs.fill_(float("nan"))
            crashes += int(out["term"].sum())
            truncations += int((out["trunc"] & ~out["term"]).sum())
        print(ck.report(), f"terms {ck.worst['terms']}; crashes {crashes} truncations {truncations}")
        assert crashes >= 1 and truncations >= 16
        assert ck.left_out <= 0.05 * ck.pairs
    finally:
        for h in (plain, final, twin):
            h.close()
