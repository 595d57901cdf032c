"""The env's dynamics on the GPU, one simulation frame per step.

Every case of tests/env_util.py::DYN_CASES runs through run_parity: kernel against oracle, every
state word and output bit for bit.  A hook keeps the kernel's state around each step and compares
the after-state directly with tests/dyn_model.py's float64 model of the before-state, within the
bound derived there -- so that check does not pass through the oracle.  tests/test_dyn_model.py
runs the same cases on the CPU oracle, where the branch counts, the 5 % cap on `uncertain` and
the model's sensitivity to every constant are shown without a GPU; counts and cap are asserted
again here from the kernel's run.

One hwy_step_group launch over three of the cases is compared with the solo steps bit for bit.
"""

import ctypes

import numpy as np
import pytest

from env_util import DYN_CASES, GROUPED_DYN, DynChecker, HipEnv, run_parity
from parity_util import diff_state

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", DYN_CASES, ids=[c.name for c in DYN_CASES])
def test_dynamics_case_kernel_equals_oracle_and_model(case):
    cfg = case.make()
    init, action_fn = case.start(cfg)
    ck = DynChecker(case, cfg)
    held = {}

    def actions(rng, E, t):
        held["a"] = np.ascontiguousarray(action_fn(rng, E, t), np.float32)
        return held["a"]

    def after_step(cfg_, hip_out, hip_state, ora_out):
        ck.check(held["state"], held["a"], hip_state, hip_out[1])
        held["state"] = hip_state

    run_parity(cfg, case.steps, seed=case.seed, action_fn=actions, hook=after_step,
               init_state=init, start_hook=lambda st: held.__setitem__("state", st))
    ck.finish()


def test_grouped_launch_of_dynamics_cases_equals_the_solo_steps():
    """Three of the cases (default traffic, 8 lanes, the crafted pairs) in one hwy_step_group
    launch against the same three stepped by hwy_step: every state word after every frame."""
    import torch

    from hwy.native import HwyStepGroupPlan, HwyStepIO, check, lib, ptr

    cases = [c for c in DYN_CASES if c.name in GROUPED_DYN]
    assert len(cases) == 3
    cfgs = [c.make() for c in cases]
    starts = [c.start(cfg) for c, cfg in zip(cases, cfgs)]
    solo = [HipEnv(cfg) for cfg in cfgs]
    grouped = [HipEnv(cfg) for cfg in cfgs]
    n = len(cases)
    try:
        for h, g, (init, _) in zip(solo, grouped, starts):
            for env in (h, g):
                env.reset()
                if init is not None:
                    env.set_state(init)
        dev = grouped[0].dev
        acts = [torch.zeros(h.E, 2, device=dev) for h in grouped]
        io = (HwyStepIO * n)(*[HwyStepIO(ptr(a), ptr(h.obs), ptr(h.rew), ptr(h.term), ptr(h.trunc),
                                         ptr(h.er), ptr(h.el)) for a, h in zip(acts, grouped)])
        hs = (ctypes.c_void_p * n)(*[h.h.value for h in grouped])
        table = torch.empty(int(lib().hwy_step_group_table_bytes(n)), dtype=torch.uint8, device=dev)
        plan = HwyStepGroupPlan()
        check(lib().hwy_step_group_prepare(hs, io, n, table.data_ptr(), ctypes.byref(plan), None),
              "hwy_step_group_prepare")
        rngs = [np.random.default_rng(c.seed) for c in cases]
        for t in range(24):
            a_np = [np.ascontiguousarray(fn(rng, h.E, t), np.float32)
                    for (_, fn), rng, h in zip(starts, rngs, grouped)]
            for a, x in zip(acts, a_np):
                a.copy_(torch.as_tensor(x))
            check(lib().hwy_step_group(ctypes.byref(plan), table.data_ptr(), None), "hwy_step_group")
            torch.cuda.synchronize()
            for i, (s, g, x) in enumerate(zip(solo, grouped, a_np)):
                want, got = s.step(x), g._out()
                for k, w, v in zip(HipEnv.STEP_KEYS, want, got):
                    np.testing.assert_array_equal(v, w, err_msg=f"{cases[i].name} {k} at frame {t}")
                d = diff_state(g.state(), s.state(), s.cfg.vehicles_count + 1)
                assert d is None, f"{cases[i].name} frame {t}: {d}"
    finally:
        for h in solo + grouped:
            h.close()
