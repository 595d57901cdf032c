"""The expected values of hwy_lookahead from the CPU oracle, the shield's choice rule in numpy, the
cases shared by the CPU coverage test and the GPU tests, and a direct C-ABI driver.

A branch is restated independently of the kernel under test: the env's exported state words go
into a one-env OracleEnv with autoreset 0, which is stepped with the branch's actions until the
first done step.  torch and libhwy.so are imported only by `hip_lookahead`.
"""

from __future__ import annotations

import ctypes
from functools import lru_cache

import numpy as np

from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import make_cfg, pe_table_for, policy_actions

OUTPUTS = ("steps", "terminated", "truncated", "rewards", "ret", "ego_final", "obs")
# deliberate mistakes of the expected-value driver, each of which some GPU case must refuse
MISTAKES = ("past_done", "discount_first", "truncated_unsafe", "last_safe", "table_by_branch")


def f32_return(rewards, n, gamma):
    """ret = ret + g * r, g = g * gamma over the first n rewards, every operation in binary32"""
    ret, g, gm = np.float32(0.0), np.float32(1.0), np.float32(gamma)
    for h in range(n):
        ret = np.float32(ret + np.float32(g * np.float32(rewards[h])))
        g = np.float32(g * gm)
    return ret


def oracle_lookahead(cfg, state, actions, *, hold=False, horizon=None, gamma=1.0, tables=None,
                     mistake=None):
    """Every output of hwy_lookahead (but the shield's) for `state` [NFIELDS, E, 64] and
    `actions` ([E, K, H, 2], or [E, K, 2] with hold and `horizon`), from the oracle.
    tables: None, one PE table, or a list of one table per env (seed groups)."""
    actions = np.asarray(actions, np.float32)
    E, K = actions.shape[:2]
    H = int(horizon) if hold else actions.shape[2]
    one = type(cfg).from_buffer_copy(cfg)
    one.num_envs, one.autoreset = 1, 0
    N, Fo = int(cfg.obs_vehicles), cfg.obs_features()
    out = dict(steps=np.zeros((E, K), np.int32), terminated=np.zeros((E, K), np.uint8),
               truncated=np.zeros((E, K), np.uint8), rewards=np.zeros((E, K, H), np.float32),
               ret=np.zeros((E, K), np.float32), ego_final=np.zeros((E, K, 4), np.float32),
               obs=np.zeros((E, K, N, Fo), np.float32))
    for e in range(E):
        for k in range(K):
            if isinstance(tables, (list, tuple)):
                b = e * K + k
                table = tables[b % len(tables)] if mistake == "table_by_branch" else tables[e]
            else:
                table = tables
            ora = OracleEnv(one, table)
            ora.state[...] = state[:, e:e + 1, :]
            n, obs, term, trunc = 0, None, False, False
            for h in range(H):
                a = actions[e, k] if hold else actions[e, k, h]
                obs, rew, term, trunc, _, _ = ora.step(a[None])
                out["rewards"][e, k, h] = rew[0]
                n = h + 1
                if term[0] or trunc[0]:
                    if mistake != "past_done":
                        break
            rw = out["rewards"][e, k]
            if mistake == "discount_first":
                out["ret"][e, k] = np.float32(np.float32(gamma) * f32_return(rw, n, gamma))
            else:
                out["ret"][e, k] = f32_return(rw, n, gamma)
            out["steps"][e, k] = n
            out["terminated"][e, k] = term[0]
            out["truncated"][e, k] = trunc[0]
            st = ora.state
            out["ego_final"][e, k] = [st[f].view(np.float32)[0, 0] for f in
                                      (_abi.F_X, _abi.F_Y, _abi.F_HEADING, _abi.F_SPEED)]
            out["obs"][e, k] = obs[0]
    return out


def not_run_mask(terminated):
    """[E, K] bool: the branches a lazy call skips (k >= 1 of envs whose candidate 0 is safe)"""
    skip = np.repeat((np.asarray(terminated)[:, :1] == 0), np.asarray(terminated).shape[1], 1)
    skip[:, 0] = False
    return skip


def lazy_expected(full):
    """the outputs of a lazy call from those of the full one"""
    skip = not_run_mask(full["terminated"])
    out = {k: v.copy() for k, v in full.items()}
    for k, v in out.items():
        v[skip] = 0
    return out


def choose(steps, terminated, truncated=None, *, lazy=False, mistake=None):
    """The shield's choice [E] int32: the least k with terminated 0, else the k with the most
    steps, the least such k on ties.  (Under lazy a safe candidate 0 hides the rest, which
    changes nothing: it is the least safe k.)"""
    steps, terminated = np.asarray(steps), np.asarray(terminated)
    E, K = steps.shape
    out = np.zeros(E, np.int32)
    for e in range(E):
        unsafe = terminated[e] != 0
        if mistake == "truncated_unsafe":
            unsafe = unsafe | (np.asarray(truncated)[e] != 0)
        safe = np.nonzero(~unsafe)[0]
        if lazy and not unsafe[0]:
            out[e] = 0
        elif len(safe):
            out[e] = safe[-1] if mistake == "last_safe" else safe[0]
        else:
            out[e] = int(np.argmax(steps[e]))  # the first of the greatest
    return out


def first_actions(actions, hold):
    """[E, K, 2]: every candidate's first-step action"""
    a = np.asarray(actions, np.float32)
    return a if hold else a[:, :, 0]


# ------------------------------------------------------------------------------- the cases
HELD = ((0.0, 0.0), (-1.0, 0.0), (1.0, 0.0), (0.3, -0.5), (0.3, 0.5))


def candidates(E, H):
    """[E, 6, H, 2]: idle, full brake, full throttle, (0.3, -0.5) and (0.3, +0.5) held, and one
    tanh(2 N(0, 1)) sequence per env from default_rng(0)"""
    a = np.zeros((E, len(HELD) + 1, H, 2), np.float32)
    for k, v in enumerate(HELD):
        a[:, k] = np.asarray(v, np.float32)
    a[:, len(HELD)] = np.tanh(2.0 * np.random.default_rng(0).normal(size=(E, H, 2))).astype(np.float32)
    return a


CASES = {
    # name: (make_cfg keywords, E, H, snapshots before these policy steps, least terminated,
    #        least truncated, least full-horizon)
    "default": (dict(max_episode_steps=6), 8, 4, (0, 1, 3, 5), 10, 10, 10),
    "policy_frequency-5": (dict(max_episode_steps=6, policy_frequency=5), 8, 4, (0, 1, 3), 5, 1, 1),
    "lanes2-V31": (dict(lanes_count=2, vehicles_count=30, max_episode_steps=8), 8, 3, (0, 3, 6),
                   10, 1, 1),
}


@lru_cache(maxsize=None)
def snapshots(name, **extra):
    """The case's states on the oracle: an autoreset policy_actions run from default_rng(0),
    copied before the listed policy steps.  Returns (cfg, [state, ...]); shared, left unchanged."""
    kw, E, H, snaps, *_ = CASES[name]
    cfg = make_cfg(E=E, autoreset=True, **dict(kw, **dict(extra)))
    ora = OracleEnv(cfg, case_table(cfg))
    ora.reset()
    rng = np.random.default_rng(0)
    states = []
    for t in range(max(snaps) + 1):
        if t in snaps:
            states.append(ora.state.copy())
        ora.step(policy_actions(rng, E, t))
    return cfg, states


def case_table(cfg, seed=3):
    if cfg.pe_kind == _abi.PE_NONE or cfg.d_embed <= 0:
        return None
    return pe_table_for(cfg.pe_kind, cfg.d_embed, cfg.obs_vehicles, seed=seed)


_EXPECTED = {}


def expected(name, gamma=1.0):
    """[(state, actions [E, 6, H, 2], oracle outputs)] per snapshot of the case; computed once"""
    if (name, gamma) not in _EXPECTED:
        cfg, states = snapshots(name)
        _, E, H, *_ = CASES[name]
        acts = candidates(E, H)
        _EXPECTED[name, gamma] = [(st, acts, oracle_lookahead(cfg, st, acts, gamma=gamma))
                                  for st in states]
    return _EXPECTED[name, gamma]


def coverage(name):
    """(terminated, truncated, full horizon, done on the first step, branches) over the case"""
    _, E, H, *_ = CASES[name]
    t = tr = full = first = total = 0
    for _, _, out in expected(name):
        term, trunc, steps = out["terminated"] != 0, out["truncated"] != 0, out["steps"]
        t += int(term.sum())
        tr += int((trunc & ~term).sum())
        full += int((~term & ~trunc).sum())
        first += int(((term | trunc) & (steps == 1)).sum())
        total += steps.size
    return t, tr, full, first, total


# ------------------------------------------------------------------------------- the GPU driver
SENTINEL = {"steps": -77, "terminated": 0xEE, "truncated": 0xEE, "rewards": -7.5, "ret": -7.5,
            "ego_final": -7.5, "obs": -7.5, "chosen": -77, "chosen_action": -7.5}
PAD = 16


def hip_lookahead(hip, actions, horizon, *, hold=False, lazy=False, gamma=1.0, outputs=OUTPUTS,
                  stream=None, keep=None):
    """hwy_lookahead on env_util.HipEnv `hip` through the C ABI.  Each output sits in the middle of
    a sentinel-filled buffer with PAD elements on either side, which are checked to be intact.
    Returns the outputs as numpy arrays.  keep (a dict): receives the device tensors (for graph
    replays: call `read(keep)` after a replay)."""
    import torch

    from hwy.native import check, lib

    dev = hip.dev
    a = torch.as_tensor(np.ascontiguousarray(actions, np.float32), device=dev)
    E, K = a.shape[:2]
    H = int(horizon)
    N, Fo = hip.N, hip.Fo
    shapes = {"steps": ((E, K), torch.int32), "terminated": ((E, K), torch.uint8),
              "truncated": ((E, K), torch.uint8), "rewards": ((E, K, H), torch.float32),
              "ret": ((E, K), torch.float32), "ego_final": ((E, K, 4), torch.float32),
              "obs": ((E, K, N, Fo), torch.float32), "chosen": ((E,), torch.int32),
              "chosen_action": ((E, 2), torch.float32)}
    args = _abi.LookaheadArgs()
    args.k, args.horizon, args.hold, args.lazy, args.gamma = K, H, int(hold), int(lazy), gamma
    args.actions = a.data_ptr()
    bufs = {}
    for name in outputs:
        shape, dtype = shapes[name]
        n = int(np.prod(shape))
        buf = torch.full((n + 2 * PAD,), SENTINEL[name], dtype=dtype, device=dev)
        bufs[name] = (buf, shape)
        setattr(args, name, buf.data_ptr() + PAD * buf.element_size())
    check(lib().hwy_lookahead(hip.h, ctypes.byref(args), stream), "hwy_lookahead")
    if keep is not None:
        keep.update(bufs=bufs, actions=a, args=args)
        return None
    return read(dict(bufs=bufs))


def read(keep):
    import torch

    torch.cuda.synchronize()
    out = {}
    for name, (buf, shape) in keep["bufs"].items():
        h = buf.cpu().numpy()
        s = np.asarray(SENTINEL[name], h.dtype)
        assert (h[:PAD] == s).all() and (h[-PAD:] == s).all(), f"{name}: a word outside the output was written"
        out[name] = h[PAD:-PAD].reshape(shape).copy()
    return out


def same_bits(got, want, msg):
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape, f"{msg}: shape {got.shape} != {want.shape}"
    if got.dtype == np.float32:
        got, want = got.view(np.uint32), np.ascontiguousarray(want, np.float32).view(np.uint32)
    bad = np.argwhere(got != want)
    assert not len(bad), f"{msg}: {len(bad)} entries differ, first at {bad[0].tolist()}"


def differs(got, want, names):
    """True if some output in `names` differs in bits: a mistaken driver refused"""
    for n in names:
        g, w = np.ascontiguousarray(got[n]), np.ascontiguousarray(want[n]).astype(got[n].dtype)
        if g.dtype == np.float32:
            g, w = g.view(np.uint32), w.view(np.uint32)
        if not np.array_equal(g, w):
            return True
    return False
