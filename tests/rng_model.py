"""A numpy restatement of what decides which world an episode is: Philox4x32-10, the draws
built on it, the seed schedule, the reset state and the `shuffled` permutation.

Independent of csrc/hwy_math.h, oracle/hwy_oracle.c and libhwy.so: uint64 / float64 numpy only.
The sources are the round function of Salmon et al. (SC'11, "Parallel random numbers: as easy
as 1, 2, 3"), include/hwy.h (the schedule, the state layout), SURVEY.md §8 a1.9 with its erratum
and the constant table of DESIGN.md §4 (`Vehicle.create_random`, `randomize_behavior`, the
lane-change timer at creation).

  * the reset draws of vehicle i: philox(counter (i, 0, 0, 'RST1'), key = the episode's seed as
    (low word, high word)); word 0 -> lane = choice(lanes), word 1 -> speed, word 2 -> the
    spacing jitter, word 3 -> the IDM exponent;
  * the shuffle key of slot q: word 0 of philox(counter (q, step, 0, 'SHUF'), key = seed); slot q
    (the row 1 + q before the shuffle) goes to row 1 + rank(key_q), ties to the lower slot;
  * u01 = (u >> 8) * 2^-24, uniform(lo, hi) = lo + (hi - lo) * u01, choice(n) = (u * n) >> 32.

Integers are exact.  Floats are `env_model.Q` values whose bound is derived as there: 2^-24 *
|intermediate| per float32 operation (a float32 literal that stands for a real number counts as
one), plus EXP_REL for the device exp (test_device_math_accuracy_against_libm pins 3e-7); the
comparison allows TOL_FACTOR = 2 times that.  Where the derivation leaves one correctly rounded
operation on exact operands (the IDM exponent 3.5 + u01, y = 4 * lane) the bound is 0: equal.

`RngModel(mut=...)` is the model with one deliberate mistake (MUTATIONS), for the test that
shows each of them is refused by at least one case.
"""

from __future__ import annotations

import numpy as np

import env_model as em
from env_model import Q, U
from hwy import _abi

EXP_REL = 3e-7                # device exp, relative (test_device_math_accuracy_against_libm)
DOMAIN_RESET = 0x52535431     # 'RST1'
DOMAIN_SHUFFLE = 0x53485546   # 'SHUF'
PI32 = float(np.float32(np.pi))
_M32 = np.uint64(0xFFFFFFFF)
_E_NWORDS = 7                 # enum hwy_env_word: the words of HWY_F_ENV in use

MUTATIONS = (
    "reset-index-in-word-1",            # reset counter (0, i, 0, 'RST1')
    "reset-domain-in-word-2",           # reset counter (i, 0, 'RST1', 0)
    "shuffle-slot-and-step-swapped",    # shuffle counter (step, q, 0, 'SHUF')
    "shuffle-domain-in-word-2",         # shuffle counter (q, step, 'SHUF', 0)
    "domains-swapped",                  # 'SHUF' keys the reset, 'RST1' the shuffle
    "high-key-dropped",                 # key (seed & 2^32 - 1, 0)
    "u01-shift-9",                      # 23 bits: (u >> 9) * 2^-23
    "tie-to-higher-slot",               # equal keys: the higher slot first
    "schedule-without-plus-1", "schedule-without-stride", "schedule-without-env_offset",
    "group-l-is-e",                     # a group's local index l replaced by the env index e
    "x-without-running-max",            # every other car placed from the ego, not from the last
    "delta-and-jitter-words-swapped",   # delta from word 2, jitter from word 3
    "shuffle-step-fixed-at-0",
)


def philox4x32_10(ctr, key):
    """ctr [..., 4], key [..., 2] (broadcast against each other) -> [..., 4] uint32 words, as
    uint64 arrays.  Ten rounds of: (hi0, lo0) = M0 * c0, (hi1, lo1) = M1 * c2,
    c = (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key is bumped by the Weyl constants between
    rounds."""
    ctr = np.asarray(ctr, np.uint64) & _M32
    key = np.asarray(key, np.uint64) & _M32
    shape = np.broadcast_shapes(ctr.shape[:-1], key.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(ctr[..., i], shape).copy() for i in range(4))
    k0, k1 = (np.broadcast_to(key[..., i], shape).copy() for i in range(2))
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    w0, w1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
    s32 = np.uint64(32)
    for r in range(10):
        if r:
            k0 = (k0 + w0) & _M32
            k1 = (k1 + w1) & _M32
        p0, p1 = m0 * c0, m1 * c2          # 32 x 32 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & _M32, (p0 >> s32) ^ c3 ^ k1, p0 & _M32
    return np.stack([c0, c1, c2, c3], -1)


def seeds_u64(seeds):
    """any integers (Python ints beyond 2^63 included) as uint64, wrapped"""
    return np.array([int(s) % (1 << 64) for s in np.asarray(seeds, object).ravel()], np.uint64)


def state_seeds(state):
    """the current episode's seed of every env, from the packed state's words: [E] uint64"""
    ew = state[_abi.F_ENV]
    return ew[:, _abi.E_SEED_LO].astype(np.uint64) | (ew[:, _abi.E_SEED_HI].astype(np.uint64) << np.uint64(32))


class RngModel:
    def __init__(self, mut: str = ""):
        assert mut == "" or mut in MUTATIONS, mut
        self.mut = mut

    # ---- draws
    def u01(self, u):
        """24 random bits: exact in float32, always < 1"""
        u = np.asarray(u, np.uint64)
        if self.mut == "u01-shift-9":
            return (u >> np.uint64(9)).astype(np.float64) * 2.0 ** -23
        return (u >> np.uint64(8)).astype(np.float64) * 2.0 ** -24

    def uniform(self, u, lo, hi) -> Q:
        """lo + (hi - lo) * u01 in float32: three operations"""
        lo, hi = Q.of(lo), Q.of(hi)
        return lo + (hi - lo) * Q(self.u01(u))

    @staticmethod
    def choice(u, n):
        return ((np.asarray(u, np.uint64) * np.uint64(n)) >> np.uint64(32)).astype(np.int64)

    def _key(self, seeds):
        s = np.asarray(seeds, np.uint64)
        hi = np.zeros_like(s) if self.mut == "high-key-dropped" else s >> np.uint64(32)
        return np.stack([s & _M32, hi], -1)

    def reset_words(self, seeds, V):
        """[E, V, 4]: the four words of every vehicle's reset draw"""
        i = np.arange(V, dtype=np.uint64)
        z = np.zeros(V, np.uint64)
        dom = np.full(V, DOMAIN_SHUFFLE if self.mut == "domains-swapped" else DOMAIN_RESET, np.uint64)
        ctr = {"reset-index-in-word-1": (z, i, z, dom),
               "reset-domain-in-word-2": (i, z, dom, z)}.get(self.mut, (i, z, z, dom))
        return philox4x32_10(np.stack(ctr, -1)[None], self._key(seeds)[:, None, :])

    def shuffle_keys(self, n, seeds, step):
        """[E, n]: the sort key of every slot at the env's step"""
        seeds = np.asarray(seeds, np.uint64)
        E = seeds.shape[0]
        q = np.broadcast_to(np.arange(n, dtype=np.uint64), (E, n))
        st = np.broadcast_to(np.asarray(step, np.uint64).reshape(-1, 1) & _M32, (E, n))
        if self.mut == "shuffle-step-fixed-at-0":
            st = np.zeros_like(st)
        z = np.zeros((E, n), np.uint64)
        dom = np.full((E, n), DOMAIN_RESET if self.mut == "domains-swapped" else DOMAIN_SHUFFLE,
                      np.uint64)
        ctr = {"shuffle-slot-and-step-swapped": (st, q, z, dom),
               "shuffle-domain-in-word-2": (q, st, dom, z)}.get(self.mut, (q, st, z, dom))
        return philox4x32_10(np.stack(ctr, -1), self._key(seeds)[:, None, :])[..., 0]

    def shuffle_dest(self, N, seeds, step):
        """[E, N - 1]: the observation row slot q (row 1 + q before the shuffle) is moved to:
        1 + the rank of its key among the N - 1 keys, ties to the lower slot.  N <= 2: identity."""
        seeds = np.asarray(seeds, np.uint64)
        n = max(N - 1, 0)
        if N <= 2:
            return np.broadcast_to(1 + np.arange(n), (seeds.shape[0], n)).copy()
        key = self.shuffle_keys(n, seeds, step)
        q = np.arange(n)
        first = q[None, :] > q[:, None] if self.mut == "tie-to-higher-slot" else q[None, :] < q[:, None]
        # before[e, q, p]: slot p stands before slot q
        before = (key[:, None, :] < key[:, :, None]) | ((key[:, None, :] == key[:, :, None]) & first[None])
        return 1 + before.sum(-1)

    # ---- the schedule
    def schedule_seed(self, cfg, e, k, group_bases=None, group_envs=None):
        """seed(env e, episode k) = seed_base + env_offset + e + 1 + seed_stride * k (include/hwy.h),
        with seed groups seed_bases[e // group_envs] + env_offset + (e % group_envs) + 1 +
        seed_stride * k; two's-complement wrap to uint64.  e and k broadcast; Python integers."""
        e, k = np.broadcast_arrays(np.asarray(e, object), np.asarray(k, object))
        out = np.empty(e.shape, np.uint64)
        for idx in np.ndindex(e.shape):
            ee, kk = int(e[idx]), int(k[idx])
            if group_bases is None:
                base, l = int(cfg.seed_base), ee
            else:
                base = int(group_bases[ee // group_envs])
                l = ee if self.mut == "group-l-is-e" else ee % group_envs
            s = base
            s += 0 if self.mut == "schedule-without-env_offset" else int(cfg.env_offset)
            s += l + (0 if self.mut == "schedule-without-plus-1" else 1)
            s += 0 if self.mut == "schedule-without-stride" else int(cfg.seed_stride) * kk
            out[idx] = s % (1 << 64)
        return out

    # ---- the reset
    def reset_state(self, cfg, seeds):
        """The state hwy_reset leaves for episodes of the given seeds [E], every field [E, 64]:
        int64 `lane`, `target_lane`, `flags` (present, and the road order in bits 8-13: a fresh
        road is in index order); Q `x`, `y`,
        `speed`, `target_speed`, `delta`, `heading`; the words of absent slots are zero.  The
        timer is not here: `check_timer` compares it from the stored x and y."""
        seeds = np.asarray(seeds, np.uint64)
        E, V, lanes = seeds.shape[0], int(cfg.vehicles_count) + 1, int(cfg.lanes_count)
        w = self.reset_words(seeds, V)
        ego = (np.arange(V) == 0)[None, :]
        lane = self.choice(w[..., 0], lanes)
        if cfg.initial_lane_id >= 0:
            lane = np.where(ego, int(cfg.initial_lane_id), lane)
        lim = Q(float(cfg.speed_limit))
        c07, c08 = Q(0.7, U * 0.7), Q(0.8, U * 0.8)           # float32 literals
        speed = self.uniform(w[..., 1], c07 * lim, c08 * lim).where(~ego, Q(np.full((E, V), 25.0)))
        spacing = (Q(1.0) / Q(float(cfg.vehicles_density))).where(
            ~ego, Q(np.full((E, V), float(cfg.ego_spacing))))
        fac = (Q(-5.0 / 40.0) * Q(float(lanes)))._through(np.exp, EXP_REL)
        offset = spacing * (Q(12.0) + speed) * fac
        jw, dw = (3, 2) if self.mut == "delta-and-jitter-words-swapped" else (2, 3)
        inc = offset * self.uniform(w[..., jw], Q(0.9, U * 0.9), Q(1.1, U * 1.1))
        xs = [Q(3.0) * offset[:, 0] + inc[:, 0]]
        mx = xs[0]
        for i in range(1, V):
            base = xs[0] if self.mut == "x-without-running-max" else mx
            xs.append(base + inc[:, i])
            mx = mx.maximum(xs[-1])
        x = em.qstack(xs)
        # uniform(3.5, 4.5): hi - lo = 1 and the product by it are exact, so the exponent is the
        # one rounding of the exact 3.5 + u01: bound 0 (this is what tells 24 bits from 23)
        delta = Q((3.5 + self.u01(w[..., dw])).astype(np.float32).astype(np.float64)).where(
            ~ego, Q(np.zeros((E, V))))

        def pad(a):
            if isinstance(a, Q):
                return Q(pad(a.v), pad(a.e))
            out = np.zeros((E, 64), a.dtype)
            out[:, :V] = a
            return out

        here = np.arange(64) < V
        flags = np.where(here, (np.arange(64) << _abi.FLAG_ORDER_SHIFT) | _abi.FLAG_PRESENT, 0)
        return dict(lane=pad(lane), target_lane=pad(lane), y=pad(Q(4.0 * lane)), speed=pad(speed),
                    target_speed=pad(speed), x=pad(x), delta=pad(delta),
                    heading=Q(np.zeros((E, 64))), flags=np.broadcast_to(flags, (E, 64)).astype(np.int64))


# the model as it is, as plain functions
_MODEL = RngModel()
u01, uniform, choice = _MODEL.u01, _MODEL.uniform, _MODEL.choice
schedule_seed, reset_state, shuffle_dest = _MODEL.schedule_seed, _MODEL.reset_state, _MODEL.shuffle_dest

FLOAT_FIELDS = dict(x=_abi.F_X, y=_abi.F_Y, speed=_abi.F_SPEED, target_speed=_abi.F_TSPEED,
                    delta=_abi.F_DELTA, heading=_abi.F_HEADING)
INT_FIELDS = dict(lane=_abi.F_LANE, target_lane=_abi.F_TLANE, flags=_abi.F_FLAGS)


def timer_model(cfg, state) -> Q:
    """The MOBIL timer at creation from the STORED x and y: frac((x + y) * float32(pi)), with the
    bound of its one sum and one product (the subtraction of the floor is exact).  Compared on
    the circle (check_fresh): x's own error times pi would cross the wrap.  The ego's and the
    absent slots' timers are 0."""
    V = int(cfg.vehicles_count) + 1
    x = state[_abi.F_X].view(np.float32).astype(np.float64)
    y = state[_abi.F_Y].view(np.float32).astype(np.float64)
    t = (Q(x) + Q(y)) * Q(PI32)
    other = (np.arange(64) >= 1) & (np.arange(64) < V)
    return Q(t.v - np.floor(t.v), t.e).where(np.broadcast_to(other, x.shape), Q(np.zeros_like(x)))


def check_fresh(cfg, state, envs, seeds=None, model=None, episode=None, worst=None):
    """The packed state's envs `envs` (indices or a bool mask) hold freshly reset episodes:
    every field against model.reset_state of the seed in their state words (or `seeds`, [len
    envs], which the words must then equal), step 0, return 0, ego action 0, no impact.
    `episode` (optional) is the expected E_EPISODE word.  `worst` (optional dict) collects
    field -> (error, allowed) of the entry with the largest ratio."""
    model = model or RngModel()
    envs = np.arange(state.shape[1])[np.asarray(envs)]
    if not len(envs):
        return
    st = state[:, envs]
    got_seeds = state_seeds(st)
    if seeds is not None:
        want = seeds_u64(seeds)
        assert (got_seeds == want).all(), (
            f"seed words of envs {envs[got_seeds != want].tolist()}: {got_seeds[got_seeds != want]} "
            f"!= {want[got_seeds != want]}")
    ref = model.reset_state(cfg, got_seeds if seeds is None else seeds_u64(seeds))
    for name, f in INT_FIELDS.items():
        got = st[f].astype(np.int64)
        bad = got != ref[name]
        assert not bad.any(), (f"{name} at (env, vehicle) {[int(envs[np.argwhere(bad)[0][0]]), int(np.argwhere(bad)[0][1])]}: "
                               f"got {got[bad][0]}, model {ref[name][bad][0]}")
    fl = {name: st[f].view(np.float32).astype(np.float64) for name, f in FLOAT_FIELDS.items()}
    q = dict(ref)
    fl["timer"] = st[_abi.F_TIMER].view(np.float32).astype(np.float64)
    q["timer"] = timer_model(cfg, st)
    for name, got in fl.items():
        err = np.abs(got - q[name].v)
        if name == "timer":
            err = np.minimum(err, 1.0 - err)     # on the circle
        tol = em.TOL_FACTOR * q[name].e
        k = np.unravel_index(int(np.argmax(err - tol)), err.shape)
        assert err[k] <= tol[k], (f"{name} at (env, vehicle) {[int(envs[k[0]]), int(k[1])]}: got {got[k]!r}, model "
                                  f"{q[name].v[k]!r}, error {err[k]:.3g} > bound {tol[k]:.3g}")
        if worst is not None:
            ratio = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), 0.0)
            k = np.unravel_index(int(np.argmax(ratio)), err.shape)
            w = worst.get(name, (0.0, 0.0))
            if w[1] == 0.0 or ratio[k] > w[0] / w[1]:
                worst[name] = (float(err[k]), float(tol[k]))
    for f in (_abi.F_IMPX, _abi.F_IMPY):
        assert not st[f].any(), "impact words of a fresh episode"
    ew = st[_abi.F_ENV]
    for wd in (_abi.E_STEP, _abi.E_EGO_ACC, _abi.E_EGO_STEER, _abi.E_RETURN):
        assert not ew[:, wd].any(), f"env word {wd} of a fresh episode"
    assert not ew[:, _E_NWORDS:].any(), "env words beyond HWY_E_NWORDS"
    if episode is not None:
        np.testing.assert_array_equal(ew[:, _abi.E_EPISODE], np.broadcast_to(episode, len(envs)),
                                      err_msg="episode counters")
