"""Seeds, reset draws and the shuffle order of the CPU oracle against tests/rng_model.py, a numpy
restatement with its own Philox that shares no code with hwy_math.h or hwy_oracle.c.

The kernel is bit-equal to the oracle (tests/test_rng_gpu.py runs the same cases on it), so a
misreading the two share -- a counter word, a dropped high key word, a 23-bit u01, two fields
fed from one word, a step-constant or biased permutation -- shows here first, without a GPU.
The ordered comparison of every shuffled case of env_util.CASES is in tests/test_env_model.py
(the Checker there takes the permutation from rng_model).

The statistics use fixed seeds, so they are deterministic; their quantile levels are conditions
on the construction, not tuned tolerances.
"""

import numpy as np
import pytest

import rng_model as rm
import rng_util as ru
from env_util import CASES, Case, Checker
from hwy import _abi
from oracle.oracle import OracleEnv
from parity_util import make_cfg

try:
    from scipy import stats as _st

    def chi2_ppf(p, df):
        return float(_st.chi2.ppf(p, df))

    def binom_band(n, p, alpha):
        return float(_st.binom.ppf(alpha / 2, n, p)), float(_st.binom.isf(alpha / 2, n, p))

    def ks_pvalue(u):
        return float(_st.kstest(u, "uniform").pvalue)
except ImportError:  # Wilson-Hilferty, the normal band and Kolmogorov's series
    from statistics import NormalDist

    def chi2_ppf(p, df):
        z = NormalDist().inv_cdf(p)
        return df * (1 - 2 / (9 * df) + z * (2 / (9 * df)) ** 0.5) ** 3

    def binom_band(n, p, alpha):
        z = NormalDist().inv_cdf(1 - alpha / 2)
        s = (n * p * (1 - p)) ** 0.5
        return n * p - z * s - 1, n * p + z * s + 1

    def ks_pvalue(u):
        u = np.sort(u)
        n = len(u)
        d = max(np.max(np.arange(1, n + 1) / n - u), np.max(u - np.arange(n) / n))
        t = (n ** 0.5 + 0.12 + 0.11 / n ** 0.5) * d
        return float(min(1.0, 2 * sum((-1) ** (j - 1) * np.exp(-2 * j * j * t * t) for j in range(1, 101))))

ALPHA = 1e-6
M = rm.RngModel()


# ------------------------------------------------------------------------------- the generator
def test_model_philox_known_answers():
    """the three Random123 kat_vectors of philox4x32-10 that tests/test_oracle_golden.py uses"""
    kat = [([0] * 4, [0] * 2, [0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8]),
           ([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2, [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]),
           ([0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344], [0xA4093822, 0x299F31D0],
            [0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1])]
    for ctr, key, want in kat:
        assert rm.philox4x32_10(ctr, key).tolist() == want
    both = rm.philox4x32_10([k[0] for k in kat], [k[1] for k in kat])   # vectorised
    assert both.tolist() == [k[2] for k in kat]


def test_model_draws_by_hand():
    assert M.u01([0, 255, 256, 0xFFFFFFFF]).tolist() == [0.0, 0.0, 2.0 ** -24, 1.0 - 2.0 ** -24]
    assert M.choice([0, 0x3FFFFFFF, 0x40000000, 0xFFFFFFFF], 4).tolist() == [0, 0, 1, 3]
    assert M.choice([0xFFFFFFFF], 7).tolist() == [6]
    q = M.uniform([0x80000000], 21.0, 24.0)
    assert q.v.tolist() == [22.5] and q.e[0] > 0
    cfg = make_cfg(E=4, seed_base=-3)
    cfg.env_offset, cfg.seed_stride = 5, 7
    assert M.schedule_seed(cfg, 2, 3).tolist() == -3 + 5 + 2 + 1 + 21
    assert M.schedule_seed(cfg, 0, 0).tolist() == 3
    cfg.seed_base, cfg.env_offset = -10, 0
    assert int(M.schedule_seed(cfg, 0, 0)) == 2 ** 64 - 9          # wraps
    assert M.schedule_seed(cfg, [0, 1, 2, 3], 1, group_bases=[100, 200], group_envs=2).tolist() == \
        [108, 109, 208, 209]
    # ties to the lower slot; N <= 2 is the identity
    assert M.shuffle_dest(2, rm.seeds_u64([5]), 0).tolist() == [[1]]
    assert M.shuffle_dest(1, rm.seeds_u64([5]), 0).shape == (1, 0)
    d = M.shuffle_dest(15, rm.seeds_u64([5, 6]), [0, 9])
    assert sorted(d[0].tolist()) == list(range(1, 15)) and (d[0] != d[1]).any()


# ------------------------------------------------------------------------------- the reset
_WORST = {}


@pytest.mark.parametrize("name", list(ru.RESET_CASES))
def test_reset_state_matches_the_model(name):
    cfg = ru.reset_cfg(name)
    w = _WORST.setdefault(name, {})
    ru.run_reset_case(OracleEnv(cfg), cfg, worst=w)
    print(name, {k: f"{e:.3g} / {b:.3g}" for k, (e, b) in w.items() if b > 0})


def test_schedule_crosses_the_key_word_boundary():
    """seed_base 2^32 - 2: env 0's seed is below 2^32, env 1's is 2^32 (key words (0, 1))"""
    cfg = ru.reset_cfg("seed_base-crosses-2^32")
    s = M.schedule_seed(cfg, np.arange(4), 0)
    assert s.tolist() == [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 2]


@pytest.mark.parametrize("order", ["sorted", "shuffled"])
def test_explicit_seeds_with_a_mask(order):
    cfg = make_cfg(E=ru.E_RESET, order=order, initial_lane_id=-1)
    w = {}
    ru.run_explicit_reset(OracleEnv(cfg), cfg, persistent_obs=False, worst=w)
    print({k: f"{e:.3g} / {b:.3g}" for k, (e, b) in w.items() if b > 0})


# ------------------------------------------------------------------------------- the schedule
def test_schedule_through_autoreset_and_explicit_reset():
    cfg = ru.schedule_cfg(order="shuffled")
    tr = ru.run_schedule(OracleEnv(cfg), cfg, lambda e, k: M.schedule_seed(cfg, e, k))
    assert tr.fresh_seen >= 4 * (1 + 3 + 1)


def test_schedule_of_seed_groups_is_each_groups_solo_schedule():
    """The oracle has no seed groups; include/hwy.h defines a group as the solo handle of its
    envs with seed_base = seed_bases[g], so on the CPU the grouped formula of the model (global
    env index e, l = e mod 2) is compared with two solo oracle envs.  The grouped handle itself
    runs in tests/test_rng_gpu.py."""
    bases, per = [2 ** 32 - 3, 900], 2
    for g in range(2):
        cfg = ru.schedule_cfg(E=per)
        cfg.seed_base = bases[g]
        grouped = ru.schedule_cfg(E=2 * per)   # the grouped handle's config: its base is unused

        def seed_fn(e, k, g=g, grouped=grouped):
            return M.schedule_seed(grouped, g * per + np.asarray(e), k, group_bases=bases, group_envs=per)

        ru.run_schedule(OracleEnv(cfg), cfg, seed_fn)


# ------------------------------------------------------------------------------- the shuffle
@pytest.mark.parametrize("N", [3, 15, 64])
def test_shuffled_reset_observation_is_the_sorted_twins_rows_moved(N):
    ru.shuffled_reset_is_the_sorted_twins_rows_moved(OracleEnv, N)


def test_equal_keys_go_to_the_lower_slot():
    cfg = ru.tie_cfg()
    key = M.shuffle_keys(63, rm.seeds_u64([ru.TIE_SEED]), ru.TIE_STEP)[0]
    a, b = ru.TIE_SLOTS
    assert key[a] == key[b] and len(set(key.tolist())) == 62
    dest = M.shuffle_dest(64, rm.seeds_u64([ru.TIE_SEED]), ru.TIE_STEP)[0]
    assert dest[b] == dest[a] + 1
    ru.run_tie_case(OracleEnv(cfg), cfg)


def test_required_shuffled_cases_are_in_the_table():
    """N = 3 and N = 64 with all 63 admitted run the ordered comparison (tests/test_env_model.py)"""
    by = {c.name: c for c in CASES}
    assert by["N3-shuffled"].cfg == dict(N=3, order="shuffled")
    assert by["N64-V64-shuffled"].need == dict(all_admitted=1)
    shuffled = [c for c in CASES if c.cfg.get("order") == "shuffled"]
    assert len(shuffled) >= 7


def test_final_obs_rows_use_the_finished_episodes_seed_and_step():
    """An autoreset-off oracle stepped to the horizon: the observation written at the done step
    (what hwy_step_with_final gives as final_obs) is ordered by the finished episode's seed and
    its step count, not by the next episode's seed at step 0."""
    cfg = make_cfg(E=16, order="shuffled", max_episode_steps=3, autoreset=False)
    ora = OracleEnv(cfg)
    ora.reset()
    case = Case("final-obs", {})
    ck = Checker(case, cfg, None)
    for t in range(3):
        out = ora.step(np.zeros((16, 2), np.float32))
        ck.check(out, ora.state)
    assert out[3].all() and (ora.state[_abi.F_ENV][:, _abi.E_STEP] == 3).all()
    nxt = ora.state.copy()   # as the autoreset would leave the words: next seed, step 0
    nxt[_abi.F_ENV][:, _abi.E_STEP] = 0
    nxt[_abi.F_ENV][:, _abi.E_SEED_LO] += cfg.seed_stride
    with pytest.raises(AssertionError):
        Checker(case, cfg, None).check(out, nxt)


# ------------------------------------------------------------------------------- statistics
def _dest_table(N, E=512, steps=6):
    """(dest [steps, E, N - 1], seeds) of the oracle's own observations: the raw absolute x column
    names each row's vehicle (a fresh road's x strictly increases with the index), all N - 1
    others admitted, the state's step word set to t"""
    cfg = make_cfg(E=E, N=N, order="shuffled", vehicles_count=N - 1, lanes_count=16, autoreset=False,
                   observation=dict(see_behind=True, absolute=True, normalize=False, features=["x"]))
    ora = OracleEnv(cfg)
    ora.reset()
    x = ora.state[_abi.F_X].view(np.float32)[:, 1:N]
    assert (np.diff(x, axis=1) > 0).all()
    dest = np.zeros((steps, E, N - 1), np.int64)
    for t in range(steps):
        ora.state[_abi.F_ENV][:, _abi.E_STEP] = t
        obs = ora.observe()[:, 1:, 0]
        hit = obs[:, None, :] == x[:, :, None]            # [E, slot, row]
        assert (hit.sum(2) == 1).all() and (hit.sum(1) == 1).all()
        dest[t] = 1 + hit.argmax(2)
        np.testing.assert_array_equal(dest[t], M.shuffle_dest(N, rm.state_seeds(ora.state), t))
    return dest


_DEST = {}


def _dest(N):
    if N not in _DEST:
        _DEST[N] = _dest_table(N)
    return _DEST[N]


@pytest.mark.parametrize("N", [3, 15, 64])
def test_shuffle_destinations_are_uniform(N):
    """chi^2 of the (slot -> row) count table over 512 envs x 6 steps, below the 1 - 1e-6
    quantile at (N - 2)^2 degrees of freedom"""
    d = _dest(N)
    n = N - 1
    table = np.zeros((n, n))
    np.add.at(table, (np.broadcast_to(np.arange(n), d.shape), d - 1), 1)
    exp = d.shape[0] * d.shape[1] / n
    chi2 = float(((table - exp) ** 2 / exp).sum())
    bound = chi2_ppf(1 - ALPHA, (N - 2) ** 2)
    print(f"N={N}: chi2 {chi2:.1f} < {bound:.1f} at {(N - 2) ** 2} degrees of freedom")
    assert chi2 < bound


@pytest.mark.parametrize("N", [3, 15, 64])
def test_shuffle_depends_on_step_and_seed(N):
    """slots whose row is unchanged from step t to t + 1, and from seed s to s + 1 (neighbouring
    envs of the schedule) at the same step: within the two-sided 1e-6 band of
    Binomial(n, 1 / (N - 1)).  A step- or seed-constant permutation gives n.  (The slots of one
    env are not independent -- the fixed points of a uniform permutation have variance 1 per env
    against the binomial's 1 - 1 / (N - 1), twice it at N = 3 -- so the band is the stricter
    reading; the counts sit well inside it.)"""
    d = _dest(N)
    for what, same in (("step", d[1:] == d[:-1]), ("seed", d[:, 1:] == d[:, :-1])):
        n, k = same.size, int(same.sum())
        lo, hi = binom_band(n, 1.0 / (N - 1), ALPHA)
        print(f"N={N} next {what}: {k} of {n} unchanged, band [{lo:.0f}, {hi:.0f}]")
        assert lo <= k <= hi


_DRAWS = {}


def _reset_draws(lanes):
    """the draws of 4,096 seeds' others, recovered from the oracle's reset state: lane, and the
    speed, jitter and exponent mapped back to [0, 1)"""
    if lanes not in _DRAWS:
        cfg = make_cfg(E=4096, lanes_count=lanes, seed_base=7)
        ora = OracleEnv(cfg)
        ora.reset()
        V = cfg.vehicles_count + 1
        f = {k: ora.state[i].view(np.float32)[:, :V].astype(np.float64)
             for k, i in (("x", _abi.F_X), ("speed", _abi.F_SPEED), ("delta", _abi.F_DELTA))}
        lane = ora.state[_abi.F_LANE][:, 1:V].astype(np.int64)
        lim = float(cfg.speed_limit)
        u_speed = (f["speed"][:, 1:] - 0.7 * lim) / (0.1 * lim)
        offset = (12.0 + f["speed"][:, 1:]) / float(cfg.vehicles_density) * np.exp(-0.125 * lanes)
        u_jit = (np.diff(f["x"], axis=1) / offset - 0.9) / 0.2
        u_delta = f["delta"][:, 1:] - 3.5
        _DRAWS[lanes] = (lane, u_speed, u_jit, u_delta)
    return _DRAWS[lanes]


@pytest.mark.parametrize("lanes", [4, 7])
def test_reset_lane_draws_are_uniform(lanes):
    lane = _reset_draws(lanes)[0]
    counts = np.bincount(lane.ravel(), minlength=lanes)
    assert len(counts) == lanes
    exp = lane.size / lanes
    chi2 = float(((counts - exp) ** 2 / exp).sum())
    bound = chi2_ppf(1 - ALPHA, lanes - 1)
    print(f"{lanes} lanes: chi2 {chi2:.2f} < {bound:.2f} over {lane.size} draws")
    assert chi2 < bound


def test_reset_float_draws_are_uniform_and_uncorrelated():
    """Kolmogorov-Smirnov of the speed, jitter and exponent draws against U(0, 1) (p >= 1e-6);
    the four words' pairwise correlations within 5 / sqrt(n)"""
    lane, u_speed, u_jit, u_delta = _reset_draws(4)
    for name, u in (("speed", u_speed), ("jitter", u_jit), ("delta", u_delta)):
        u = u.ravel()
        assert u.min() > -1e-5 and u.max() < 1 + 1e-5, (name, u.min(), u.max())
        p = ks_pvalue(np.clip(u, 0.0, 1.0))
        print(f"{name}: KS p = {p:.3g} over {u.size} draws")
        assert p >= ALPHA
    cols = np.stack([lane.ravel().astype(np.float64), u_speed.ravel(), u_jit.ravel(), u_delta.ravel()])
    r = np.corrcoef(cols)
    off = np.abs(r[~np.eye(4, dtype=bool)]).max()
    print(f"largest pairwise correlation {off:.2e}, allowed {5 / cols.shape[1] ** 0.5:.2e}")
    assert off <= 5 / cols.shape[1] ** 0.5


def test_u01_is_below_one():
    """so uniform's real value never reaches hi (24 bits: at most 1 - 2^-24)"""
    cfg = make_cfg(E=4096, seed_base=7)
    w = M.reset_words(M.schedule_seed(cfg, np.arange(4096), 0), 51)
    u = M.u01(w)
    assert u.max() < 1.0 and u.min() >= 0.0
    assert M.u01([0xFFFFFFFF])[0] == 1.0 - 2.0 ** -24
    assert (np.unique(u * 2.0 ** 24 % 2).tolist()) == [0.0, 1.0]   # the 24th bit is used


# ------------------------------------------------------------------------------- mutations
def _all_cases(model):
    """a short pass over every kind of case, on the oracle, with `model` as the reference"""
    cfg = ru.reset_cfg("seed_base-2^33+5")
    ru.run_reset_case(OracleEnv(cfg), cfg, model=model)
    cfg = ru.reset_cfg("default", order="shuffled")
    ru.run_reset_case(OracleEnv(cfg), cfg, model=model)
    cfg = ru.schedule_cfg()
    ru.run_schedule(OracleEnv(cfg), cfg, lambda e, k: model.schedule_seed(cfg, e, k), model=model)
    solo, grouped = ru.schedule_cfg(E=2), ru.schedule_cfg(E=4)
    solo.seed_base = 900
    ru.run_schedule(OracleEnv(solo), solo, model=model, seed_fn=lambda e, k: model.schedule_seed(
        grouped, 2 + np.asarray(e), k, group_bases=[2 ** 32 - 3, 900], group_envs=2))
    cfg = ru.tie_cfg()
    ru.run_tie_case(OracleEnv(cfg), cfg, model=model)


def test_every_case_passes_with_the_model_as_it_is():
    _all_cases(rm.RngModel())


@pytest.mark.parametrize("mut", rm.MUTATIONS)
def test_mutation_of_the_model_fails_a_case(mut):
    """each deliberate mistake in the model is refused by at least one case"""
    with pytest.raises(AssertionError):
        _all_cases(rm.RngModel(mut))
