"""A numpy restatement of hwy_observe's row -> vehicle map and of its scatter.

Independent of csrc/hwy_kernels.hip and of oracle/hwy_oracle.c.  It composes what the other
models already state: `env_model.observed_vehicles` (who is admitted, the `sorted` key as one
float32 subtraction of the stored positions with ties to the lower index, the cap at N - 1) and
`rng_model.shuffle_dest` on `rng_model.state_seeds` and the state's step word (the `shuffled`
permutation).  Slot q before the shuffle goes to row `dest[q]`; row 0 is the ego (vehicle 0); a
row no slot fills is -1.

`identify` is the check against an observation that shares nothing with this model: under
`identity_cfg` (absolute, un-normalised, no wrapper) a row's x and y ARE the stored words of the
vehicle it shows, so an observer's rows name their vehicles themselves.

`row_vehicles(mut=...)` is the model with one deliberate mistake (MUTATIONS), for the test that
shows each of them is refused by at least one case.
"""

from __future__ import annotations

import numpy as np

import env_model as em
import rng_model as rm
from hwy import _abi

MUTATIONS = (
    "permutation-inverted",       # row 1 + q shows slot dest[q] - 1 (the inverse permutation)
    "empty-slots-compacted",      # the filled rows moved ahead of the empty ones
    "ties-to-higher-index",       # equal |dx|: the higher vehicle index first
    "cap-at-N",                   # N slots admitted and shuffled, the row past the last dropped
    "shuffle-step-fixed-at-0",    # the permutation of step 0 at every step
)

ORDERS = {None: None, "sorted": _abi.ORDER_SORTED, "shuffled": _abi.ORDER_SHUFFLED}


def with_order(cfg, order):
    """a copy of cfg observed under `order` (None: its own)"""
    c = _abi.HwyConfig.from_buffer_copy(cfg)
    if ORDERS[order] is not None:
        c.order = ORDERS[order]
    return c


def _mirrored(cfg, state):
    """the state with traffic vehicles 1..V-1 in reverse index order, and the map back"""
    V = int(cfg.vehicles_count) + 1
    st = state.copy()
    st[:_abi.F_ENV, :, 1:V] = state[:_abi.F_ENV, :, 1:V][:, :, ::-1]
    return st, (lambda idx: np.where(idx > 0, V - idx, idx))


def row_vehicles(cfg, state, order=None, mut=""):
    """[E, N] int64: the vehicle index row r of the observation shows, -1 for an empty row."""
    assert mut == "" or mut in MUTATIONS, mut
    c = with_order(cfg, order)
    state = np.asarray(state).view(np.uint32)
    E, N = state.shape[1], int(c.obs_vehicles)
    n = N - 1
    slots_cfg = c
    if mut == "cap-at-N":
        slots_cfg = _abi.HwyConfig.from_buffer_copy(c)
        slots_cfg.obs_vehicles = N + 1
        n = N
    if mut == "ties-to-higher-index" and c.order == _abi.ORDER_SORTED:
        st, back = _mirrored(c, state)
        slots = back(em.observed_vehicles(slots_cfg, st))
    else:
        slots = em.observed_vehicles(slots_cfg, state)        # [E, n]
    if c.order == _abi.ORDER_SHUFFLED:
        model = rm.RngModel("shuffle-step-fixed-at-0" if mut == "shuffle-step-fixed-at-0" else "")
        dest = model.shuffle_dest(n + 1, rm.state_seeds(state), state[_abi.F_ENV][:, _abi.E_STEP])
    else:
        dest = np.broadcast_to(1 + np.arange(n), (E, n))
    out = np.full((E, max(N, n + 1)), -1, np.int64)
    out[:, 0] = 0
    ar = np.arange(E)
    for q in range(n):
        if mut == "permutation-inverted":
            out[:, 1 + q] = slots[ar, dest[:, q] - 1]
        else:
            out[ar, dest[:, q]] = slots[:, q]
    out = out[:, :N]
    if mut == "empty-slots-compacted":
        for e in range(E):
            rest = out[e, 1:]
            filled = rest[rest >= 0]
            out[e, 1:] = -1
            out[e, 1:1 + len(filled)] = filled
    return out


def scatter(row_vehicle, row_values):
    """hwy_observe's veh_values as uint32 words [E, 64]: the bits of row_values[e][r] at vehicle
    row_vehicle[e][r] for every row with a vehicle, +0.0 everywhere else."""
    rv = np.asarray(row_vehicle)
    bits = np.ascontiguousarray(row_values, np.float32).view(np.uint32).reshape(rv.shape)
    out = np.zeros((rv.shape[0], _abi.HWY_MAX_VEHICLES), np.uint32)
    e, r = np.nonzero(rv >= 0)
    out[e, rv[e, r]] = bits[e, r]
    return out


# ------------------------------------------------------------------------------- identification
def identity_cfg(cfg, order=None):
    """cfg under `order`, observing absolute, un-normalised x and y with no wrapper: what a row
    then holds in its first two columns are the stored x and y words of its vehicle"""
    c = with_order(cfg, order)
    c.absolute, c.normalize, c.pe_kind, c.d_embed = 1, 0, _abi.PE_NONE, 0
    fid = [int(c.feature_ids[f]) for f in range(c.n_features)]
    assert _abi.FEATURES["x"] in fid and _abi.FEATURES["y"] in fid, "identification needs x and y"
    return c


def identify(cfg, state, rows, obs_abs, keep=None):
    """The mismatches of a row -> vehicle map `rows` [E, N] against `obs_abs` [E, N, F], an
    observation of `state` under identity_cfg: a row with a vehicle must hold that vehicle's stored
    x and y words bit for bit (a NaN position is never admitted, so none is compared), a -1 row
    must be all zeros.  Returns (rows compared, empty rows, list of (env, row, why))."""
    state = np.asarray(state).view(np.uint32)
    rows = np.asarray(rows)
    fid = [int(cfg.feature_ids[f]) for f in range(cfg.n_features)]
    cx, cy = fid.index(_abi.FEATURES["x"]), fid.index(_abi.FEATURES["y"])
    words = np.ascontiguousarray(obs_abs, np.float32).view(np.uint32)
    E, N = rows.shape
    bad, empty, seen = [], 0, 0
    for e in range(E):
        if keep is not None and not keep[e]:
            continue
        for r in range(N):
            seen += 1
            v = int(rows[e, r])
            if v < 0:
                empty += 1
                if words[e, r].any():
                    bad.append((e, r, "a -1 row that is not all zero"))
            elif (words[e, r, cx] != state[_abi.F_X][e, v]
                  or words[e, r, cy] != state[_abi.F_Y][e, v]):
                bad.append((e, r, f"x, y are not vehicle {v}'s stored words"))
    return seen, empty, bad
