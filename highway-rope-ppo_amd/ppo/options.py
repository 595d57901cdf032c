"""The run options of the training routine, one record each: what LockstepRollout's checks
(ppo/rollout.py), train_with_experiment_name (training/routine.py) and ExperimentRunner
(experiments/runner.py) know about an option -- when it counts as given, how its value is
normalised, what it needs, where it is refused and which other options it excludes -- is read from
OPTIONS and written nowhere else.  To add an option: add a record, then the code that acts on it.
"""

from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

EPISODE_SCHEDULES = ("lockstep", "reference")
TRUNCATIONS = ("terminal", "bootstrap")
# the per-episode lists episode_stats / safety_stats add to metrics_history
STATS_KEYS = ("episode_lengths", "episode_crashed", "episode_mean_speed", "episode_lane_changes")
SAFETY_KEYS = ("episode_min_ttc", "episode_min_headway", "episode_min_gap", "episode_min_distance",
               "episode_ttc_critical_share", "episode_tailgating_share")

VECTOR = "(num_envs > 1, or make_env's vector_env key for one env)"


class RunOption(NamedTuple):
    name: str
    default: object                  # the value that means "not given"
    given: Callable                  # value -> whether the option counts as given
    normalise: Callable              # value -> the form the routine and the rollout work with
    label: Optional[str] = None      # how the messages call the option when given (None: its name)
    choices: Optional[tuple] = None  # an enumeration's values, the default first
    # what follows "<label> needs a HighwayVecEnv " where the one-env loop does not take the option
    vector: Optional[str] = VECTOR
    # refused over a process group: by the routine ("routine"), by launch() before it too ("launch")
    group: Optional[str] = None
    group_first: bool = False        # the group refusal precedes the vector one
    grouped: bool = False            # launch_group / launch_batch take it (the cells share it)
    rollout: bool = False            # the vectorised loop and LockstepRollout take it
    # a view: its record (hwy.SensorModel, GridSpec, LidarSpec) says what the policy acts on
    # instead of the step's own rows, through HighwayVecEnv.view_into; a run has at most one
    view: bool = False
    on_agent: bool = False           # a PPOAgent argument: the routine reads it from the agent
    # ((other option, reason), ...): "<name> does not go with <reason>", checked with the value
    excludes: Tuple[tuple, ...] = ()
    # the same, checked by the routine alone, after what the option needs
    excludes_late: Tuple[tuple, ...] = ()
    # what a run with the option puts into metrics_history at its start: a tuple of keys (one
    # empty list each) or "value" (the value, as its dict where it has one)
    metrics: object = None


def _flag(name, **kw):
    return RunOption(name, False, bool, bool, **kw)


def _choice(name, choices, **kw):
    def check(v):
        if v not in choices:
            raise ValueError(f"{name} must be one of {choices}, got {v!r}")
        return v

    return RunOption(name, choices[0], lambda v: v != choices[0], check, choices=choices,
                     label=f"{name}={choices[1]!r}", **kw)


def _spec(name, cls_name, absent=(None,), **kw):
    """An option whose value is a hwy._abi record or its dict (imported late: hwy loads the
    native library's ABI); a value of ``absent`` means none."""
    def given(v):
        return not any(v is a for a in absent)

    def normalise(v):
        import hwy._abi as abi

        return getattr(abi, cls_name).from_dict(v) if given(v) else None

    return RunOption(name, None, given, normalise, **kw)


def check_eval_orders(eval_orders) -> list:
    """``eval_orders`` as a list of row-order names (None or empty: none), each "sorted" or
    "shuffled" and none twice; ValueError otherwise."""
    names = [] if eval_orders is None else list(eval_orders)
    if any(n not in ("sorted", "shuffled") for n in names) or len(set(names)) != len(names):
        raise ValueError(f"eval_orders must list 'sorted' and / or 'shuffled' once each, got "
                         f"{eval_orders!r}")
    return names


def _named(name, what, cls_name, value, none_ok=False) -> dict:
    import hwy._abi as abi

    if value is None:
        return {}
    if not isinstance(value, dict) or not all(isinstance(n, str) for n in value):
        raise ValueError(f"{name} must be a dict of names to {what}, got {value!r}")
    cls = getattr(abi, cls_name)
    return {n: None if none_ok and s is None else cls.from_dict(s) for n, s in value.items()}


def check_eval_sensors(eval_sensors) -> dict:
    """``eval_sensors`` as {name: hwy.SensorModel} (None or empty: none) from a dict of names to
    sensors or their dicts; ValueError otherwise."""
    return _named("eval_sensors", "sensors", "SensorModel", eval_sensors)


def check_eval_shields(eval_shields) -> dict:
    """``eval_shields`` as {name: hwy.Shield or None} (None or empty: none) from a dict of names
    to shields, their dicts or None (the unshielded evaluation); ValueError otherwise."""
    return _named("eval_shields", "shields", "Shield", eval_shields, none_ok=True)


_ONE_ENV_LOOP = VECTOR + "; the one-env reference loop "
_UNTESTED = "the combination is not tested"
_KINEMATICS = ("attribution, eval_orders, eval_sensors or eval_shields: they evaluate the policy on "
               "Kinematics rows")

OPTIONS = (
    _choice("episode_schedule", EPISODE_SCHEDULES, rollout=True, group="routine", group_first=True,
            grouped=True,
            vector="(make_env's vector_env key for one env); the one-env facade already runs the "
                   "reference loop"),
    _flag("episode_stats", rollout=True, group="routine", grouped=True, metrics=STATS_KEYS),
    _flag("safety_stats", rollout=True, group="launch", grouped=True, metrics=SAFETY_KEYS),
    _choice("truncation", TRUNCATIONS, rollout=True, group="launch", metrics="value",
            vector=_ONE_ENV_LOOP + "books a time limit as terminal"),
    _flag("attribution"),
    RunOption("eval_orders", None, bool, check_eval_orders),
    RunOption("eval_sensors", None, bool, check_eval_sensors),
    _spec("sensor", "SensorModel", view=True, rollout=True, group="launch", metrics="value", excludes=(
        ("truncation", 'truncation="bootstrap": the terminal observations (final_obs) would not '
                       "be sensed"),
        ("episode_schedule", 'episode_schedule="reference": the first observations after the cut '
                             "would not be sensed"))),
    RunOption("eval_shields", None, bool, check_eval_shields),
    _spec("shield", "Shield", rollout=True, group="launch", metrics="value", excludes=(
        ("sensor", "sensor: " + _UNTESTED),
        ("truncation", 'truncation="bootstrap": ' + _UNTESTED),
        ("episode_schedule", 'episode_schedule="reference": ' + _UNTESTED))),
    _spec("grid", "GridSpec", absent=(None, False), view=True, rollout=True, group="launch",
          metrics="value",
          excludes=(
              ("truncation", 'truncation="bootstrap": the terminal observations (final_obs) would '
                             "be Kinematics rows, not grids"),
              ("episode_schedule", 'episode_schedule="reference": the first observations after '
                                   "the cut would be Kinematics rows, not grids"),
              ("sensor", "sensor: a grid of the perceived vehicles is not built"),
              ("shield", "shield: " + _UNTESTED)),
          excludes_late=tuple((n, _KINEMATICS) for n in ("attribution", "eval_orders",
                                                         "eval_sensors", "eval_shields"))),
    # the two agent controls (PPOAgent): the KL target and the lr schedule
    RunOption("target_kl", None, lambda v: v is not None, lambda v: v, on_agent=True, grouped=True,
              vector=_ONE_ENV_LOOP + "does not take it", metrics="value"),
    RunOption("lr_anneal_updates", None, lambda v: v is not None, lambda v: v, on_agent=True,
              grouped=True, vector=_ONE_ENV_LOOP + "does not take it", metrics="value"),
    # the lidar comes last in the table and so in every order below: no older refusal moves
    _spec("lidar", "LidarSpec", absent=(None, False), view=True, rollout=True, group="launch",
          metrics="value",
          excludes=(
              ("grid", "grid: the policy acts on one of the two observations"),
              ("sensor", "sensor: the lidar has its own dropout and noise"),
              ("shield", "shield: " + _UNTESTED),
              ("truncation", 'truncation="bootstrap": the terminal observations (final_obs) would '
                             "be Kinematics rows, not lidar rows"),
              ("episode_schedule", 'episode_schedule="reference": the first observations after '
                                   "the cut would be Kinematics rows, not lidar rows")),
          excludes_late=tuple((n, _KINEMATICS) for n in ("attribution", "eval_orders",
                                                         "eval_sensors", "eval_shields"))),
)
BY_NAME = {o.name: o for o in OPTIONS}
VIEWS = tuple(o.name for o in OPTIONS if o.view)


def _order(*first) -> tuple:
    return first + tuple(o.name for o in OPTIONS if o.name not in first)


# Which refusal fires first when several apply is the order an entry point reads the options in,
# and the three entry points differ in it (an option named in none of them is read last):
ROUTINE_ORDER = _order("attribution", "eval_orders", "eval_sensors", "sensor", "eval_shields",
                       "shield", "grid", "truncation", "episode_stats", "safety_stats",
                       "target_kl", "lr_anneal_updates", "episode_schedule")
LAUNCH_ORDER = _order("episode_schedule", "episode_stats", "truncation", "safety_stats",
                      "attribution", "eval_orders", "eval_sensors", "sensor", "eval_shields",
                      "shield", "grid")
GROUPED_ORDER = _order("truncation", "attribution", "eval_orders", "eval_sensors", "sensor", "grid",
                       "eval_shields", "shield")
# what selects the launches a batch's cells share, and so must be the same in all of them
GROUPED_SHARED = tuple(o.name for o in OPTIONS if o.grouped and o.rollout)


def label(opt) -> str:
    return opt.label or opt.name


def extra_label(opt) -> str:
    """The option as the runner's messages call it: extra['truncation']='bootstrap'."""
    return f"extra[{opt.name!r}]" + label(opt)[len(opt.name):]


def extra_value(extra: dict, name: str):
    """Experiment.extra's value of option ``name`` (absent: its default) as the runner reads it:
    an enumeration's validated, a flag's as a bool, anything else as it is."""
    opt = BY_NAME[name]
    v = extra.get(name, opt.default)
    return opt.normalise(v) if opt.choices or opt.default is False else v


def extra_given(extra: dict, order):
    """The options of ``order`` (names) that Experiment.extra gives, in that order, lazily."""
    return (BY_NAME[n] for n in order if BY_NAME[n].given(extra_value(extra, n)))


def given(**kw) -> dict:
    """The keywords that were given, to be passed on with ``**``: a run option by its record's
    rule, anything else unless it is None or False.  A callee never sees a keyword at its default,
    so one that does not know the option (an older signature, a test's spy) still serves every
    call that does not use it."""
    return {k: v for k, v in kw.items()
            if (BY_NAME[k].given(v) if k in BY_NAME else v is not None and v is not False)}


def given_view(values: dict):
    """(name, spec) of the view that ``values`` (normalised, by option name; a missing one is not
    given) gives, or None.  The view options exclude each other, so where a caller has not yet
    refused a pair the first in the table's order is named."""
    return next(((n, values[n]) for n in VIEWS if BY_NAME[n].given(values.get(n))), None)


def _excluded(opt, rules, others: dict) -> None:
    """ValueError where an option that ``rules`` (of ``opt``) exclude is given in ``others``."""
    for other, reason in rules:
        o = BY_NAME[other]
        v = others.get(other, o.default)
        if o.given(v) and (o.choices is None or v in o.choices):
            raise ValueError(f"{opt.name} does not go with {reason}")


def checked(name: str, value, **others):
    """``value`` of option ``name`` normalised (None where it is not given), refusing the options
    of ``others`` (name: raw value) it excludes: what check_sensor / check_shield / check_grid
    do."""
    opt = BY_NAME[name]
    value = opt.normalise(value)
    if opt.given(value):
        _excluded(opt, opt.excludes, others)
    return value


def check_run(values: dict, is_vector, over_group: bool) -> dict:
    """train_with_experiment_name's argument checks: ``values`` (every option's raw value by
    name) normalised, after one pass over the options in ROUTINE_ORDER that refuses what an
    option excludes, a one-env loop that does not take it (``is_vector()`` False; the env is
    looked at only for an option that is given) and a process group that does not."""
    out = {}

    def norm(name):
        if name not in out:
            out[name] = BY_NAME[name].normalise(values[name])
        return out[name]

    for name in ROUTINE_ORDER:
        opt = BY_NAME[name]
        for other, _ in opt.excludes:  # an excluded option's value is validated first
            norm(other)
        if not opt.given(norm(name)):
            continue
        _excluded(opt, opt.excludes, out)
        needs = [(lambda: opt.vector is not None and not is_vector(),
                  f"{label(opt)} needs a HighwayVecEnv {opt.vector}"),
                 (lambda: opt.group is not None and over_group,
                  f"{label(opt)} does not run over a process group")]
        for refuse, message in (needs[::-1] if opt.group_first else needs):
            if refuse():
                raise ValueError(message)
        _excluded(opt, opt.excludes_late, out)
    return out


def initial_metrics(values: dict) -> dict:
    """What the given options of ``values`` (normalised, by name) put into metrics_history."""
    mh = {}
    for opt in OPTIONS:
        v = values.get(opt.name, opt.default)
        if opt.metrics is None or not opt.given(v):
            continue
        if opt.metrics == "value":
            mh[opt.name] = v.to_dict() if hasattr(v, "to_dict") else v
        else:
            mh.update({k: [] for k in opt.metrics})
    return mh
