"""Scheduled dispatch: battery dispatch whose rule changes at known times (tmh_schedule).

`dispatch` runs one rule per chain for the whole run.  Here a chain has one battery and R <= RULES_MAX rule
sets, and one uint8 array shared by all chains says which rule is in force in each metering interval of the
table: a time-of-use tariff (discharge only in the expensive hours, hold the charge otherwise), charging from
the grid in the cheap night hours, delayed charging under a feed-in limit (a high charge threshold in the
morning), a controller that picks the thresholds per quarter hour.  The parameters are the rows of an int64
array params [6 + 4 R, n] (`quantize_params`): battery.PARAMS' six, constant over the run, then for each rule
r its RULE_PARAMS in rows 6 + 4 r .. 9 + 4 r -- the thresholds Tc and Td, the feed-in limit L (NO_LIMIT = 2^27:
none) and the grid-charge power G (0: none), in 2^-FRAC_BITS W.  A "hold" rule is Tc = Td = 2^27.  Per-chain
behaviour lives in the rule parameters (a chain without a tariff gives all its rules the same values), not in
the array.  An ok second in interval k, with (Tc, Td, L, G) the chain's rule rule_of_interval[k],
d = q(pv) - q(meter) and the SoC x before it:

    a0 = dispatch's ask of d under Tc, Td
    a  = G == 0 ? a0 : min(max(a0, 0) + G, Pc)       a grid-charging rule never discharges
    s, x1, g, b, x', r = d - b, import_b, export_b = min(max(r, 0), L), curtailed, loss: dispatch's on this a

With G > 0, b may exceed max(d, 0): the difference is bought from the grid and is part of import_b.  The
engine fills an int64 tensor [n_intervals, 13, n] (BatchedSim.enable_schedule, tmh_set_schedule; fp64 engines,
one site) with dispatch's thirteen columns; in every cell [4] - [5] == [1] - [0] + [6] - [7] + [10], columns 4-7,
9 and 10 are >= 0, [6] - [7] - [9] is the interval's SoC change and the peak in [12] is <= the L of the
interval's rule.  With G = 0 everywhere and a chain's rules equal, with R = 1, or with an array that names one
rule throughout, the table and the SoC are `dispatch`'s bit for bit.  The ask depends on d, the chain's
constants and the time, never on the SoC, so the second is still a clamped addition followed by the drain's:
`second_maps` gives the triples that storage.compose / storage.apply fold.  `from_traces` is the contract as a
plain loop; `daily` builds the array of a daily local-time tariff.

The schedule sweep (BatchedSim.enable_schedule_sweep, tmh_set_schedule_sweep) runs the same second for K <=
SWEEP_MAX variants of every chain in one run -- a battery, R rule sets and a rule array each: one household under
K tariffs and batteries.  params [K, 6 + 4 R, n], arrays uint8 [K, n_intervals], tables [K, n_intervals, 13, n],
SoC [K, n]; variant v's slice is the schedule's bit for bit.  `sweep_from_traces` is the reference loop,
`quantize_sweep_params`, `check_sweep_params` and `check_sweep_rules` mirror the dispatch sweep's, `sweep_summary`
gives the run's totals per variant and chain and `energy_cost` what a tariff comparison ends in.
"""
from __future__ import annotations

import numpy as np

from . import battery, demand, dispatch, intervals
from .battery import (FRAC_BITS, HI, KEY_SHIFT, LO, MAX_INTERVAL_S, MAX_POWER, apply, compose,   # noqa: F401
                      n_intervals, quantize, quantize_soc, unpack_soc)

COLUMNS = dispatch.COLUMNS
RULE_PARAMS = ("charge_above", "discharge_above", "feed_in_limit", "grid_charge")   # a rule's rows of params
RULES_MAX = 8          # TMH_SCHEDULE_RULES_MAX
NO_LIMIT = MAX_POWER   # a rule's third row: no feed-in limit
HOLD = MAX_POWER       # Tc = Td = HOLD: the battery neither charges nor discharges
to_watts = dispatch.to_watts


def n_rules_of(params):
    """R of params [6 + 4 R, n] (ValueError when the row count is not of that form or R is outside [1, RULES_MAX])."""
    rows = int(params.shape[0])
    r, rem = divmod(rows - 6, len(RULE_PARAMS))
    if rows < 6 or rem or not 1 <= r <= RULES_MAX:
        raise ValueError(f"schedule params must have 6 + 4 R rows, 1 <= R <= {RULES_MAX}: {rows}")
    return r


def check_params(params, n_rules=None):
    """params as an int64 [6 + 4 R, n] array, every row inside its range (ValueError otherwise); n_rules, when
    given, is checked against the row count."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 2 or params.dtype != np.int64:
        raise ValueError("schedule params must be an int64 [6 + 4 R, n] array")
    r = n_rules_of(params)
    if n_rules is not None and int(n_rules) != r:
        raise ValueError(f"schedule params of {params.shape[0]} rows hold {r} rules, not {int(n_rules)}")
    names = battery.PARAMS + tuple(f"rule {k} {name}" for k in range(r) for name in RULE_PARAMS)
    ranges = battery.RANGES + ((0, MAX_POWER),) * (len(RULE_PARAMS) * r)
    for name, row, (lo, hi) in zip(names, params, ranges):
        if row.size and (int(row.min()) < lo or int(row.max()) > hi):
            raise ValueError(f"schedule {name} outside [{lo}, {hi}]: [{int(row.min())}, {int(row.max())}]")
    return params


def check_rules(rule_of_interval, n_rules, n_intervals):
    """The rule array as uint8 [n_intervals] with every entry below n_rules (ValueError otherwise)."""
    a = np.asarray(rule_of_interval.cpu() if hasattr(rule_of_interval, "cpu") else rule_of_interval)
    if a.ndim != 1 or a.dtype != np.uint8:
        raise ValueError("schedule rule_of_interval must be a uint8 [n_intervals] array")
    if a.shape[0] != int(n_intervals):
        raise ValueError(f"schedule rule_of_interval has {a.shape[0]} entries for {int(n_intervals)} intervals")
    if a.size and int(a.max()) >= int(n_rules):
        raise ValueError(f"schedule rule_of_interval names rule {int(a.max())} of {int(n_rules)}")
    return a


def quantize_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, *,
                    rules, n=None):
    """The int64 [6 + 4 R, n] parameters: battery.quantize_params' six rows, then per rule of `rules` (a list of
    dicts with the keys charge_above_w, discharge_above_w, feed_in_limit_w and grid_charge_w, each optional: 0,
    0, no limit, 0) its four rows in W (times 2^FRAC_BITS, rounded half to even).  Every value is a scalar or [n];
    feed_in_limit_w=None (or a None entry of a sequence) means no limit.  Raises ValueError on anything outside
    tmh_schedule's ranges (NaN included) and on a rule count outside [1, RULES_MAX]."""
    rules = list(rules)
    if not 1 <= len(rules) <= RULES_MAX:
        raise ValueError(f"schedule: {len(rules)} rules outside [1, {RULES_MAX}]")
    p = float(1 << FRAC_BITS)
    cols = []
    for k, rule in enumerate(rules):
        unknown = set(rule) - {name + "_w" for name in RULE_PARAMS}
        if unknown:
            raise ValueError(f"schedule rule {k}: unknown keys {sorted(unknown)}")
        lim = rule.get("feed_in_limit_w")
        if lim is None:
            lim = NO_LIMIT / p
        elif not np.isscalar(lim):
            lim = [NO_LIMIT / p if v is None else v for v in lim]
        vals = (rule.get("charge_above_w", 0.0), rule.get("discharge_above_w", 0.0), lim, rule.get("grid_charge_w", 0.0))
        arrs = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in vals]
        if any(a.ndim != 1 for a in arrs):
            raise ValueError("schedule quantities are scalars or [n] arrays")
        cols.append(arrs)
    if n is None:
        first = [np.atleast_1d(np.asarray(v)) for v in (capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w)]
        n = max(a.shape[0] for a in first + [a for arrs in cols for a in arrs])
    n = int(n)
    out = np.empty((6 + len(RULE_PARAMS) * len(rules), n), dtype=np.int64)
    out[:6] = battery.quantize_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w, n=n)
    for k, arrs in enumerate(cols):
        for j, (name, a) in enumerate(zip(RULE_PARAMS, arrs)):
            if a.shape[0] not in (1, n):
                raise ValueError(f"schedule rule {k} {name}: {a.shape[0]} values for {n} chains")
            q = np.rint(a * p)
            good = (q >= 0) & (q <= MAX_POWER)   # (NaN fails both)
            if not bool(good.all()):
                raise ValueError(f"schedule rule {k} {name} {a[~good][0]!r} outside [0, {MAX_POWER / p:.6g}]")
            out[6 + len(RULE_PARAMS) * k + j] = q.astype(np.int64)
    return out


def to_dispatch_params(params, r):
    """The dispatch kind's [9, n] params of rule r: the battery's six rows and the rule's Tc, Td and L (a copy).
    The rule's grid-charge power has no place in them: equal behaviour needs it to be 0."""
    params = check_params(params)
    r = int(r)
    if not 0 <= r < n_rules_of(params):
        raise ValueError(f"schedule: rule {r} of {n_rules_of(params)}")
    return np.concatenate([params[:6], params[6 + 4 * r:9 + 4 * r]])


def _rule_rows(params, rule):
    """(tc, td, lim, g), each [len(rule), n], of the rule index array `rule`: row 6 + 4 rule + j per entry."""
    base = 6 + len(RULE_PARAMS) * np.asarray(rule, dtype=np.int64)
    return tuple(params[base + j] for j in range(len(RULE_PARAMS)))


def _ask(d, pc, pd, tc, td, g):
    """a of the second's d under the rule (tc, td, g): dispatch's ask, and with g > 0 the grid-charge power on top
    of its charging part, within Pc."""
    a0 = np.where(d >= 0, np.minimum(np.maximum(d - tc, 0), pc), -np.minimum(np.maximum(-d - td, 0), pd))
    return np.where(g == 0, a0, np.minimum(np.maximum(a0, 0) + g, pc))


def second_maps(pv, meter, covered, interval_s, *, params, rule_of_interval, origin=0):
    """The per-second triples of traces [n_steps, n] with the parameters [6 + 4 R, n] and the rule array:
    dispatch.second_maps' with each second's ask under the rule of its interval (origin + t) // interval_s; int64
    arrays [n_steps, n] each (storage.compose, storage.apply)."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    params = check_params(params)
    n_steps, n = pv.shape
    interval_s, origin = int(interval_s), int(origin)
    rules = check_rules(rule_of_interval, n_rules_of(params), n_intervals(origin + n_steps, interval_s))
    cap, pc, pd, ec, ed, sb = params[:6]
    tc, td, _, g = _rule_rows(params, rules[(origin + np.arange(n_steps)) // interval_s])
    ok, d = battery._ok_d(pv, meter, covered)
    s = battery._stored(_ask(d, pc, pd, tc, td, g), ec, battery._recip(ed))
    a, lo, hi = compose((s, 0, np.broadcast_to(cap, s.shape)), (-sb, 0, cap))
    return np.where(ok, a, 0), np.where(ok, lo, LO).astype(np.int64), np.where(ok, hi, HI).astype(np.int64)


def from_traces(pv, meter, covered, interval_s, *, params, rule_of_interval, soc0, origin=0):
    """The schedule table of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_intervals, 13, n_chains], int64 [n_chains]).  A plain loop over the seconds, vectorised over the chains.
    params: int64 [6 + 4 R, n_chains] inside their ranges; rule_of_interval: uint8 [n_intervals], entry k the
    rule of interval k = (origin + t) // interval_s; soc0: the SoC before the first second, a scalar or
    [n_chains], clamped into [0, C]; ok seconds, interval_s and origin as intervals.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"schedule params for {params.shape[1]} chains, traces of {n}")
    rules = check_rules(rule_of_interval, n_rules_of(params), base.shape[0])
    cap, pc, pd, ec, ed, sb = params[:6]
    kc, kd = battery._recip(ec), battery._recip(ed)
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :4] = base
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, cap)
    ok, d_all = battery._ok_d(pv, meter, covered)
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        tc, td, lim, g = params[6 + 4 * int(rules[k]):10 + 4 * int(rules[k])]
        oks, d = ok[t], d_all[t]
        a = _ask(d, pc, pd, tc, td, g)
        s = battery._stored(a, ec, kd)
        x1 = np.clip(x + s, 0, cap)
        mv = x1 - x
        fill = np.minimum(a, (mv * kc + 65535) >> 16)
        drain = -np.minimum(-a, (-mv * ed) >> 16)
        b = np.where(mv == s, a, np.where(mv > 0, fill, np.where(mv < 0, drain, 0)))
        xn = np.maximum(x1 - sb, 0)
        r = d - b
        imp, sur = np.maximum(-r, 0), np.maximum(r, 0)
        exp = np.minimum(sur, lim)
        row = out[k]
        row[4] += np.where(oks, imp, 0)
        row[5] += np.where(oks, exp, 0)
        row[6] += np.where(oks, np.maximum(b, 0), 0)
        row[7] += np.where(oks, np.maximum(-b, 0), 0)
        row[8] = np.where(oks, ((o + 1) << KEY_SHIFT) | xn, row[8])                 # later seconds have larger keys
        row[9] += np.where(oks, b - (xn - x), 0)
        row[10] += np.where(oks, sur - exp, 0)
        row[11] = np.maximum(row[11], np.where(oks, demand.pack(imp, o), 0))
        row[12] = np.maximum(row[12], np.where(oks, demand.pack(exp, o), 0))
        x = np.where(oks, xn, x)
    return out, x


def daily(start, tz, n_steps, interval_s, starts, step0=0):
    """The uint8 rule array [ceil(n_steps / interval_s)] of a daily local-time tariff, for a table whose first
    step is step0 of a run from `start` in `tz`.  starts: a list of (seconds after local midnight, rule); the
    rule of the latest start at or before a time of day is in force at it (before the day's first start: the
    rule of the last one, carried over midnight).  An interval gets the rule in force at the local wall-clock
    time of its first second -- taken from clock.make_clock(...).local_at, so the daylight-saving shifts are the
    engine's: in the hour that runs twice in autumn a period edge inside it is crossed twice, and the hour that
    is skipped in spring skips its edges.  An interval that contains a period edge therefore belongs wholly to
    the earlier period: the array lives on the table's interval grid, and a tariff with edges off that grid is
    followed one interval late at most."""
    from .clock import make_clock
    n_steps, interval_s, step0 = int(n_steps), int(interval_s), int(step0)
    if n_steps <= 0 or interval_s <= 0:
        raise ValueError("schedule daily: n_steps and interval_s must be positive")
    pts = sorted((int(s), int(r)) for s, r in starts)
    if not pts:
        raise ValueError("schedule daily: no period starts")
    if any(not 0 <= s < 86400 for s, _ in pts) or any(not 0 <= r < RULES_MAX for _, r in pts):
        raise ValueError(f"schedule daily: starts are (seconds in [0, 86400), rule in [0, {RULES_MAX}))")
    if len({s for s, _ in pts}) != len(pts):
        raise ValueError("schedule daily: two periods start at the same time")
    ck = make_clock(start, n_steps, tz=tz, step0=step0)
    edges = np.array([s for s, _ in pts], dtype=np.int64)
    rule = np.array([r for _, r in pts], dtype=np.uint8)
    n_iv = n_intervals(n_steps, interval_s)
    tod = np.array([ck.local_at(step0 + k * interval_s) % 86400 for k in range(n_iv)], dtype=np.int64)
    return rule[np.searchsorted(edges, tod, side="right") - 1]   # (index -1: the last period, over midnight)


def fleet_from_traces(pv, meter, covered, interval_s, *, params, rule_of_interval, soc0, origin=0, group_chains=0):
    """The dispatch fleet series behind the schedule: dispatch.fleet_from_traces with each second under the rule of
    its interval (origin + t) // interval_s -- (int64 [n_groups, n_steps, 9], int64 [n_chains]).  params [6 + 4 R,
    n_chains], rule_of_interval, soc0, interval_s and origin as from_traces; groups as series.from_traces.  Under a
    grid-charging rule the import holds what the batteries buy and the charge may exceed the PV."""
    from . import series
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = series.from_traces(pv, meter, covered, group_chains)                  # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if not 1 <= interval_s <= MAX_INTERVAL_S:
        raise ValueError("1 <= interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"schedule params for {params.shape[1]} chains, traces of {n}")
    rules = check_rules(rule_of_interval, n_rules_of(params), n_intervals(origin + n_steps, interval_s))
    cap, pc, pd, ec, ed, sb = params[:6]
    kc, kd = battery._recip(ec), battery._recip(ed)

    def second(t, x, d):
        tc, td, lim, g = params[6 + 4 * int(rules[(origin + t) // interval_s]):][:4]
        a = _ask(d, pc, pd, tc, td, g)
        s = battery._stored(a, ec, kd)
        x1 = np.clip(x + s, 0, cap)
        mv = x1 - x
        fill = np.minimum(a, (mv * kc + 65535) >> 16)
        drain = -np.minimum(-a, (-mv * ed) >> 16)
        b = np.where(mv == s, a, np.where(mv > 0, fill, np.where(mv < 0, drain, 0)))
        return b, np.maximum(x1 - sb, 0), lim

    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, cap)
    ok, d_all = battery._ok_d(pv, meter, covered)
    return dispatch._fleet_rows(base, ok, d_all, x, second, base.shape[0], int(group_chains) or max(n, 1))


# The schedule sweep (tmh_set_schedule_sweep, BatchedSim.enable_schedule_sweep): the same second for K <= SWEEP_MAX
# variants of every chain -- a battery, R rule sets and a rule array each -- in one run; variant v's table and SoC are
# bit for bit what the schedule gives for params[v], rule_of_interval[v] and soc0[v].
SWEEP_MAX = 16   # TMH_SCHEDULE_SWEEP_MAX


def check_sweep_params(params, n_rules=None):
    """Sweep parameters as an int64 [K, 6 + 4 R, n] array, 1 <= K <= SWEEP_MAX, every variant inside tmh_schedule's
    ranges (check_params per variant; ValueError otherwise); n_rules, when given, is checked against the row count."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 3 or params.dtype != np.int64:
        raise ValueError("schedule sweep params must be an int64 [K, 6 + 4 R, n] array")
    if not 1 <= params.shape[0] <= SWEEP_MAX:
        raise ValueError(f"schedule sweep: {params.shape[0]} variants outside [1, {SWEEP_MAX}]")
    for p in params:
        check_params(p, n_rules)
    return params


def check_sweep_rules(rule_of_interval, n_rules, n_intervals, n_variants):
    """The variants' rule arrays as uint8 [K, n_intervals] with every entry below n_rules; a [n_intervals] array is
    every variant's (broadcast, a copy).  ValueError otherwise."""
    a = np.asarray(rule_of_interval.cpu() if hasattr(rule_of_interval, "cpu") else rule_of_interval)
    if a.dtype != np.uint8 or a.ndim not in (1, 2):
        raise ValueError("schedule sweep rule_of_interval must be a uint8 [n_intervals] or [K, n_intervals] array")
    if a.ndim == 1:
        a = np.broadcast_to(a, (int(n_variants), a.shape[0]))
    if a.shape != (int(n_variants), int(n_intervals)):
        raise ValueError(f"schedule sweep rule_of_interval is {tuple(a.shape)} for {int(n_variants)} variants of "
                         f"{int(n_intervals)} intervals")
    if a.size and int(a.max()) >= int(n_rules):
        raise ValueError(f"schedule sweep rule_of_interval names rule {int(a.max())} of {int(n_rules)}")
    return np.ascontiguousarray(a)


def quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, *,
                          rules, n, n_variants=None):
    """The int64 [K, 6 + 4 R, n] parameters of a schedule sweep: each battery quantity and each value of a rule of
    `rules` (quantize_params' dicts) a scalar (every variant and chain), a sequence of K values (one per variant,
    uniform over the chains) or a [K, n] array; quantised per variant by quantize_params.  feed_in_limit_w=None, or
    an entry that is None, means no limit.  Every variant has the len(rules) rules (one with fewer repeats one).  K
    is n_variants when given, else the longest argument's length; ValueError when an argument's length is neither 1
    nor K or K is outside [1, SWEEP_MAX]."""
    rules = list(rules)
    if not 1 <= len(rules) <= RULES_MAX:
        raise ValueError(f"schedule sweep: {len(rules)} rules outside [1, {RULES_MAX}]")
    none_w = NO_LIMIT / float(1 << FRAC_BITS)
    names = list(battery.PARAMS)
    vals = [capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w]
    for r, rule in enumerate(rules):
        unknown = set(rule) - {name + "_w" for name in RULE_PARAMS}
        if unknown:
            raise ValueError(f"schedule sweep rule {r}: unknown keys {sorted(unknown)}")
        lim = rule.get("feed_in_limit_w")
        if lim is None:
            lim = none_w
        elif not np.isscalar(lim):
            lim = np.asarray(lim, dtype=object)
            lim = np.where(lim == None, none_w, lim).astype(np.float64)   # noqa: E711 (elementwise)
        vals += [rule.get("charge_above_w", 0.0), rule.get("discharge_above_w", 0.0), lim, rule.get("grid_charge_w", 0.0)]
        names += [f"rule {r} {name}" for name in RULE_PARAMS]
    args = [np.asarray(v, dtype=np.float64) for v in vals]
    if any(a.ndim > 2 for a in args):
        raise ValueError("schedule sweep quantities are scalars, [K] sequences or [K, n] arrays")
    k = int(n_variants) if n_variants is not None else max([a.shape[0] for a in args if a.ndim] or [1])
    if not 1 <= k <= SWEEP_MAX:
        raise ValueError(f"schedule sweep: {k} variants outside [1, {SWEEP_MAX}]")
    for name, a in zip(names, args):
        if a.ndim and a.shape[0] not in (1, k):
            raise ValueError(f"schedule sweep {name}: {a.shape[0]} values for {k} variants")
        if a.ndim == 2 and a.shape[1] not in (1, int(n)):
            raise ValueError(f"schedule sweep {name}: {a.shape[1]} values for {n} chains")
    rows = [np.broadcast_to(a if a.ndim == 2 else a.reshape(-1, 1), (k, a.shape[1] if a.ndim == 2 else 1)) for a in args]
    keys = [name + "_w" for name in RULE_PARAMS]
    return np.stack([quantize_params(*(row[v] for row in rows[:6]),
                                     rules=[dict(zip(keys, (row[v] for row in rows[6 + 4 * r:10 + 4 * r])))
                                            for r in range(len(rules))], n=int(n)) for v in range(k)])


def quantize_sweep_soc(soc0_wh, params):
    """The starting SoC [K, n] of a sweep's batteries from watt-hours (a scalar, [K] or [K, n]); ValueError
    outside [0, C]."""
    k, _, n = params.shape
    a = np.asarray(soc0_wh, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    a = np.broadcast_to(a, (k, n))
    return np.stack([quantize_soc(a[v], params[v, :6]) for v in range(k)])


def sweep_from_traces(pv, meter, covered, interval_s, *, params, rule_of_interval, soc0, origin=0):
    """The schedule sweep of time-major traces [n_steps, n_chains]: every chain under each of K variants -- (int64
    [K, n_intervals, 13, n_chains], int64 [K, n_chains]), variant v what from_traces gives for params[v],
    rule_of_interval[v] and soc0[v].  One pass over the seconds with the state [K, n]: the second is written out here
    on [K, n] arrays, apart from from_traces and _ask, so that comparing the two compares two derivations.  params:
    int64 [K, 6 + 4 R, n_chains]; rule_of_interval: uint8 [n_intervals] (every variant's) or [K, n_intervals]; soc0:
    a scalar, [K, 1] or [K, n_chains], clamped into [0, C]."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_sweep_params(params)
    if params.shape[2] != n:
        raise ValueError(f"schedule sweep params for {params.shape[2]} chains, traces of {n}")
    K, R = params.shape[0], n_rules_of(params[0])
    arr = check_sweep_rules(rule_of_interval, R, base.shape[0], K).astype(np.int64)
    cap, pc, pd, ec, ed, sb = (params[:, r] for r in range(6))                           # [K, n] each
    kc, kd = ((1 << 32) - 1) // ec + 1, ((1 << 32) - 1) // ed + 1
    rule_rows = params[:, 6:].reshape(K, R, len(RULE_PARAMS), n)
    vs = np.arange(K)
    out = np.zeros((K, base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :, :4] = base[None]
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (K, n)), 0, cap)
    nan = np.isnan(pv) | np.isnan(meter) | (covered == 255)
    qd = np.where(nan, 0, quantize(pv) - quantize(meter)).astype(np.int64)
    k_at = -1
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        if k != k_at:                                                       # each variant's rule of the interval
            tc, td, lim, grid = (rule_rows[vs, arr[:, k], j] for j in range(len(RULE_PARAMS)))
            k_at = k
        oks, d = ~nan[t][None], qd[t][None]                                 # [1, n] against the variants' [K, n]
        charge = np.minimum(np.clip(d - tc, 0, None), pc)                   # from the surplus above Tc
        drain = np.minimum(np.clip(-d - td, 0, None), pd)                   # into the deficit above Td
        plain = np.where(d >= 0, charge, -drain)
        ask = np.where(grid > 0, np.minimum(np.clip(plain, 0, None) + grid, pc), plain)   # grid charging: never discharges
        up = ask >= 0
        mag = np.abs(ask)
        stored = np.where(up, (mag * ec) >> 16, -((mag * kd + 65535) >> 16))
        x1 = np.minimum(np.maximum(x + stored, 0), cap)
        moved = x1 - x
        cost = np.where(moved > 0, (moved * kc + 65535) >> 16, (-moved * ed) >> 16)   # at the meter side, unsigned
        clipped = np.sign(moved) * np.minimum(mag, cost)
        b = np.where(moved == stored, ask, clipped)
        xn = np.maximum(x1 - sb, 0)
        rest = d - b                                                        # left at the meter
        imp = np.where(rest < 0, -rest, 0)
        sur = np.where(rest > 0, rest, 0)
        fed = np.where(sur > lim, lim, sur)
        cell = out[:, k]
        cell[:, 4] += np.where(oks, imp, 0)
        cell[:, 5] += np.where(oks, fed, 0)
        cell[:, 6] += np.where(oks, np.maximum(b, 0), 0)
        cell[:, 7] += np.where(oks, np.maximum(-b, 0), 0)
        cell[:, 8] = np.where(oks, ((o + 1) << KEY_SHIFT) | xn, cell[:, 8])
        cell[:, 9] += np.where(oks, b - (xn - x), 0)
        cell[:, 10] += np.where(oks, sur - fed, 0)
        cell[:, 11] = np.maximum(cell[:, 11], np.where(oks, demand.pack(imp, o), 0))
        cell[:, 12] = np.maximum(cell[:, 12], np.where(oks, demand.pack(fed, o), 0))
        x = np.where(oks, xn, x)
    return out, x


def sweep_summary(raw, interval_s, params, fleet=False):
    """Per variant and chain, over all the intervals of a raw schedule sweep table [K, n_intervals, 13, n] with the
    parameters [K, 6 + 4 R, n]: dispatch.sweep_summary's keys, float64 [K, n] each (fleet=True: [K], of the integer
    totals over the chains).  The rules do not enter the summary: the battery's six rows do."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    params = check_sweep_params(params)
    if raw.ndim != 4 or raw.shape[2] != len(COLUMNS) or raw.shape[0] != params.shape[0] or raw.shape[3] != params.shape[2]:
        raise ValueError("raw schedule sweep table must be [K, n_intervals, 13, n] with params [K, 6 + 4 R, n]")
    rule0 = np.zeros((params.shape[0], 3, params.shape[2]), dtype=np.int64)   # (a valid dispatch rule: unused by the summary)
    return dispatch.sweep_summary(raw, interval_s, np.concatenate([params[:, :6], rule0], axis=1), fleet=fleet)


def energy_cost(table, import_price, feed_in_price):
    """What the energy of a raw table costs, per variant and chain: the sum over the intervals of import_price times
    the interval's import minus feed_in_price times its export, float64 [K, n] from the integer columns 4 and 5 of a
    raw table [K, n_intervals, 13, n] (or [n] of a single table [n_intervals, 13, n]).  Both prices are in currency
    per kWh; import_price is a scalar, [n_intervals] (a time-of-use tariff) or [K, n_intervals] (a tariff per
    variant), feed_in_price a scalar.  The number a tariff comparison ends in."""
    raw = np.asarray(table.cpu() if hasattr(table, "cpu") else table).astype(np.int64, copy=False)
    if raw.ndim not in (3, 4) or raw.shape[-2] != len(COLUMNS):
        raise ValueError("energy_cost: a raw table [K, n_intervals, 13, n] or [n_intervals, 13, n]")
    single = raw.ndim == 3
    if single:
        raw = raw[None]
    K, nk = raw.shape[:2]
    price = np.asarray(import_price, dtype=np.float64)
    if price.ndim > 2 or (price.ndim >= 1 and price.shape[-1] != nk) or (price.ndim == 2 and price.shape[0] != K):
        raise ValueError(f"energy_cost: import_price is a scalar, [{nk}] or [{K}, {nk}]")
    if np.ndim(feed_in_price) != 0:
        raise ValueError("energy_cost: feed_in_price is a scalar")
    price = np.broadcast_to(price, (K, nk))
    kwh = float(1 << FRAC_BITS) * 3600.0 * 1000.0                           # a column's units per kWh
    cost = (price[:, :, None] * raw[:, :, 4].astype(np.float64)).sum(axis=1) / kwh
    cost -= float(feed_in_price) * raw[:, :, 5].sum(axis=1).astype(np.float64) / kwh
    return cost[0] if single else cost
