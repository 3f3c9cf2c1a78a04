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
