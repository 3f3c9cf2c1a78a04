"""Battery dispatch: the battery kind under thresholds and a feed-in limit (tmh_dispatch).

`battery` runs one control rule, greedy self-consumption: the battery takes every surplus watt and gives
into every deficit watt.  Here each chain's battery charges only from the surplus above a threshold Tc,
discharges only into the deficit above a threshold Td, and what is left of the surplus is fed in up to a
limit L, the rest curtailed -- a household under a 70 % or 60 % feed-in limit, a battery that charges only
from what would be curtailed, a battery that caps the import peak.  The parameters are the nine rows of an
int64 array params [9, n] (`quantize_params`): battery.PARAMS' six, then Tc, Td and L in 2^-FRAC_BITS W;
L = NO_LIMIT = 2^27 means no limit, since a second's surplus stays below 2^26.  An ok second with
d = q(pv) - q(meter) and the SoC x before it:

    a  = d >= 0 ?  min(max(d - Tc, 0), Pc)  :  -min(max(-d - Td, 0), Pd)      asked at the meter side
    s, x1, g, b, x'   exactly battery's rule applied to this a
    r  = d - b                       what is left at the meter (b lies between 0 and d)
    import_b  = max(-r, 0)           surplus = max(r, 0)
    export_b  = min(surplus, L)      fed in
    curtailed = surplus - export_b   what the inverter throws away
    loss      = b - (x' - x)

A second that is not ok leaves x unchanged and adds nothing.  The engine fills an int64 tensor
[n_intervals, 13, n] (BatchedSim.enable_dispatch, tmh_set_dispatch; fp64 engines only):

    [k, 0:4, i]  the interval table's columns (pv, meter, n_ok, covered); [0] stays the available PV,
                 what was produced is [0] - [10]
    [k, 4, i]    sum of import_b          [k, 5, i] sum of export_b (after the limit)
    [k, 6, i]    sum of max(b, 0)         [k, 7, i] sum of max(-b, 0)
    [k, 8, i]    storage's SoC key        [k, 9, i] sum of loss
    [k, 10, i]   sum of curtailed
    [k, 11, i]   peak import behind the battery: the maximum of demand's key(import_b, o)
    [k, 12, i]   peak feed-in: the maximum of key(export_b, o)

In every cell [4] - [5] == [1] - [0] + [6] - [7] + [10], columns 4-7, 9 and 10 are >= 0, [6] - [7] - [9] is
the interval's SoC change and the peak in [12] is <= L.  With Tc = Td = 0 and L = NO_LIMIT columns 0-9 and the
SoC are `battery`'s bit for bit and column 10 is 0; with C = 0 and L = NO_LIMIT columns 11 and 12 are `demand`'s
6 and 7; with C = 0 and any L, [5] + [10] is the registers' export.  The ask depends on d and the chain's
constants only, so the second is still a clamped addition followed by the drain's: `second_maps` gives the
triples that storage.compose / storage.apply fold.  `from_traces` is the contract as a plain loop.

The dispatch sweep (BatchedSim.enable_dispatch_sweep, tmh_set_dispatch_sweep) runs the same rule for K <= SWEEP_MAX
parameter sets per chain in one run -- one household under K rules and batteries: params [K, 9, n]
(`quantize_sweep_params`), the state of charge [K, n], the tables [K, n_intervals, 13, n], variant v's slice of each
what the single kind is given and gives.  `sweep_from_traces` is that contract as one loop with the state [K, n],
`sweep_summary` the run's totals, shares and peaks per variant and chain.
"""
from __future__ import annotations

import numpy as np

from . import battery, demand, intervals
from .battery import (FRAC_BITS, HI, KEY_SHIFT, LO, MAX_INTERVAL_S, MAX_POWER, MAX_W, apply, compose,   # noqa: F401
                      n_intervals, quantize, quantize_soc, unpack_soc)

COLUMNS = battery.COLUMNS + ("curtailed", "peak_import", "peak_export")
PARAMS = battery.PARAMS + ("charge_above", "discharge_above", "feed_in_limit")   # the rows of params
NO_LIMIT = MAX_POWER   # row 8: no feed-in limit
# each row's inclusive range (tmh_dispatch)
RANGES = battery.RANGES + ((0, MAX_POWER),) * 3


def check_params(params):
    """params as an int64 [9, n] array, every row inside its range (ValueError otherwise)."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 2 or params.shape[0] != len(PARAMS) or params.dtype != np.int64:
        raise ValueError("dispatch params must be an int64 [9, n] array")
    for name, row, (lo, hi) in zip(PARAMS, params, RANGES):
        if row.size and (int(row.min()) < lo or int(row.max()) > hi):
            raise ValueError(f"dispatch {name} outside [{lo}, {hi}]: [{int(row.min())}, {int(row.max())}]")
    return params


def quantize_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0,
                    charge_above_w=0.0, discharge_above_w=0.0, feed_in_limit_w=None, n=None):
    """The int64 [9, n] parameters: battery.quantize_params' six rows, then the two thresholds and the feed-in
    limit in W (times 2^FRAC_BITS, rounded half to even), each a scalar or [n].  feed_in_limit_w=None (or
    an entry that is None in a sequence) means no limit.  Raises ValueError on anything outside tmh_dispatch's
    ranges (NaN included)."""
    p = float(1 << FRAC_BITS)
    if feed_in_limit_w is None:
        feed_in_limit_w = NO_LIMIT / p
    elif not np.isscalar(feed_in_limit_w):
        feed_in_limit_w = [NO_LIMIT / p if v is None else v for v in feed_in_limit_w]
    extra = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in (charge_above_w, discharge_above_w, feed_in_limit_w)]
    if any(a.ndim != 1 for a in extra):
        raise ValueError("dispatch quantities are scalars or [n] arrays")
    if n is None:
        first = [np.atleast_1d(np.asarray(v)) for v in (capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w)]
        n = max(a.shape[0] for a in first + extra)
    out = np.empty((len(PARAMS), int(n)), dtype=np.int64)
    out[:6] = battery.quantize_params(capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w, n=n)
    for r, (name, a, (lo, hi)) in enumerate(zip(PARAMS[6:], extra, RANGES[6:]), start=6):
        if a.shape[0] not in (1, n):
            raise ValueError(f"dispatch {name}: {a.shape[0]} values for {n} chains")
        q = np.rint(a * p)
        if not bool(((q >= lo) & (q <= hi)).all()):   # (NaN fails both)
            raise ValueError(f"dispatch {name} {a[~((q >= lo) & (q <= hi))][0]!r} outside [{lo / p:.6g}, {hi / p:.6g}]")
        out[r] = q.astype(np.int64)
    return out


def _ask(d, params):
    """a of the second's d: the surplus above Tc up to Pc, or the deficit above Td up to Pd (negative)."""
    pc, pd, tc, td = params[1], params[2], params[6], params[7]
    return np.where(d >= 0, np.minimum(np.maximum(d - tc, 0), pc), -np.minimum(np.maximum(-d - td, 0), pd))


def second_maps(pv, meter, covered, *, params):
    """The per-second triples of traces [n_steps, n] with the parameters [9, n]: battery.second_maps' with
    the thresholded ask; int64 arrays [n_steps, n] each (storage.compose, storage.apply)."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    params = check_params(params)
    cap, ec, ed, sb = params[0], params[3], params[4], params[5]
    ok, d = battery._ok_d(pv, meter, covered)
    s = battery._stored(_ask(d, params), ec, battery._recip(ed))
    a, lo, hi = compose((s, 0, np.broadcast_to(cap, s.shape)), (-sb, 0, cap))
    return np.where(ok, a, 0), np.where(ok, lo, LO).astype(np.int64), np.where(ok, hi, HI).astype(np.int64)


def _second(x, d, params):
    """One second of every chain: (b, x') of the SoC x before it and d, as if the second were ok."""
    cap, pc, pd, ec, ed, sb = params[:6]
    a = _ask(d, params)
    s = battery._stored(a, ec, battery._recip(ed))
    x1 = np.clip(x + s, 0, cap)
    g = x1 - x
    fill = np.minimum(a, (g * battery._recip(ec) + 65535) >> 16)
    drain = -np.minimum(-a, (-g * ed) >> 16)
    b = np.where(g == s, a, np.where(g > 0, fill, np.where(g < 0, drain, 0)))
    return b, np.maximum(x1 - sb, 0)


def from_traces(pv, meter, covered, interval_s, *, params, soc0, origin=0):
    """The dispatch table of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_intervals, 13, n_chains], int64 [n_chains]).  A plain loop over the seconds, vectorised over the
    chains.  params: int64 [9, n_chains] inside their ranges; soc0: the SoC before the first second, a
    scalar or [n_chains], clamped into [0, C]; ok seconds, interval_s and origin as intervals.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"dispatch params for {params.shape[1]} chains, traces of {n}")
    lim = params[8]
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :4] = base
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, params[0])
    ok, d_all = battery._ok_d(pv, meter, covered)
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        oks, d = ok[t], d_all[t]
        b, xn = _second(x, d, params)
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


def to_battery(raw):
    """The battery table [n_intervals, 10, n] inside a dispatch table (its first ten columns; a view)."""
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw dispatch table must be [n_intervals, 13, n]")
    return raw[:, :10]


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 13, n]: battery.to_watts' keys plus energy_wh_curtailed (Wh
    the inverter threw away above the feed-in limit), curtailed_share = curtailed / available PV (NaN without
    PV), peak_w_import and peak_w_export (W, behind the battery and after the limit) and t_peak_import and
    t_peak_export (seconds into the interval of the earliest second at the peak; NaN without an ok second).
    energy_wh_pv stays the available PV; self_consumption counts what was used on site or stored, so the
    curtailed energy is taken out of it as the export is: (pv - export - curtailed) / pv, battery's ratio
    where nothing is curtailed.  n_steps, when given, is checked against the interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    out = battery.to_watts(to_battery(raw), interval_s, n_steps=n_steps)
    e, scale = float(1 << FRAC_BITS) * 3600.0, float(1 << FRAC_BITS)
    qpv = np.where(raw[:, 0] != 0, raw[:, 0], np.nan).astype(np.float64)
    out.update({"energy_wh_curtailed": raw[:, 10] / e, "curtailed_share": raw[:, 10] / qpv,
                "self_consumption": (raw[:, 0] - raw[:, 5] - raw[:, 10]) / qpv})
    for name, col in (("import", 11), ("export", 12)):
        v, o = demand.unpack(raw[:, col])
        out["peak_w_" + name] = v / scale
        out["t_peak_" + name] = np.where(o >= 0, o, np.nan).astype(np.float64)
    return out


SWEEP_MAX = 16   # TMH_DISPATCH_SWEEP_MAX: the variants of one dispatch sweep


def check_sweep_params(params):
    """Sweep parameters as an int64 [K, 9, n] array, 1 <= K <= SWEEP_MAX, every variant inside tmh_dispatch's
    ranges (check_params per variant; ValueError otherwise)."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 3 or params.shape[1] != len(PARAMS) or params.dtype != np.int64:
        raise ValueError("dispatch sweep params must be an int64 [K, 9, n] array")
    if not 1 <= params.shape[0] <= SWEEP_MAX:
        raise ValueError(f"dispatch sweep: {params.shape[0]} variants outside [1, {SWEEP_MAX}]")
    for p in params:
        check_params(p)
    return params


def quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0,
                          charge_above_w=0.0, discharge_above_w=0.0, feed_in_limit_w=None, *, n, n_variants=None):
    """The int64 [K, 9, n] parameters of a dispatch sweep: each quantity a scalar (every variant and chain), a
    sequence of K values (one per variant, uniform over the chains) or a [K, n] array; quantised per variant by
    quantize_params.  feed_in_limit_w=None, or an entry that is None, means no limit.  K is n_variants when
    given, else the longest argument's length; ValueError when an argument's length is neither 1 nor K or K is
    outside [1, SWEEP_MAX]."""
    none_w = NO_LIMIT / float(1 << FRAC_BITS)
    if feed_in_limit_w is None:
        feed_in_limit_w = none_w
    elif not np.isscalar(feed_in_limit_w):
        lim = np.asarray(feed_in_limit_w, dtype=object)
        feed_in_limit_w = np.where(lim == None, none_w, lim).astype(np.float64)   # noqa: E711 (elementwise)
    args = [np.asarray(v, dtype=np.float64) for v in (capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff,
                                                      standby_w, charge_above_w, discharge_above_w, feed_in_limit_w)]
    if any(a.ndim > 2 for a in args):
        raise ValueError("dispatch sweep quantities are scalars, [K] sequences or [K, n] arrays")
    k = int(n_variants) if n_variants is not None else max([a.shape[0] for a in args if a.ndim] or [1])
    if not 1 <= k <= SWEEP_MAX:
        raise ValueError(f"dispatch sweep: {k} variants outside [1, {SWEEP_MAX}]")
    for name, a in zip(PARAMS, args):
        if a.ndim and a.shape[0] not in (1, k):
            raise ValueError(f"dispatch sweep {name}: {a.shape[0]} values for {k} variants")
        if a.ndim == 2 and a.shape[1] not in (1, int(n)):
            raise ValueError(f"dispatch sweep {name}: {a.shape[1]} values for {n} chains")
    rows = [np.broadcast_to(a if a.ndim == 2 else a.reshape(-1, 1), (k, a.shape[1] if a.ndim == 2 else 1)) for a in args]
    return np.stack([quantize_params(*(r[v] for r in rows), n=int(n)) for v in range(k)])


def quantize_sweep_soc(soc0_wh, params):
    """The starting SoC [K, n] of a sweep's batteries from watt-hours (a scalar, [K] or [K, n]); ValueError
    outside [0, C]."""
    k, _, n = params.shape
    a = np.asarray(soc0_wh, dtype=np.float64)
    if a.ndim == 1:
        a = a.reshape(-1, 1)
    a = np.broadcast_to(a, (k, n))
    return np.stack([quantize_soc(a[v], params[v]) for v in range(k)])


def sweep_from_traces(pv, meter, covered, interval_s, *, params, soc0, origin=0):
    """The dispatch sweep of time-major traces [n_steps, n_chains]: every chain under each of K rule sets --
    (int64 [K, n_intervals, 13, n_chains], int64 [K, n_chains]), variant v what from_traces gives for params[v]
    and soc0[v].  One loop over the seconds with the state [K, n]: the second's rule is written out here on
    [K, n] arrays, apart from from_traces, _ask and _second, so that comparing the two compares two derivations.
    params: int64 [K, 9, n_chains]; soc0: a scalar, [K, 1] or [K, n_chains], clamped into [0, C]."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_sweep_params(params)
    if params.shape[2] != n:
        raise ValueError(f"dispatch sweep params for {params.shape[2]} chains, traces of {n}")
    K = params.shape[0]
    cap, pc, pd, ec, ed, sb, tc, td, lim = (params[:, r] for r in range(9))              # [K, n] each
    kc, kd = ((1 << 32) - 1) // ec + 1, ((1 << 32) - 1) // ed + 1
    out = np.zeros((K, base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :, :4] = base[None]
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (K, n)), 0, cap)
    nan = np.isnan(pv) | np.isnan(meter) | (covered == 255)
    qd = np.where(nan, 0, quantize(pv) - quantize(meter)).astype(np.int64)
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        oks, d = ~nan[t][None], qd[t][None]                                 # [1, n] against the variants' [K, n]
        charge = np.minimum(np.clip(d - tc, 0, None), pc)                   # from the surplus above Tc
        drain = np.minimum(np.clip(-d - td, 0, None), pd)                   # into the deficit above Td
        ask = np.where(d >= 0, charge, -drain)
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
    """Per variant and chain, over all the intervals of a raw dispatch sweep table [K, n_intervals, 13, n] with
    the parameters [K, 9, n]: battery.sweep_summary's keys (self_consumption with the curtailed energy taken out,
    as to_watts: (pv - export - curtailed) / pv) plus energy_wh_curtailed, curtailed_share = curtailed /
    available PV (NaN without PV) and peak_w_import and peak_w_export, the run's largest import and feed-in
    behind the battery in W -- float64 [K, n] each.  fleet=True: [K], of the integer totals over the chains; the
    peaks are then the largest of any chain (the chains' peaks need not coincide: not the fleet's peak)."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    params = check_sweep_params(params)
    if raw.ndim != 4 or raw.shape[2] != len(COLUMNS) or raw.shape[0] != params.shape[0] or raw.shape[3] != params.shape[2]:
        raise ValueError("raw dispatch sweep table must be [K, n_intervals, 13, n] with params [K, 9, n]")
    out = battery.sweep_summary(raw[:, :, :10], interval_s, params[:, :6], fleet=fleet)
    tot = raw.sum(axis=1)                                                   # [K, 13, n] (columns 8, 11, 12 are keys: unused)
    pk_im = demand.unpack(raw[:, :, 11])[0].max(axis=1) if raw.shape[1] else np.zeros(tot[:, 0].shape, dtype=np.int64)
    pk_ex = demand.unpack(raw[:, :, 12])[0].max(axis=1) if raw.shape[1] else np.zeros(tot[:, 0].shape, dtype=np.int64)
    if fleet:
        tot = tot.sum(axis=2)
        pk_im, pk_ex = (p.max(axis=1) if p.shape[1] else np.zeros(p.shape[0], dtype=np.int64) for p in (pk_im, pk_ex))
    e, scale = float(1 << FRAC_BITS) * 3600.0, float(1 << FRAC_BITS)
    pv, exp, cur = tot[:, 0], tot[:, 5], tot[:, 10]
    qpv = np.where(pv != 0, pv, np.nan).astype(np.float64)
    out.update({"energy_wh_curtailed": cur / e, "curtailed_share": cur / qpv, "self_consumption": (pv - exp - cur) / qpv,
                "peak_w_import": pk_im / scale, "peak_w_export": pk_ex / scale})
    return out


# The dispatch fleet series (tmh_set_dispatch_fleet, BatchedSim.enable_dispatch_fleet): battery.FLEET_COLUMNS behind
# this kind's rule -- the export after the limit -- and the curtailed power beside them.
FLEET_COLUMNS = battery.FLEET_COLUMNS + ("curtailed",)


def _fleet_rows(base, ok, d_all, x, second, n_groups, gc):
    """The loop the two kinds' fleet_from_traces share: second(t, x, d) -> (b, x', lim) of second t; base is
    series.from_traces' [n_groups, n_steps, 4].  Returns ([n_groups, n_steps, 9], the SoC after the seconds)."""
    n_steps = ok.shape[0]
    out = np.zeros((n_groups, n_steps, len(FLEET_COLUMNS)), dtype=np.int64)
    out[..., :4] = base
    for t in range(n_steps):
        oks, d = ok[t], d_all[t]
        b, xn, lim = second(t, x, d)
        x = np.where(oks, xn, x)
        r = d - b
        sur = np.maximum(r, 0)
        exp = np.minimum(sur, lim)
        cols = np.where(oks, np.stack([np.maximum(-r, 0), exp, x, np.maximum(b, 0), sur - exp]), 0)
        for g in range(n_groups):
            out[g, t, 4:] = cols[:, g * gc:(g + 1) * gc].sum(axis=1)
    return out, x


def fleet_from_traces(pv, meter, covered, *, params, soc0, group_chains=0):
    """The dispatch fleet series of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_groups, n_steps, 9], int64 [n_chains]).  from_traces' loop over the seconds (on _second), summed over the
    chains of a group instead of the seconds of an interval: row t of a group holds, over its chains that are ok at
    second t, FLEET_COLUMNS -- series.from_traces' four columns, the sums of import_b, of export_b after the limit,
    of the SoC x' after the second, of max(b, 0) and of the curtailed power.  params [9, n_chains], soc0: as
    from_traces; groups as series.from_traces (chain i in group i // group_chains, 0: one group, else a multiple of
    512; the last may be partial)."""
    from . import series
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = series.from_traces(pv, meter, covered, group_chains)                   # (checks the arguments)
    n = pv.shape[1]
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"dispatch params for {params.shape[1]} chains, traces of {n}")
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, params[0])
    ok, d_all = battery._ok_d(pv, meter, covered)
    return _fleet_rows(base, ok, d_all, x, lambda t, x, d: _second(x, d, params) + (params[8],), base.shape[0],
                       int(group_chains) or max(n, 1))


def fleet_to_watts(raw, bin_s=1, mean=False):
    """float64 series of a raw dispatch fleet table [..., n_steps, 9]: battery.fleet_to_watts' keys (pv, meter,
    import_w, export_w -- after the limit --, charge_w, discharge_w, soc_wh, n_ok, covered) plus curtailed_w, each
    [..., n_bins]; fleet sums, or with mean=True the means per ok chain-second.  Bins of bin_s seconds are summed
    as integers first; a last partial bin is kept; a bin without an ok chain-second gives NaN.  The discharging
    power is [7] - sum of b with sum of b = [4] - [5] - [8] - ([1] - [0]), the row's identity."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.ndim < 2 or raw.shape[-1] != len(FLEET_COLUMNS):
        raise ValueError("raw dispatch fleet series must end in the 9 columns")
    bin_s = int(bin_s)
    if bin_s < 1:
        raise ValueError("bin_s must be >= 1")
    n_steps = raw.shape[-2]
    secs = np.ones(n_steps, dtype=np.int64)
    if bin_s > 1 and n_steps:
        edges = np.arange(0, n_steps, bin_s)
        raw, secs = np.add.reduceat(raw, edges, axis=-2), np.add.reduceat(secs, edges)
    n_ok = raw[..., 2]
    den = np.where(n_ok > 0, n_ok, np.nan).astype(np.float64)
    scale = float(1 << FRAC_BITS)
    div = den * scale if mean else np.where(n_ok > 0, scale, np.nan)
    dis = raw[..., 7] - (raw[..., 4] - raw[..., 5] - raw[..., 8] - (raw[..., 1] - raw[..., 0]))
    return {"pv": raw[..., 0] / div, "meter": raw[..., 1] / div, "import_w": raw[..., 4] / div,
            "export_w": raw[..., 5] / div, "charge_w": raw[..., 7] / div, "discharge_w": dis / div,
            "curtailed_w": raw[..., 8] / div,
            "soc_wh": raw[..., 6] / ((div if mean else div * secs) * 3600.0),
            "n_ok": n_ok.astype(np.float64), "covered": raw[..., 3] / den}


def fleet_peaks(raw, bin_s):
    """Per bin of bin_s seconds of a raw dispatch fleet table [..., n_steps, 9] (a last partial bin is kept): the
    fleet's highest import and highest feed-in of any one second in W and the second of each -- dict of
    peak_w_import, peak_w_export (float64 [..., n_bins]) and t_peak_import, t_peak_export (int64, seconds into the
    bin of the earliest second at the peak).  The coincident peak: what the feeder sees, not the sum of the chains'
    own peaks (table columns 11 and 12)."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.ndim < 2 or raw.shape[-1] != len(FLEET_COLUMNS):
        raise ValueError("raw dispatch fleet series must end in the 9 columns")
    bin_s = int(bin_s)
    if bin_s < 1:
        raise ValueError("bin_s must be >= 1")
    n_steps = raw.shape[-2]
    n_bins = -(-n_steps // bin_s)
    out = {}
    for name, col in (("import", 4), ("export", 5)):
        v = raw[..., col]
        pad = np.full(v.shape[:-1] + (n_bins * bin_s - n_steps,), -1, dtype=np.int64)   # (below every sum: never the peak)
        v = np.concatenate([v, pad], axis=-1).reshape(v.shape[:-1] + (n_bins, bin_s))
        out["peak_w_" + name] = v.max(axis=-1) / float(1 << FRAC_BITS)
        out["t_peak_" + name] = v.argmax(axis=-1).astype(np.int64)                       # (the first maximum)
    return out
