"""The battery kind: battery storage with losses and per-chain batteries (tmh_battery).

`storage` puts a lossless battery of one size behind every meter.  Here each chain has its
own battery -- capacity C, charge and discharge limits Pc and Pd at the meter side, charge
and discharge efficiency ec and ed in units of 2^-16, and a standby drain sigma per ok
second -- as the six rows of an int64 array params [6, n] (`quantize_params`).  Everything
is an integer in the fleet series' units: powers in 2^-FRAC_BITS W, energies and the state
of charge (SoC) in 2^-FRAC_BITS W s.  With kc = ceil(2^32 / ec), kd = ceil(2^32 / ed), an ok
second with d = q(pv) - q(meter) and the SoC x before it (clamped into [0, C] when a window
reads it):

    a  = clamp(d, -Pd, Pc)                                   asked at the meter side
    s  = a >= 0 ?  (a ec) >> 16  :  -((-a kd + 65535) >> 16) stored (floor) / drained (ceil)
    x1 = clamp(x + s, 0, C)          g = x1 - x
    b  = a                                   if g == s       (not clipped)
       =  min( a, (g kc + 65535) >> 16)      if g > 0        (fills during this second)
       = -min(-a, (-g ed) >> 16)             if g < 0        (runs empty during this second)
       = 0                                   if g == 0
    x' = max(x1 - sigma, 0)
    import_b = max(b - d, 0)    export_b = max(d - b, 0)    loss = b - (x' - x)

A second that is not ok leaves x unchanged and adds nothing.  The engine fills an int64 tensor
[n_intervals, 10, n] (BatchedSim.enable_battery, tmh_set_battery; fp64 engines only):

    [k, 0:4, i] the interval table's columns (pv, meter, n_ok, covered), added
    [k, 4, i]   sum of import_b          [k, 5, i] sum of export_b
    [k, 6, i]   sum of max(b, 0)         [k, 7, i] sum of max(-b, 0)   (charged, discharged: meter side)
    [k, 8, i]   storage's SoC key: the maximum of ((o + 1) << 40) | x'
    [k, 9, i]   sum of loss

In every cell [4] - [5] == [1] - [0] + [6] - [7], columns 4-7 and 9 are >= 0 and [6] - [7] - [9]
is the interval's SoC change.  With ec = ed = 2^16 and sigma = 0 columns 0-8 and the SoC are
`storage`'s bit for bit and column 9 is 0.  s does not depend on x, so the second is still a
clamped addition (followed by the drain's): `second_maps` gives the per-second triples that
storage.compose / storage.apply fold, as the engine's map pass and scan do.  `from_traces` is the
contract as a plain loop over the seconds.

The battery fleet series (BatchedSim.enable_battery_fleet after enable_battery, tmh_set_battery_fleet)
is the same second summed over the chains instead of over an interval: an int64 tensor
[n_groups, n_steps, 8] whose row of a second holds, over the group's chains that are ok at it,

    [.., 0:4] the fleet series' columns (series.COLUMNS: pv, meter, n_ok, covered)
    [.., 4]   sum of import_b      [.., 5] sum of export_b
    [.., 6]   sum of x' (the state of charge after the second)      [.., 7] sum of max(b, 0)

with [4] - [5] == [1] - [0] + sum of b in every row.  `fleet_from_traces` is that contract as the same
loop over the seconds, `fleet_to_watts` its rows in W and Wh per bin.
"""
from __future__ import annotations

import numpy as np

from . import intervals, storage
from .intervals import FRAC_BITS, MAX_W, n_intervals, quantize   # the series' units, as the loaded library has them
from .storage import (HI, KEY_SHIFT, LO, MAX_CAPACITY, MAX_INTERVAL_S, MAX_POWER, apply, compose,   # noqa: F401
                      unpack_soc)

COLUMNS = storage.COLUMNS + ("loss",)
# a row of the battery fleet series (tmh_set_battery_fleet): the fleet series' columns and the battery's four
FLEET_COLUMNS = ("pv", "meter", "n_ok", "covered", "import", "export", "soc", "charge")
PARAMS = ("capacity", "p_charge", "p_discharge", "eff_charge", "eff_discharge", "standby")   # the rows of params
EFF_ONE, EFF_MIN = 1 << 16, 1 << 15
# each row's inclusive range (tmh_battery)
RANGES = ((0, MAX_CAPACITY - 1), (0, MAX_POWER), (0, MAX_POWER), (EFF_MIN, EFF_ONE), (EFF_MIN, EFF_ONE), (0, MAX_POWER))


def check_params(params):
    """params as an int64 [6, n] array, every row inside its range (ValueError otherwise)."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 2 or params.shape[0] != len(PARAMS) or params.dtype != np.int64:
        raise ValueError("battery params must be an int64 [6, n] array")
    for name, row, (lo, hi) in zip(PARAMS, params, RANGES):
        if row.size and (int(row.min()) < lo or int(row.max()) > hi):
            raise ValueError(f"battery {name} outside [{lo}, {hi}]: [{int(row.min())}, {int(row.max())}]")
    return params


def quantize_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, n=None):
    """The int64 [6, n] parameters of batteries given in Wh, W and efficiencies as floats in [0.5, 1], each
    a scalar or [n] (n: the longest argument's length when not given): watt-hours times 3600 * 2^FRAC_BITS,
    watts times 2^FRAC_BITS, efficiencies times 2^16, each rounded half to even.  Raises ValueError on
    anything outside tmh_battery's ranges (NaN included)."""
    e, p = 3600.0 * (1 << FRAC_BITS), float(1 << FRAC_BITS)
    args = [np.atleast_1d(np.asarray(v, dtype=np.float64)) for v in
            (capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w)]
    if any(a.ndim != 1 for a in args):
        raise ValueError("battery quantities are scalars or [n] arrays")
    if n is None:
        n = max(a.shape[0] for a in args)
    out = np.empty((len(PARAMS), int(n)), dtype=np.int64)
    for r, (name, a, scale, (lo, hi)) in enumerate(zip(PARAMS, args, (e, p, p, float(EFF_ONE), float(EFF_ONE), p), RANGES)):
        if a.shape[0] not in (1, n):
            raise ValueError(f"battery {name}: {a.shape[0]} values for {n} chains")
        q = np.rint(a * scale)
        if not bool(((q >= lo) & (q <= hi)).all()):   # (NaN fails both)
            raise ValueError(f"battery {name} {a[~((q >= lo) & (q <= hi))][0]!r} outside [{lo / scale:.6g}, {hi / scale:.6g}]")
        out[r] = q.astype(np.int64)
    return out


def quantize_soc(soc0_wh, params):
    """The starting SoC [n] of batteries `params` from watt-hours (a scalar or [n]); ValueError outside [0, C]."""
    n = params.shape[1]
    x0 = np.rint(np.broadcast_to(np.asarray(soc0_wh, dtype=np.float64), (n,)) * (3600.0 * (1 << FRAC_BITS)))
    if not bool(((x0 >= 0) & (x0 <= params[0])).all()):
        raise ValueError("battery soc0 outside [0, capacity]")
    return x0.astype(np.int64)


def _recip(e):
    return ((1 << 32) - 1) // e + 1   # ceil(2^32 / e)


def _stored(a, ec, kd):
    """s of the ask a: what it stores (floor) or drains (ceil)."""
    return np.where(a >= 0, (a * ec) >> 16, -((-a * kd + 65535) >> 16))


def _ok_d(pv, meter, covered):
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    return ok, np.where(ok, quantize(pv) - quantize(meter), 0).astype(np.int64)


def second_maps(pv, meter, covered, *, params):
    """The per-second triples of traces [n_steps, n] with the batteries params [6, n]: the clamped
    addition (s, 0, C) composed with the standby drain's (-sigma, 0, C) for an ok second, the identity
    otherwise; int64 arrays [n_steps, n] each (storage.compose, storage.apply)."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    cap, pc, pd, ec, ed, sb = check_params(params)
    ok, d = _ok_d(pv, meter, covered)
    s = _stored(np.clip(d, -pd, pc), ec, _recip(ed))
    a, lo, hi = compose((s, 0, np.broadcast_to(cap, s.shape)), (-sb, 0, cap))
    return np.where(ok, a, 0), np.where(ok, lo, LO).astype(np.int64), np.where(ok, hi, HI).astype(np.int64)


def _second(x, d, params):
    """One second of every chain: (b, x') of the SoC x before it and d = q(pv) - q(meter), as if the second
    were ok (the caller keeps x where it is not)."""
    cap, pc, pd, ec, ed, sb = params
    a = np.clip(d, -pd, pc)
    s = _stored(a, ec, _recip(ed))
    x1 = np.clip(x + s, 0, cap)
    g = x1 - x
    fill = np.minimum(a, (g * _recip(ec) + 65535) >> 16)
    drain = -np.minimum(-a, (-g * ed) >> 16)
    b = np.where(g == s, a, np.where(g > 0, fill, np.where(g < 0, drain, 0)))
    return b, np.maximum(x1 - sb, 0)


def from_traces(pv, meter, covered, interval_s, *, params, soc0, origin=0):
    """The battery table of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_intervals, 10, n_chains], int64 [n_chains]).  A plain loop over the seconds, vectorised over the
    chains.  params: int64 [6, n_chains] inside their ranges; soc0: the SoC before the first second, a
    scalar or [n_chains], clamped into [0, C]; ok seconds, interval_s and origin as intervals.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"battery params for {params.shape[1]} chains, traces of {n}")
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :4] = base
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, params[0])
    ok, d_all = _ok_d(pv, meter, covered)
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        oks, d = ok[t], d_all[t]
        b, xn = _second(x, d, params)
        row = out[k]
        row[4] += np.where(oks, np.maximum(b - d, 0), 0)
        row[5] += np.where(oks, np.maximum(d - b, 0), 0)
        row[6] += np.where(oks, np.maximum(b, 0), 0)
        row[7] += np.where(oks, np.maximum(-b, 0), 0)
        row[8] = np.where(oks, ((o + 1) << KEY_SHIFT) | xn, row[8])                 # later seconds have larger keys
        row[9] += np.where(oks, b - (xn - x), 0)
        x = np.where(oks, xn, x)
    return out, x


def fleet_from_traces(pv, meter, covered, *, params, soc0, group_chains=0):
    """The battery fleet series of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_groups, n_steps, 8], int64 [n_chains]).  The same loop over the seconds as from_traces, summed over the
    chains of a group instead of the seconds of an interval: row t of a group holds, over its chains that are
    ok at second t, FLEET_COLUMNS -- series.from_traces' four columns, the sums of import_b and export_b, of
    the SoC x' after the second and of max(b, 0).  params, soc0: as from_traces; groups as series.from_traces
    (chain i in group i // group_chains, 0: one group, else a multiple of 512; the last may be partial)."""
    from . import series
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = series.from_traces(pv, meter, covered, group_chains)                   # (checks the arguments)
    n_steps, n = pv.shape
    params = check_params(params)
    if params.shape[1] != n:
        raise ValueError(f"battery params for {params.shape[1]} chains, traces of {n}")
    n_groups = base.shape[0]
    gc = int(group_chains) or max(n, 1)
    out = np.zeros((n_groups, n_steps, len(FLEET_COLUMNS)), dtype=np.int64)
    out[..., :4] = base
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)), 0, params[0])
    ok, d_all = _ok_d(pv, meter, covered)
    for t in range(n_steps):
        oks, d = ok[t], d_all[t]
        b, xn = _second(x, d, params)
        x = np.where(oks, xn, x)
        cols = np.stack([np.maximum(b - d, 0), np.maximum(d - b, 0), x, np.maximum(b, 0)])
        cols = np.where(oks, cols, 0)
        for g in range(n_groups):
            out[g, t, 4:] = cols[:, g * gc:(g + 1) * gc].sum(axis=1)
    return out, x


SWEEP_MAX = 16   # TMH_BATTERY_SWEEP_MAX: the variants of one battery sweep


def check_sweep_params(params):
    """Sweep parameters as an int64 [K, 6, n] array, 1 <= K <= SWEEP_MAX, every variant inside tmh_battery's
    ranges (check_params per variant; ValueError otherwise)."""
    params = np.asarray(params.cpu() if hasattr(params, "cpu") else params)
    if params.ndim != 3 or params.shape[1] != len(PARAMS) or params.dtype != np.int64:
        raise ValueError("battery sweep params must be an int64 [K, 6, n] array")
    if not 1 <= params.shape[0] <= SWEEP_MAX:
        raise ValueError(f"battery sweep: {params.shape[0]} variants outside [1, {SWEEP_MAX}]")
    for p in params:
        check_params(p)
    return params


def quantize_sweep_params(capacity_wh, charge_w, discharge_w, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, *, n,
                          n_variants=None):
    """The int64 [K, 6, n] parameters of a battery sweep: each quantity a scalar (every variant and chain), a
    sequence of K values (one per variant, uniform over the chains) or a [K, n] array; quantised per variant
    by quantize_params.  K is n_variants when given, else the longest argument's length; ValueError when an
    argument's length is neither 1 nor K or K is outside [1, SWEEP_MAX]."""
    args = [np.asarray(v, dtype=np.float64) for v in (capacity_wh, charge_w, discharge_w, charge_eff, discharge_eff, standby_w)]
    if any(a.ndim > 2 for a in args):
        raise ValueError("battery sweep quantities are scalars, [K] sequences or [K, n] arrays")
    k = int(n_variants) if n_variants is not None else max([a.shape[0] for a in args if a.ndim] or [1])
    if not 1 <= k <= SWEEP_MAX:
        raise ValueError(f"battery sweep: {k} variants outside [1, {SWEEP_MAX}]")
    for name, a in zip(PARAMS, args):
        if a.ndim and a.shape[0] not in (1, k):
            raise ValueError(f"battery sweep {name}: {a.shape[0]} values for {k} variants")
        if a.ndim == 2 and a.shape[1] not in (1, int(n)):
            raise ValueError(f"battery sweep {name}: {a.shape[1]} values for {n} chains")
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
    """The battery sweep of time-major traces [n_steps, n_chains]: every chain behind each of K batteries --
    (int64 [K, n_intervals, 10, n_chains], int64 [K, n_chains]), variant v what from_traces gives for params[v]
    and soc0[v].  One loop over the seconds with the state [K, n]: the second's rule is written out here on
    [K, n] arrays, apart from from_traces and _second, so that comparing the two compares two derivations.
    params: int64 [K, 6, n_chains]; soc0: a scalar, [K, 1] or [K, n_chains], clamped into [0, C]."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin = int(interval_s), int(origin)
    if interval_s > MAX_INTERVAL_S:
        raise ValueError("interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    params = check_sweep_params(params)
    if params.shape[2] != n:
        raise ValueError(f"battery sweep params for {params.shape[2]} chains, traces of {n}")
    K = params.shape[0]
    cap, pc, pd, ec, ed, sb = (params[:, r] for r in range(6))              # [K, n] each
    kc, kd = ((1 << 32) - 1) // ec + 1, ((1 << 32) - 1) // ed + 1
    out = np.zeros((K, base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :, :4] = base[None]
    x = np.clip(np.broadcast_to(np.asarray(soc0, dtype=np.int64), (K, n)), 0, cap)
    nan = np.isnan(pv) | np.isnan(meter) | (covered == 255)
    qd = np.where(nan, 0, quantize(pv) - quantize(meter)).astype(np.int64)
    for t in range(n_steps):
        k, o = divmod(origin + t, interval_s)
        oks, d = ~nan[t][None], qd[t][None]                                 # [1, n] against the variants' [K, n]
        ask = np.minimum(np.maximum(d, -pd), pc)
        up = ask >= 0
        mag = np.abs(ask)
        stored = np.where(up, (mag * ec) >> 16, -((mag * kd + 65535) >> 16))
        x1 = np.minimum(np.maximum(x + stored, 0), cap)
        moved = x1 - x
        cost = np.where(moved > 0, (moved * kc + 65535) >> 16, (-moved * ed) >> 16)   # at the meter side, unsigned
        clipped = np.sign(moved) * np.minimum(mag, cost)
        b = np.where(moved == stored, ask, clipped)
        xn = np.maximum(x1 - sb, 0)
        cell = out[:, k]
        cell[:, 4] += np.where(oks, np.maximum(b - d, 0), 0)
        cell[:, 5] += np.where(oks, np.maximum(d - b, 0), 0)
        cell[:, 6] += np.where(oks, np.maximum(b, 0), 0)
        cell[:, 7] += np.where(oks, np.maximum(-b, 0), 0)
        cell[:, 8] = np.where(oks, ((o + 1) << KEY_SHIFT) | xn, cell[:, 8])
        cell[:, 9] += np.where(oks, b - (xn - x), 0)
        x = np.where(oks, xn, x)
    return out, x


def sweep_summary(raw, interval_s, params, fleet=False):
    """Per variant and chain, over all the intervals of a raw sweep table [K, n_intervals, 10, n] with the
    parameters [K, 6, n]: dict of float64 [K, n] arrays (fleet=True: [K], of the integer totals over the chains,
    the capacity's included) -- energy_wh_pv, energy_wh_meter, energy_wh_import,
    energy_wh_export, energy_wh_charge, energy_wh_discharge, energy_wh_loss (Wh), self_consumption = (pv -
    export) / pv, self_sufficiency = (meter - import) / meter (NaN where the denominator is 0) and full_cycles =
    discharged Wh / capacity (NaN for a chain without a battery, C = 0).  The columns are summed over the
    intervals as integers first and turned into floats once, as fleet_to_watts does.  (interval_s: the table's,
    checked only; the sums do not depend on it.)"""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    params = check_sweep_params(params)
    if raw.ndim != 4 or raw.shape[2] != len(COLUMNS) or raw.shape[0] != params.shape[0] or raw.shape[3] != params.shape[2]:
        raise ValueError("raw battery sweep table must be [K, n_intervals, 10, n] with params [K, 6, n]")
    if int(interval_s) < 1:
        raise ValueError("interval_s must be >= 1")
    tot, cap = raw.sum(axis=1), params[:, 0]                               # [K, 10, n] (column 8 is a key: unused)
    if fleet:
        tot, cap = tot.sum(axis=2), cap.sum(axis=1)
    e = float(1 << FRAC_BITS) * 3600.0
    pv, meter, imp, exp, ch, dis, loss = (tot[:, c] for c in (0, 1, 4, 5, 6, 7, 9))
    nz = lambda a: np.where(a != 0, a, np.nan).astype(np.float64)
    return {"energy_wh_pv": pv / e, "energy_wh_meter": meter / e, "energy_wh_import": imp / e,
            "energy_wh_export": exp / e, "energy_wh_charge": ch / e, "energy_wh_discharge": dis / e,
            "energy_wh_loss": loss / e, "self_consumption": (pv - exp) / nz(pv),
            "self_sufficiency": (meter - imp) / nz(meter), "full_cycles": dis / nz(cap)}


def fleet_to_watts(raw, bin_s=1, mean=False):
    """float64 series of a raw battery fleet table [..., n_steps, 8]: dict of pv, meter, import_w, export_w,
    charge_w, discharge_w (W) and soc_wh (Wh) -- fleet sums, or with mean=True the means per ok chain-second
    -- n_ok (ok chain-seconds per bin) and covered (the fraction of them under cloud), each [..., n_bins].
    Bins of bin_s seconds are summed as integers first, as series.to_watts does; the state of charge of a bin
    is its seconds' mean (of the fleet's total, or per ok chain-second); a last partial bin is kept; a bin
    without an ok chain-second gives NaN.  The discharging power is [7] - sum of b with sum of b = [4] - [5] -
    ([1] - [0]), the row's identity."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.ndim < 2 or raw.shape[-1] != len(FLEET_COLUMNS):
        raise ValueError("raw battery fleet series must end in the 8 columns")
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
    dis = raw[..., 7] - (raw[..., 4] - raw[..., 5] - (raw[..., 1] - raw[..., 0]))
    return {"pv": raw[..., 0] / div, "meter": raw[..., 1] / div, "import_w": raw[..., 4] / div,
            "export_w": raw[..., 5] / div, "charge_w": raw[..., 7] / div, "discharge_w": dis / div,
            "soc_wh": raw[..., 6] / ((div if mean else div * secs) * 3600.0),
            "n_ok": n_ok.astype(np.float64), "covered": raw[..., 3] / den}


def to_registers(raw):
    """The registers table [n_intervals, 6, n] of the meter behind the battery (the first six columns; a view)."""
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw battery table must be [n_intervals, 10, n]")
    return raw[:, :6]


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 10, n]: storage.to_watts' keys (charge and discharge at the
    meter side) plus energy_wh_loss (Wh lost in conversion and standby) and round_trip = discharged /
    (charged - the interval's SoC change), the share of what went in and is no longer stored that came out
    again -- NaN where the denominator is 0.  n_steps, when given, is checked against the interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw battery table must be [n_intervals, 10, n]")
    out = storage.to_watts(raw[:, :9], interval_s, n_steps=n_steps)
    e = float(1 << FRAC_BITS) * 3600.0
    dsoc = raw[:, 6] - raw[:, 7] - raw[:, 9]
    den = raw[:, 6] - dsoc
    out.update({"energy_wh_loss": raw[:, 9] / e,
                "round_trip": raw[:, 7] / np.where(den != 0, den, np.nan).astype(np.float64)})
    return out
