"""Battery storage: a battery behind each household's meter and what the meter reads with it (tmh_storage).

The battery charges from the PV surplus and discharges into the deficit (greedy
self-consumption, lossless).  Its state of charge (SoC) depends on every earlier second of
the chain, so no other table can be post-processed into this one.  Everything is an integer
in the fleet series' units: powers in 2^-FRAC_BITS W, energies and the SoC in 2^-FRAC_BITS
W s.  For an ok second with d = q(pv) - q(meter), capacity C, charge limit Pc, discharge
limit Pd and the SoC x before it:

    a  = clamp(d, -Pd, Pc)        what the battery is asked to take (+) or give (-)
    x' = clamp(x + a, 0, C)
    g  = x' - x                   what it took / gave
    import_b = max(g - d, 0)      export_b = max(d - g, 0)

A second that is not ok leaves x unchanged.  The engine fills, per chain and per interval of
interval_s seconds, an int64 tensor [n_intervals, 9, n] (BatchedSim.enable_storage,
tmh_set_storage; fp64 engines only):

    [k, 0:4, i] the interval table's columns (pv, meter, n_ok, covered), added
    [k, 4, i]   sum of import_b          [k, 5, i] sum of export_b
    [k, 6, i]   sum of max(g, 0)         [k, 7, i] sum of max(-g, 0)   (charged, discharged)
    [k, 8, i]   the maximum of ((o + 1) << 40) | x', o the second's offset in the interval

so column 8 is the key of the interval's last ok second: `unpack_soc` gives the SoC at the
interval's end (or at the chain's fault); 0 means no ok second.  In every cell
[4] - [5] == [1] - [0] + [6] - [7], columns 4-7 are >= 0 and [6] - [7] is the interval's SoC
change.  A clamped addition x -> min(max(x + a, lo), hi) composes with another into a third,
exactly and associatively (`compose`, `apply`): the engine collapses each 128-second block
into one such triple, scans the blocks for their starting SoC and replays the seconds.
`from_traces` is the contract as a plain loop over the seconds.
"""
from __future__ import annotations

import numpy as np

from . import intervals
from .intervals import FRAC_BITS, MAX_W, n_intervals, quantize   # the series' units, as the loaded library has them

COLUMNS = intervals.COLUMNS + ("import", "export", "charge", "discharge", "soc_key")
KEY_SHIFT = 40
MAX_CAPACITY = 1 << 40      # capacity < 2^40
MAX_POWER = 1 << 27         # p_charge, p_discharge <= 2^27
MAX_INTERVAL_S = (1 << 23) - 1
LO, HI = -(1 << 62), (1 << 62) - 1   # the identity's bounds (INT64_MIN / 2, INT64_MAX / 2)
IDENTITY = (0, LO, HI)


def quantize_params(capacity_wh, charge_w, discharge_w, soc0_wh=0.0):
    """(capacity, p_charge, p_discharge, soc0) as the engine's integers: watt-hours times 3600 * 2^FRAC_BITS,
    watts times 2^FRAC_BITS, each rounded half to even; the ranges are tmh_set_storage's."""
    e, p = 3600.0 * (1 << FRAC_BITS), float(1 << FRAC_BITS)
    cap, pc, pd, x0 = (int(np.rint(v)) for v in (capacity_wh * e, charge_w * p, discharge_w * p, soc0_wh * e))
    if not 0 <= cap < MAX_CAPACITY:
        raise ValueError(f"capacity {capacity_wh} Wh outside [0, {MAX_CAPACITY / e:.4g}) Wh")
    if not (0 <= pc <= MAX_POWER and 0 <= pd <= MAX_POWER):
        raise ValueError(f"charge {charge_w} W, discharge {discharge_w} W outside [0, {MAX_POWER / p:.0f}] W")
    return cap, pc, pd, x0


def compose(f, g):
    """f first, then g: triples (a, lo, hi) of int64 arrays (or ints) meaning x -> min(max(x + a, lo), hi)."""
    a1, lo1, hi1 = (np.asarray(v, dtype=np.int64) for v in f)
    a2, lo2, hi2 = (np.asarray(v, dtype=np.int64) for v in g)
    return a1 + a2, np.minimum(np.maximum(lo1 + a2, lo2), hi2), np.minimum(np.maximum(hi1 + a2, lo2), hi2)


def apply(f, x):
    """min(max(x + a, lo), hi) for the triple f = (a, lo, hi)."""
    a, lo, hi = (np.asarray(v, dtype=np.int64) for v in f)
    return np.minimum(np.maximum(np.asarray(x, dtype=np.int64) + a, lo), hi)


def second_maps(pv, meter, covered, *, capacity, p_charge, p_discharge):
    """The per-second triples of traces [n_steps, n]: (clamp(d, -Pd, Pc), 0, C) for an ok second, the
    identity otherwise; int64 arrays [n_steps, n] each."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    d = np.where(ok, quantize(pv) - quantize(meter), 0).astype(np.int64)
    a = np.where(ok, np.clip(d, -int(p_discharge), int(p_charge)), 0)
    return a, np.where(ok, 0, LO).astype(np.int64), np.where(ok, int(capacity), HI).astype(np.int64)


def from_traces(pv, meter, covered, interval_s, *, capacity, p_charge, p_discharge, soc0, origin=0):
    """The storage table of time-major traces [n_steps, n_chains] and the SoC after them: (int64
    [n_intervals, 9, n_chains], int64 [n_chains]).  A plain loop over the seconds, vectorised over
    the chains.  soc0: the SoC before the first second, a scalar or [n_chains]; ok seconds,
    interval_s and origin as intervals.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)      # (checks the arguments)
    interval_s, origin, cap, pc, pd = int(interval_s), int(origin), int(capacity), int(p_charge), int(p_discharge)
    if not (0 <= cap < MAX_CAPACITY and 0 <= pc <= MAX_POWER and 0 <= pd <= MAX_POWER and interval_s <= MAX_INTERVAL_S):
        raise ValueError("capacity in [0, 2^40), p_charge and p_discharge in [0, 2^27], interval_s <= 2^23 - 1")
    n_steps, n = pv.shape
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :4] = base
    x = np.broadcast_to(np.asarray(soc0, dtype=np.int64), (n,)).copy()
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    d_all = np.where(ok, quantize(pv) - quantize(meter), 0).astype(np.int64)
    for s in range(n_steps):
        k, o = divmod(origin + s, interval_s)
        oks, d = ok[s], d_all[s]
        a = np.clip(d, -pd, pc)
        xn = np.where(oks, np.clip(x + a, 0, cap), x)
        g = xn - x
        row = out[k]
        row[4] += np.where(oks, np.maximum(g - d, 0), 0)
        row[5] += np.where(oks, np.maximum(d - g, 0), 0)
        row[6] += np.maximum(g, 0)
        row[7] += np.maximum(-g, 0)
        row[8] = np.where(oks, ((o + 1) << KEY_SHIFT) | xn, row[8])                 # later seconds have larger keys
        x = xn
    return out, x


def unpack_soc(key):
    """(soc, offset) of SoC keys: the SoC after the interval's last ok second and that second's offset
    in the interval; (0, -1) where the key is 0 (no ok second)."""
    key = np.asarray(key, dtype=np.int64)
    return key & ((1 << KEY_SHIFT) - 1), (key >> KEY_SHIFT) - 1


def to_registers(raw):
    """The registers table [n_intervals, 6, n] of the meter behind the battery (the first six columns: the
    intervals' four, import_b and export_b; a view)."""
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw storage must be [n_intervals, 9, n]")
    return raw[:, :6]


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 9, n]: the keys of intervals.to_watts, unchanged, plus
    energy_wh_import and energy_wh_export (Wh: drawn from the grid and fed in with the battery),
    energy_wh_charge and energy_wh_discharge (Wh into and out of the battery), soc_wh (the SoC after the
    interval's last ok second; NaN without one) and two ratios: self_consumption = (pv - export) / pv,
    the share of the PV energy not fed in (used on site or stored), and self_sufficiency = (meter -
    import) / meter, the share of the consumption not drawn from the grid -- NaN where the denominator's
    sum is 0.  n_steps, when given, is checked against the table's interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    out = intervals.to_watts(to_registers(raw)[:, :4], interval_s, n_steps=n_steps)
    e = float(1 << FRAC_BITS) * 3600.0
    qpv, qm = raw[:, 0], raw[:, 1]
    soc, off = unpack_soc(raw[:, 8])
    nan0 = lambda a: np.where(a != 0, a, np.nan).astype(np.float64)   # a zero denominator: NaN
    out.update({"energy_wh_import": raw[:, 4] / e, "energy_wh_export": raw[:, 5] / e, "energy_wh_charge": raw[:, 6] / e,
                "energy_wh_discharge": raw[:, 7] / e, "soc_wh": np.where(off >= 0, soc / e, np.nan),
                "self_consumption": (qpv - raw[:, 5]) / nan0(qpv), "self_sufficiency": (qm - raw[:, 4]) / nan0(qm)})
    return out
