"""Demand registers: each household meter's maximum-demand registers (tmh_demand).

Beside the energies of an interval (registers.py) a meter keeps its maximum demand, and
sizing a feeder, a transformer or an inverter asks for exactly that: the highest power drawn
from the grid and the highest power fed in, and when each happened.  A maximum is non-linear,
so no sum table gives it.  The engine keeps, per chain and per interval of interval_s
seconds, an int64 tensor [n_intervals, 8, n] (BatchedSim.enable_demand, tmh_set_demand):

    [k, 0:6, i] the registers' columns (pv, meter, n_ok, covered, import, export), added
    [k, 6, i]   peak import: the maximum of key(max(q(meter) - q(pv), 0), o)
    [k, 7, i]   peak export: the maximum of key(max(q(pv) - q(meter), 0), o)

over the seconds of interval k at which chain i is ok, o the second's offset in the interval
and key(v, o) = (v << 32) | (0xFFFFFFFF - o): the high word is the peak in q units, the low
word gives the earliest second at which it occurred.  Every ok second's key is positive, so 0
means "no ok second" and is the identity of the maximum; an interval without feed-in has
key(0, its first ok second) in column 7.  Integer maxima are as order-free as the sums: the
bits do not depend on block, window, batch, compaction or shard order, and `from_traces` is
the same contract in numpy.
"""
from __future__ import annotations

import numpy as np

from . import registers
from .registers import FRAC_BITS, MAX_W, n_intervals, quantize   # the series' units, as the loaded library has them

COLUMNS = registers.COLUMNS + ("peak_import", "peak_export")
_LOW = 0xFFFFFFFF


def pack(v, o):
    """key(v, o): int64, the value v (q units, 0 <= v < 2^27) above the complement of the offset o."""
    return (np.asarray(v, dtype=np.int64) << 32) | (_LOW - np.asarray(o, dtype=np.int64))


def unpack(key):
    """(value, offset) of packed keys: int64 arrays; offset -1 (and value 0) where the key is 0."""
    key = np.asarray(key, dtype=np.int64)
    return key >> 32, np.where(key != 0, _LOW - (key & _LOW), -1)


def from_traces(pv, meter, covered, interval_s, origin=0):
    """The demand table of time-major traces [n_steps, n_chains] (numpy or tensors on any
    device): int64 [n_intervals, 8, n_chains]; ok seconds, interval_s and origin as
    registers.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = registers.from_traces(pv, meter, covered, interval_s, origin=origin)     # (checks the arguments)
    n_steps, n = pv.shape
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :6] = base
    if n_steps:
        ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
        d = np.where(ok, quantize(meter) - quantize(pv), 0).astype(np.int64)        # the second's net import, in q units
        s = int(origin) + np.arange(n_steps)
        k = s // int(interval_s)
        o = (s - k * int(interval_s))[:, None]
        keys = np.stack([np.where(ok, pack(np.maximum(d, 0), o), 0), np.where(ok, pack(np.maximum(-d, 0), o), 0)], axis=1)
        first = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])                        # the rows that begin an interval
        out[k[first], 6:] = np.maximum.reduceat(keys, first, axis=0)
    return out


def to_registers(raw):
    """The registers table [n_intervals, 6, n] inside a demand table (its first six columns; a view)."""
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw demand must be [n_intervals, 8, n]")
    return raw[:, :6]


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 8, n]: the keys of registers.to_watts,
    unchanged, plus peak_import and peak_export (W), t_peak_import and t_peak_export (seconds
    into the interval of the earliest second at the peak; NaN without an ok second) and
    load_factor = the mean import power over the ok seconds / the peak import (NaN where the
    peak is 0).  n_steps, when given, is checked against the table's interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    out = registers.to_watts(to_registers(raw), interval_s, n_steps=n_steps)
    scale = float(1 << FRAC_BITS)
    for name, col in (("import", 6), ("export", 7)):
        v, o = unpack(raw[:, col])
        out["peak_" + name] = v / scale
        out["t_peak_" + name] = np.where(o >= 0, o, np.nan).astype(np.float64)
    vi = unpack(raw[:, 6])[0]
    nz = lambda a: np.where(a != 0, a, np.nan).astype(np.float64)   # a zero denominator: NaN
    out["load_factor"] = raw[:, 4] / nz(raw[:, 2]) / nz(vi)
    return out
