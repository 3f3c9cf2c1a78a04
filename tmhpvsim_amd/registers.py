"""Import / export registers: what each household's bidirectional meter reads (tmh_registers).

A household with PV sits behind a meter with two registers (OBIS 1.8.0 / 2.8.0): what it
drew from the grid and what it fed in.  Both are non-linear per second, so the interval
meter's net (intervals.py: sum of pv, sum of meter) does not give them.  The engine adds,
per chain and per interval of interval_s seconds, integers to an int64 tensor
[n_intervals, 6, n] (BatchedSim.enable_registers, tmh_set_registers):

    [k, 0, i] sum of q(pv)      [k, 1, i] sum of q(meter)
    [k, 2, i] ok seconds        [k, 3, i] ok seconds with the covered bit set
    [k, 4, i] import = sum of max(q(meter) - q(pv), 0)
    [k, 5, i] export = sum of max(q(pv) - q(meter), 0)

over the seconds of interval k at which chain i is ok.  Columns 0-3 are the interval
table's (`to_intervals`); the registers are defined on the quantised integers, so for every
cell import - export == meter - pv bit for bit, and the self-consumed PV energy is
pv - export == meter - import.  Integer sums: the bits do not depend on block, window,
batch, compaction or shard order, and `from_traces` is the same contract in numpy.
"""
from __future__ import annotations

import numpy as np

from . import intervals
from .intervals import FRAC_BITS, MAX_W, n_intervals, quantize   # the series' units, as the loaded library has them

COLUMNS = ("pv", "meter", "n_ok", "covered", "import", "export")


def from_traces(pv, meter, covered, interval_s, origin=0):
    """The registers table of time-major traces [n_steps, n_chains] (numpy or tensors on any
    device): int64 [n_intervals, 6, n_chains]; ok seconds, interval_s and origin as
    intervals.from_traces."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    base = intervals.from_traces(pv, meter, covered, interval_s, origin=origin)     # (checks the arguments)
    n_steps, n = pv.shape
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    d = np.where(ok, quantize(meter) - quantize(pv), 0).astype(np.int64)            # the second's net import, in q units
    cols = np.stack([np.maximum(d, 0), np.maximum(-d, 0)], axis=1)                  # [n_steps, 2, n]
    out = np.zeros((base.shape[0], len(COLUMNS), n), dtype=np.int64)
    out[:, :4] = base
    if n_steps:
        k = (int(origin) + np.arange(n_steps)) // int(interval_s)
        first = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])                        # the rows that begin an interval
        out[k[first], 4:] = np.add.reduceat(cols, first, axis=0)
    return out


def to_intervals(raw):
    """The interval table [n_intervals, 4, n] inside a registers table (its first four columns; a view)."""
    if raw.ndim != 3 or raw.shape[1] != len(COLUMNS):
        raise ValueError("raw registers must be [n_intervals, 6, n]")
    return raw[:, :4]


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 6, n]: the keys of intervals.to_watts (pv,
    meter, residual, energy_wh_pv, energy_wh_meter, energy_wh_residual, n_ok, covered) plus
    energy_wh_import, energy_wh_export and energy_wh_self (Wh: the PV energy used behind the
    meter, pv - export) and two ratios: self_consumption = (pv - export) / pv, the share of
    the PV energy used on site, and self_sufficiency = (meter - import) / meter, the share of
    the consumption it covered -- NaN where the denominator's sum is 0 (no PV energy, or an
    empty cell).  n_steps, when given, is checked against the table's interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    out = intervals.to_watts(to_intervals(raw), interval_s, n_steps=n_steps)
    scale = float(1 << FRAC_BITS)
    qpv, qm, qim, qex = raw[:, 0], raw[:, 1], raw[:, 4], raw[:, 5]
    nan0 = lambda a: np.where(a != 0, a, np.nan).astype(np.float64)   # a zero denominator: NaN
    out.update({"energy_wh_import": qim / scale / 3600.0, "energy_wh_export": qex / scale / 3600.0,
                "energy_wh_self": (qpv - qex) / scale / 3600.0,
                "self_consumption": (qpv - qex) / nan0(qpv), "self_sufficiency": (qm - qim) / nan0(qm)})
    return out
