"""Interval metering: exact per-chain sums per metering interval (tmh_intervals).

What each household's interval meter reads: the engine adds, per chain and per interval
of interval_s seconds (900 and 3600 are the usual ones), integers to an int64 tensor
[n_intervals, 4, n] (BatchedSim.enable_intervals, tmh_set_intervals):

    [k, 0, i] sum of q(pv)      [k, 1, i] sum of q(meter)
    [k, 2, i] ok seconds        [k, 3, i] ok seconds with the covered bit set

over the seconds of interval k at which chain i is ok (live, before its fault), with the
fleet series' q(v) = rint(v * 2^FRAC_BITS) (round half to even).  The sums are integers,
so they do not depend on block, window, batch, compaction or shard order, and a table can
be checked bit for bit against traces: `from_traces` is the same contract in numpy.
Residual energy is column 1 minus column 0 over the same seconds.  It is the per-chain
dual of the fleet series (series.py), which keeps every second and sums over the chains.
"""
from __future__ import annotations

import numpy as np

from .series import FRAC_BITS, MAX_W, quantize   # the series' units, as the loaded library has them

COLUMNS = ("pv", "meter", "n_ok", "covered")


def n_intervals(n_steps, interval_s):
    """Intervals that cover n_steps steps: ceil(n_steps / interval_s); a last partial one is kept."""
    n_steps, interval_s = int(n_steps), int(interval_s)
    if n_steps < 0 or interval_s < 1:
        raise ValueError("n_steps >= 0 and interval_s >= 1")
    return -(-n_steps // interval_s)


def from_traces(pv, meter, covered, interval_s, origin=0):
    """The interval table of time-major traces [n_steps, n_chains] (numpy or tensors on any
    device): int64 [n_intervals, 4, n_chains].  A chain-second is ok unless its pv or meter
    is NaN or its covered byte is 255 (the engine's fault marks).  origin: the offset of the
    traces' first step from the intervals' step0, so trace row s belongs to interval
    (origin + s) // interval_s and the table covers origin + n_steps steps."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    if not pv.shape == meter.shape == covered.shape or pv.ndim != 2:
        raise ValueError("pv, meter and covered must be [n_steps, n_chains] alike")
    interval_s, origin = int(interval_s), int(origin)
    if interval_s < 1 or origin < 0:
        raise ValueError("interval_s >= 1 and origin >= 0")
    n_steps, n = pv.shape
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    cols = np.stack([np.where(ok, quantize(pv), 0), np.where(ok, quantize(meter), 0), ok.astype(np.int64),
                     (ok & (covered == 1)).astype(np.int64)], axis=1)          # [n_steps, 4, n]
    out = np.zeros((n_intervals(origin + n_steps, interval_s), 4, n), dtype=np.int64)
    if n_steps:
        k = (origin + np.arange(n_steps)) // interval_s
        first = np.flatnonzero(np.r_[True, k[1:] != k[:-1]])                   # the rows that begin an interval
        out[k[first]] = np.add.reduceat(cols, first, axis=0)
    return out


def to_watts(raw, interval_s, n_steps=None):
    """float64 views of a raw table [n_intervals, 4, n]: dict of pv, meter, residual (W: means
    over the interval's ok seconds), energy_wh_pv, energy_wh_meter, energy_wh_residual (Wh:
    sum of q / 2^FRAC_BITS / 3600), n_ok (ok seconds) and covered (the fraction of them
    under cloud), each [n_intervals, n].  A cell without an ok second gives NaN for the means
    and the fraction and 0 for the energies.  n_steps, when given, is checked against the
    table's interval count."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.ndim != 3 or raw.shape[1] != 4:
        raise ValueError("raw intervals must be [n_intervals, 4, n]")
    if n_steps is not None and n_intervals(n_steps, interval_s) != raw.shape[0]:
        raise ValueError(f"{raw.shape[0]} intervals do not cover {n_steps} steps of {interval_s} s")
    scale = float(1 << FRAC_BITS)
    qpv, qm, n_ok, ncov = raw[:, 0], raw[:, 1], raw[:, 2], raw[:, 3]
    den = np.where(n_ok > 0, n_ok, np.nan).astype(np.float64)   # an empty cell: NaN
    # (integers below 2^53 convert exactly and the scale is a power of two: one rounding per quotient)
    out = {"pv": qpv / (den * scale), "meter": qm / (den * scale), "residual": (qm - qpv) / (den * scale),
           "energy_wh_pv": qpv / scale / 3600.0, "energy_wh_meter": qm / scale / 3600.0,
           "energy_wh_residual": (qm - qpv) / scale / 3600.0, "n_ok": n_ok.astype(np.float64), "covered": ncov / den}
    return out
