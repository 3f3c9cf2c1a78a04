"""Fleet aggregate time series: exact per-second sums over chains (tmh_series).

The engine adds, per second and per group of chains, integers to an int64 tensor
[n_groups, n_steps, 4] (BatchedSim.enable_series, tmh_set_series):

    [..., 0] sum of q(pv)      [..., 1] sum of q(meter)
    [..., 2] n_ok              [..., 3] ok chains with the covered bit set

over the chains that are ok at that second (live, before their fault), with
q(v) = rint(v * 2^FRAC_BITS) (round half to even; the scaling is exact).  The sums are
integers, so they do not depend on block, window, batch or shard order, and a series can
be checked bit for bit against traces: `from_traces` is the same contract in numpy.
Residual load is column 1 minus column 0 over the same chain-seconds.
"""
from __future__ import annotations

import numpy as np

from . import _lib

COLUMNS = ("pv", "meter", "n_ok", "covered")


def _units():
    L = _lib.load()
    return int(L.tmh_series_frac_bits()), float(L.tmh_series_max_w())


FRAC_BITS, MAX_W = _units()   # TMH_SERIES_FRAC_BITS / TMH_SERIES_MAX_W of the loaded library


def quantize(x):
    """q(x): int64 rint(x * 2^FRAC_BITS), round half to even; x is taken in its own precision
    (an fp32 value widens exactly, the power-of-two scaling is exact).  NaN gives 0 -- a
    second that is not ok adds nothing."""
    x = np.asarray(x)
    v = np.rint(x.astype(np.float64) * float(1 << FRAC_BITS))
    if v.size and not bool((np.abs(v[np.isfinite(v)]) < 2.0 ** 62).all()):
        raise OverflowError("value beyond the series' fixed-point range")
    return np.where(np.isfinite(v), v, 0.0).astype(np.int64)


def from_traces(pv, meter, covered, group_chains=0, n_groups=None):
    """The series of time-major traces [n_steps, n_chains] (numpy or tensors on any
    device): int64 [n_groups, n_steps, 4].  A chain-second is ok unless its pv or meter is
    NaN or its covered byte is 255 (the engine's fault marks).  Chain i belongs to group
    i // group_chains (0: one group); the last group may be partial.  n_groups: the groups
    of the result when a buffer has room for more than the chains fill (zeros)."""
    pv, meter, covered = (np.asarray(a.cpu() if hasattr(a, "cpu") else a) for a in (pv, meter, covered))
    if not pv.shape == meter.shape == covered.shape or pv.ndim != 2:
        raise ValueError("pv, meter and covered must be [n_steps, n_chains] alike")
    n_steps, n = pv.shape
    gc = int(group_chains)
    if gc < 0 or gc % 512:
        raise ValueError("group_chains must be 0 or a multiple of 512")
    ok = ~(np.isnan(pv) | np.isnan(meter) | (covered == 255))
    cols = np.stack([np.where(ok, quantize(pv), 0), np.where(ok, quantize(meter), 0), ok.astype(np.int64),
                     (ok & (covered == 1)).astype(np.int64)], axis=-1)          # [n_steps, n, 4]
    need = 1 if gc == 0 else max(1, -(-n // gc))
    n_groups = need if n_groups is None else int(n_groups)
    if n_groups < need:
        raise ValueError(f"{n_groups} groups of {gc} chains do not hold {n} chains")
    if gc == 0:
        gc = max(n, 1)
    out = np.zeros((n_groups, n_steps, 4), dtype=np.int64)
    for g in range(n_groups):
        out[g] = cols[:, g * gc:(g + 1) * gc].sum(axis=1, dtype=np.int64)
    return out


def to_watts(raw, bin_s=1, mean=False):
    """float64 series of raw sums [..., n_steps, 4]: dict of pv, meter, residual (W: fleet
    sums, or with mean=True the means per ok chain-second), n_ok (ok chain-seconds per bin)
    and covered (the fraction of them under cloud), each [..., n_bins].  Bins of bin_s
    seconds are summed as integers first; a last partial bin is kept; means divide by the
    bin's n_ok, and a bin without an ok chain-second gives NaN (means and fraction)."""
    raw = np.asarray(raw.cpu() if hasattr(raw, "cpu") else raw).astype(np.int64, copy=False)
    if raw.shape[-1] != 4:
        raise ValueError("raw series must end in the 4 columns")
    bin_s = int(bin_s)
    if bin_s < 1:
        raise ValueError("bin_s must be >= 1")
    n_steps = raw.shape[-2]
    if bin_s > 1:
        edges = np.arange(0, n_steps, bin_s)
        raw = np.add.reduceat(raw, edges, axis=-2) if n_steps else raw
    scale = float(1 << FRAC_BITS)
    n_ok = raw[..., 2]
    den = np.where(n_ok > 0, n_ok, np.nan).astype(np.float64)   # an empty bin: NaN
    cov = raw[..., 3] / den
    # (integers below 2^53 convert exactly and the scale is a power of two: one rounding per quotient)
    div = den * scale if mean else np.where(n_ok > 0, scale, np.nan)
    pv, meter, res = raw[..., 0] / div, raw[..., 1] / div, (raw[..., 1] - raw[..., 0]) / div
    return {"pv": pv, "meter": meter, "residual": res, "n_ok": n_ok.astype(np.float64), "covered": cov}


def all_reduce_series(raw, group=None):
    """The fleet series of every rank of `group`: one int64 SUM all-reduce (exact and
    order-free, like dist.all_reduce_stats).  Returns a new tensor; every rank gets it.
    Without an initialised process group: a copy."""
    import torch
    import torch.distributed as dist
    t = torch.as_tensor(raw).to(torch.int64).clone()
    if dist.is_available() and dist.is_initialized():
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    return t
