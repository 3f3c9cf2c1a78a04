"""Shared by the battery-kind tests: the per-chain parameter recipe (one draw order, so the CPU and the GPU
tests speak of the same batteries), uniform parameters from a storage battery, and the events a battery
input must hold -- seconds that fill or empty the battery partway (where the meter side is computed back
from what was stored), charges refused by a full battery, standby clipping at empty, chains with a loss."""
import numpy as np

from series_util import A_N

WH = 3600 << 12          # 1 Wh in the series' units (2^-12 W s)
QUARTER_WH = 3686400     # 0.25 Wh


def recipe(n=A_N):
    """(params int64 [6, n], soc0 int64 [n]) of the tests' fleet: capacities 0 (no battery), 0.25, 0.5 and
    0.75 Wh, charge limits 500 .. 2000 W, discharge limits 1000 .. 4000 W, efficiencies in [0.885, 1] with
    every 7th / 11th chain lossless, standby drains 0 .. 3 W; every battery starts at min(C, 0.25 Wh)."""
    rng = np.random.default_rng(7)
    cap = rng.integers(0, 4, n) * QUARTER_WH
    pc = rng.integers(1, 5, n) * 500 << 12
    pd = rng.integers(1, 5, n) * 1000 << 12
    ec = rng.integers(58000, 65537, n)
    ec[::7] = 65536
    ed = rng.integers(58000, 65537, n)
    ed[::11] = 65536
    sb = rng.integers(0, 4, n) << 12
    params = np.stack([cap, pc, pd, ec, ed, sb]).astype(np.int64)
    return params, np.minimum(cap, QUARTER_WH).astype(np.int64)


def uniform(n, capacity, p_charge, p_discharge, ec=65536, ed=65536, standby=0):
    """params [6, n] of n equal batteries."""
    return np.tile(np.array([[capacity], [p_charge], [p_discharge], [ec], [ed], [standby]], dtype=np.int64), (1, n))


def events(pv, meter, cov, params, soc0):
    """Counts over traces [steps, n] from a plain sequential run written apart from battery.from_traces:
    partial_fill / partial_empty -- ok seconds whose SoC change g differs from the stored amount s with
    g > 0 / g < 0; refused -- ok seconds with s > 0 and g == 0 (a full battery, or none, refuses a
    charge); standby_clip -- ok seconds where the drain would go below empty; loss_chains -- chains
    whose losses sum to more than 0."""
    from tmhpvsim_amd import battery
    pv, meter, cov = (np.asarray(a) for a in (pv, meter, cov))
    cap, pc, pd, ec, ed, sb = (np.asarray(r, dtype=np.int64) for r in params)
    kc, kd = ((1 << 32) - 1) // ec + 1, ((1 << 32) - 1) // ed + 1
    ok = ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))
    d = np.where(ok, battery.quantize(pv) - battery.quantize(meter), 0).astype(np.int64)
    x = np.clip(np.asarray(soc0, dtype=np.int64), 0, cap)
    loss = np.zeros(pv.shape[1], dtype=np.int64)
    fill = empty = refused = clip = 0
    for t in range(pv.shape[0]):
        o = ok[t]
        a = np.clip(d[t], -pd, pc)
        s = np.where(a >= 0, (a * ec) >> 16, -((-a * kd + 65535) >> 16))
        x1 = np.clip(x + s, 0, cap)
        g = x1 - x
        b = np.where(g == s, a, np.where(g > 0, np.minimum(a, (g * kc + 65535) >> 16),
                                         np.where(g < 0, -np.minimum(-a, (-g * ed) >> 16), 0)))
        xn = np.maximum(x1 - sb, 0)
        fill += int((o & (g != s) & (g > 0)).sum())
        empty += int((o & (g != s) & (g < 0)).sum())
        refused += int((o & (s > 0) & (g == 0)).sum())
        clip += int((o & (x1 - sb < 0)).sum())
        loss += np.where(o, b - (xn - x), 0)
        x = np.where(o, xn, x)
    return dict(partial_fill=fill, partial_empty=empty, refused=refused, standby_clip=clip,
                loss_chains=int((loss > 0).sum()))
