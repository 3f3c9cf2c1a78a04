"""Shared by the battery-dispatch tests: the per-chain parameter recipe (battery_util.recipe's batteries plus a
charge threshold, a discharge threshold and a feed-in limit per chain, one draw order, so the CPU and the GPU
tests speak of the same households), and a sequential run written apart from dispatch.from_traces that gives
the table, the end state and the events a dispatch input must hold -- charges blocked and let through by the
charge threshold, discharges blocked and let through by the discharge threshold, seconds that curtail (while a
full battery clips the charge, while the battery charges), partial fills and partial empties, chains that curtail."""
import numpy as np

from battery_util import recipe as battery_recipe
from series_util import A_N

W = 1 << 12              # 1 W in the series' units
NO_LIMIT = 1 << 27       # 32768 W: no feed-in limit
# (tcs, tds, ls) in W of the main input (A: 60 modules from 05:30) and of the boundary input (C: sunrise)
LEVELS = {"A": ((0, 250, 500, 1000), (0, 2000, 4000, 6000), (250, 500, 1500, 32768)),
          "C": ((0, 50, 100, 200), (0, 2000, 4000, 6000), (50, 100, 300, 32768))}
# the main input's floors (the counts on the oracle's traces are two to three times these)
A_FLOORS = dict(charge_blocked=100000, charge_above=100000, discharge_blocked=1000000, discharge_above=50000,
                curtail=50000, curtail_full=20000, curtail_charging=20000, partial_fill=20000, partial_empty=50000,
                curtail_chains=300)


def recipe(n=A_N, which="A"):
    """(params int64 [9, n], soc0 int64 [n]): battery_util.recipe(n)'s six rows and start, then Tc, Td and L
    drawn in this order from the input's levels."""
    bat, soc0 = battery_recipe(n)
    tcs, tds, ls = (np.array(v, dtype=np.int64) * W for v in LEVELS[which])
    rng = np.random.default_rng(11)
    tc = tcs[rng.integers(0, 4, n)]
    td = tds[rng.integers(0, 4, n)]
    lim = ls[rng.integers(0, 4, n)]
    return np.vstack([bat, tc, td, lim]).astype(np.int64), soc0


def tiled(n, which):
    """The A_N-chain recipe tiled to n chains (the boundary tests run more chains than the recipe has)."""
    par, soc0 = recipe(A_N, which)
    reps = -(-n // A_N)
    return np.tile(par, (1, reps))[:, :n], np.tile(soc0, reps)[:n]


def run(pv, meter, cov, interval_s, params, soc0, origin=0):
    """(table int64 [n_intervals, 13, n], end state [n], events dict) of traces [steps, n]: the contract
    second by second from tmhpvsim.h's text, in magnitudes and signs rather than dispatch.py's selects."""
    pv, meter, cov = (np.asarray(a) for a in (pv, meter, cov))
    steps, n = pv.shape
    cap, pc, pd, ec, ed, sb, tc, td, lim = (np.asarray(r, dtype=np.int64) for r in params)
    kc, kd = -(-(1 << 32) // ec), -(-(1 << 32) // ed)
    ok = ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))
    q = lambda v: np.rint(np.where(ok, v, 0.0) * 4096.0).astype(np.int64)
    qp, qm = q(pv), q(meter)
    out = np.zeros((-(-(origin + steps) // interval_s), 13, n), dtype=np.int64)
    x = np.minimum(np.maximum(np.asarray(soc0, dtype=np.int64), 0), cap)
    ev = dict.fromkeys(A_FLOORS, 0)
    curtails = np.zeros(n, bool)
    for t in range(steps):
        k, off = divmod(origin + t, interval_s)
        o = ok[t]
        d = qp[t] - qm[t]
        sur, dfc = np.maximum(d, 0), np.maximum(-d, 0)                 # the second's surplus and deficit before the battery
        up = np.minimum(np.maximum(sur - tc, 0), pc)                     # asked to charge
        dn = np.minimum(np.maximum(dfc - td, 0), pd)                     # asked to discharge
        s = ((up * ec) >> 16) - ((dn * kd + 65535) >> 16)                # (one of up, dn is 0; ceil of 0 is 0)
        x1 = np.minimum(np.maximum(x + s, 0), cap)
        g = x1 - x
        took = np.where(g == s, up, np.minimum(up, (np.maximum(g, 0) * kc + 65535) >> 16))
        gave = np.where(g == s, dn, np.minimum(dn, (np.maximum(-g, 0) * ed) >> 16))
        xn = np.maximum(x1 - sb, 0)
        left = sur - took                                                # surplus behind the battery
        fed = np.minimum(left, lim)
        cut = left - fed
        imp = dfc - gave
        assert (took >= 0).all() and (gave >= 0).all() and (left >= 0).all() and (imp >= 0).all()
        assert ((took == 0) | (gave == 0)).all() and (np.where(o, took - gave - (xn - x), 0) >= 0).all()
        key = lambda v: np.where(o, (v << 32) | (0xFFFFFFFF - off), 0)
        cell = out[k]
        for col, v in ((0, qp[t]), (1, qm[t]), (2, 1), (3, cov[t] == 1), (4, imp), (5, fed), (6, took), (7, gave),
                       (9, took - gave - (xn - x)), (10, cut)):
            cell[col] += np.where(o, v, 0)
        cell[8] = np.where(o, ((off + 1) << 40) | xn, cell[8])
        cell[11] = np.maximum(cell[11], key(imp))
        cell[12] = np.maximum(cell[12], key(fed))
        cnt = lambda m: int((o & m).sum())
        ev["charge_blocked"] += cnt((tc > 0) & (d > 0) & (d <= tc))
        ev["charge_above"] += cnt((tc > 0) & (d > tc))
        ev["discharge_blocked"] += cnt((td > 0) & (-d > 0) & (-d <= td))
        ev["discharge_above"] += cnt((td > 0) & (-d > td) & (gave > 0))
        ev["curtail"] += cnt(cut > 0)
        ev["curtail_full"] += cnt((cut > 0) & (up > 0) & (g != s))
        ev["curtail_charging"] += cnt((cut > 0) & (took > 0))
        ev["partial_fill"] += cnt((g != s) & (g > 0))
        ev["partial_empty"] += cnt((g != s) & (g < 0))
        curtails |= o & (cut > 0)
        x = np.where(o, xn, x)
    ev["curtail_chains"] = int(curtails.sum())
    return out, x, ev


def identities(raw, params):
    """[4] - [5] == [1] - [0] + [6] - [7] + [10]; columns 4-7, 9 and 10 >= 0; the peak fed in <= L; the SoC key
    and both peak keys are set iff the cell has an ok second."""
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7] + raw[:, 10])
    assert (raw[:, 4:8] >= 0).all() and (raw[:, 9:11] >= 0).all()
    assert ((raw[:, 12] >> 32) <= np.asarray(params)[8]).all()
    for col in (8, 11, 12):
        np.testing.assert_array_equal(raw[:, col] != 0, raw[:, 2] > 0)


def soc_changes(raw, soc0, end):
    """[6] - [7] - [9] is each interval's change of the state of charge, from soc0 to the state after the run."""
    soc, off = raw[:, 8] & ((1 << 40) - 1), (raw[:, 8] >> 40) - 1
    prev = np.asarray(soc0, dtype=np.int64).copy()
    for k in range(raw.shape[0]):
        now = np.where(off[k] >= 0, soc[k], prev)
        np.testing.assert_array_equal(raw[k, 6] - raw[k, 7] - raw[k, 9], now - prev, err_msg=f"interval {k}")
        prev = now
    np.testing.assert_array_equal(prev, end)
