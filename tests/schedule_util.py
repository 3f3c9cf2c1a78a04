"""Shared by the scheduled-dispatch tests: the recipe (battery_util.recipe's batteries, four rule sets per chain
drawn in one order, and the rule array of each input, so the CPU and the GPU tests speak of the same households
and tariffs), and a sequential run written apart from schedule.from_traces -- in magnitudes and signs, from
tmhpvsim.h's text -- that gives the table, the end state and the events a schedule input must hold: seconds
that charge under a grid rule, that buy from the grid, grid charges a full battery clips, grid charging on top
of a surplus, hold seconds and rule changes met with the state of charge strictly inside (0, C), and seconds
that curtail."""
import numpy as np

from battery_util import recipe as battery_recipe
from dispatch_util import LEVELS, recipe as dispatch_recipe
from series_util import A_N

W = 1 << 12              # 1 W in the series' units
NO_LIMIT = 1 << 27       # no feed-in limit
HOLD = 1 << 27           # Tc = Td = HOLD: the battery neither charges nor discharges
R = 4
GS = {"A": (0, 20, 100, 400), "C": (0, 5, 20, 50)}      # the grid-charge powers in W of rule 1
A_RULES = np.array([1, 0, 2, 3, 0, 1, 1, 3, 2, 0, 3, 1, 0], dtype=np.uint8)   # input A: 13 intervals of 900 s
# the main input's floors (conditions on the input; the counts on the oracle's traces are well above them)
A_FLOORS = dict(grid_charge=500000, grid_buy=500000, grid_partial_fill=500000, grid_on_surplus=100, hold_inside=2000,
                change_inside=1000, curtail=50000)
EVENTS = tuple(A_FLOORS)


def c_rules(n_intervals):
    """The boundary input's rule array: (5 k + k // 3) % 4 over its intervals."""
    k = np.arange(int(n_intervals))
    return ((5 * k + k // 3) % 4).astype(np.uint8)


def recipe(n=A_N, which="A"):
    """(params int64 [6 + 4 R, n], soc0 int64 [n]): battery_util.recipe(n)'s six rows and start, then four rules --
    0: dispatch_util.recipe's rows 6-8 with G = 0; 1: Tc, Td, L and G drawn from the input's levels; 2: hold, L
    drawn, G = 0; 3: Tc, Td, L drawn, G = 0 -- in this order from default_rng(13)."""
    bat, soc0 = battery_recipe(n)
    tcs, tds, ls = (np.array(v, dtype=np.int64) * W for v in LEVELS[which])
    gs = np.array(GS[which], dtype=np.int64) * W
    rng = np.random.default_rng(13)
    draw = lambda levels: levels[rng.integers(0, 4, n)]
    zero, hold = np.zeros(n, dtype=np.int64), np.full(n, HOLD, dtype=np.int64)
    rule0 = list(dispatch_recipe(n, which)[0][6:9]) + [zero]
    rule1 = [draw(tcs), draw(tds), draw(ls), draw(gs)]
    rule2 = [hold, hold, draw(ls), zero]
    rule3 = [draw(tcs), draw(tds), draw(ls), zero]
    return np.vstack([bat] + rule0 + rule1 + rule2 + rule3).astype(np.int64), soc0


def tiled(n, which):
    """The A_N-chain recipe tiled to n chains (the boundary tests run more chains than the recipe has)."""
    par, soc0 = recipe(A_N, which)
    reps = -(-n // A_N)
    return np.tile(par, (1, reps))[:, :n], np.tile(soc0, reps)[:n]


def limits(params, rules):
    """The feed-in limit in force per interval and chain, [n_intervals, n]."""
    return np.asarray(params)[8 + 4 * np.asarray(rules, dtype=np.int64)]


def run(pv, meter, cov, interval_s, params, rules, soc0, origin=0):
    """(table int64 [n_intervals, 13, n], end state [n], events dict) of traces [steps, n]: the contract second
    by second, the battery's side in magnitudes (took, gave) rather than schedule.py's signed selects."""
    pv, meter, cov = (np.asarray(a) for a in (pv, meter, cov))
    steps, n = pv.shape
    params = np.asarray(params, dtype=np.int64)
    cap, pc, pd, ec, ed, sb = params[:6]
    kc, kd = -(-(1 << 32) // ec), -(-(1 << 32) // ed)
    ok = ~(np.isnan(pv) | np.isnan(meter) | (cov == 255))
    q = lambda v: np.rint(np.where(ok, v, 0.0) * 4096.0).astype(np.int64)
    qp, qm = q(pv), q(meter)
    out = np.zeros((-(-(origin + steps) // interval_s), 13, n), dtype=np.int64)
    assert len(rules) == out.shape[0]
    x = np.minimum(np.maximum(np.asarray(soc0, dtype=np.int64), 0), cap)
    ev = dict.fromkeys(EVENTS, 0)
    last_rule = None
    for t in range(steps):
        k, off = divmod(origin + t, interval_s)
        rule = int(rules[k])
        tc, td, lim, grid = params[6 + 4 * rule:10 + 4 * rule]
        o = ok[t]
        inside = (x > 0) & (x < cap)
        if last_rule is not None and rule != last_rule:
            ev["change_inside"] += int((o & inside).sum())
        last_rule = rule
        d = qp[t] - qm[t]
        sur, dfc = np.maximum(d, 0), np.maximum(-d, 0)                   # the second's surplus and deficit before the battery
        buys = grid > 0                                                  # a grid-charging rule: never discharges
        up = np.minimum(np.maximum(sur - tc, 0), pc)
        up = np.where(buys, np.minimum(up + grid, pc), up)               # asked to charge
        dn = np.where(buys, 0, np.minimum(np.maximum(dfc - td, 0), pd))  # asked to discharge
        s = ((up * ec) >> 16) - ((dn * kd + 65535) >> 16)                # (one of up, dn is 0; ceil of 0 is 0)
        x1 = np.minimum(np.maximum(x + s, 0), cap)
        g = x1 - x
        took = np.where(g == s, up, np.minimum(up, (np.maximum(g, 0) * kc + 65535) >> 16))
        gave = np.where(g == s, dn, np.minimum(dn, (np.maximum(-g, 0) * ed) >> 16))
        xn = np.maximum(x1 - sb, 0)
        bought = np.maximum(took - sur, 0)                               # what the charge exceeds the surplus by: from the grid
        left = sur - (took - bought)                                     # surplus behind the battery
        fed = np.minimum(left, lim)
        cut = left - fed
        imp = dfc - gave + bought
        assert (took >= 0).all() and (gave >= 0).all() and (left >= 0).all() and (imp >= 0).all()
        assert ((took == 0) | (gave == 0)).all() and (np.where(o, took - gave - (xn - x), 0) >= 0).all()
        assert (np.where(buys, 0, bought) == 0).all() and ((bought == 0) | (left == 0)).all()
        key = lambda v: np.where(o, (v << 32) | (0xFFFFFFFF - off), 0)
        cell = out[k]
        for col, v in ((0, qp[t]), (1, qm[t]), (2, 1), (3, cov[t] == 1), (4, imp), (5, fed), (6, took), (7, gave),
                       (9, took - gave - (xn - x)), (10, cut)):
            cell[col] += np.where(o, v, 0)
        cell[8] = np.where(o, ((off + 1) << 40) | xn, cell[8])
        cell[11] = np.maximum(cell[11], key(imp))
        cell[12] = np.maximum(cell[12], key(fed))
        cnt = lambda m: int((o & m).sum())
        ev["grid_charge"] += cnt(buys & (took > 0))
        ev["grid_buy"] += cnt(buys & (bought > 0))
        ev["grid_partial_fill"] += cnt(buys & (g != s) & (g > 0))
        ev["grid_on_surplus"] += cnt(buys & (sur > 0) & (took > sur))
        ev["hold_inside"] += cnt((tc == HOLD) & (td == HOLD) & ~buys & inside)
        ev["curtail"] += cnt(cut > 0)
        x = np.where(o, xn, x)
    return out, x, ev
