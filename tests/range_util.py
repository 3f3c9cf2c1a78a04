"""Shared by the range-end tests: inputs that put the integer table kinds at the ends of the ranges tmhpvsim.h
documents, so the CPU and the GPU tests speak of the same ones.

Input D: a fleet clipped at the inverter.  A's parameters with 130 modules behind an inverter whose Paco is
16383.75 W -- representable in fp32, one quantum of 2^-2 W under TMH_SERIES_MAX_W, q(Paco) = 67,107,840 -- at midday,
so nearly every ok chain-second sits exactly at Paco and a half-wave of 32 such lanes sums to 2^31 - 32,768, the
largest int32 partial the series' bound allows.
The corner recipe: every battery and dispatch parameter of every chain at an end of its range (or one step inside
it), the state of charge starting at an end of [0, C].
The clamp pattern: out-of-range values written over valid device tensors after enable_*, as a C caller could pass
them; the kernels clamp each into its range as a lane loads it."""
import dataclasses
import functools

import numpy as np

from series_util import A_CHAIN0, A_N, A_TZ, a_params
from storage_util import modules_params

# ---- input D
D_PACO = 16383.75
D_Q = 67107840                       # q(Paco) = Paco * 2^12
D_HALF_WAVE = 32 * D_Q               # 2,147,450,880 = 2^31 - 32,768
D_N, D_CHAIN0, D_STEPS = 1000, A_CHAIN0, 1300
D_START, D_TZ = "2019-09-05 12:30:00", A_TZ
D_WINDOWS = (517, 783)               # the second window starts off the 4-step and the 128-step grid
# conditions on D (observed on the oracle's traces: 3,523 pairs, a share of 0.943, 24 chains)
D_MIN_PAIRS, D_MIN_SHARE, D_MIN_DEAD = 1000, 0.9, 10

# ---- input C as the boundary tests run it (test_gpu_registers: asserted equal there)
C_START, C_STEPS, C_WINDOWS, C_LEAD = "2019-09-05 06:58:00", 2405, (1100, 1305), 3

INT64_MAX, INT64_MIN = np.iinfo(np.int64).max, np.iinfo(np.int64).min


def d_params():
    """A's parameters with 130 modules and the inverter scaled to Paco = 16383.75 W exactly."""
    mp = a_params()
    mod, inv = dict(mp.module), dict(mp.inverter)
    mod["Impo"] *= 130
    k = D_PACO / inv["Paco"]
    for key in ("Paco", "Pdco", "Pso", "Pnt"):
        inv[key] *= k
    inv["C0"] /= k
    inv["Paco"] = D_PACO
    assert inv["Paco"] == 16383.75 and float(np.float32(inv["Paco"])) == inv["Paco"] and inv["Paco"] < 16384.0
    assert inv["Paco"] * 4096 == D_Q and D_HALF_WAVE == (1 << 31) - 32768
    return dataclasses.replace(mp, module=mod, inverter=inv)


@functools.lru_cache(maxsize=None)
def d_oracle():
    """The oracle's fp64 traces of D: dict(pv, meter, covered [steps, n], status [n])."""
    from oracle import oracle as O
    ref = O.run(d_params(), D_CHAIN0, D_N, D_STEPS, D_START, tz=D_TZ, n_threads=8, outputs=("covered", "pv", "meter"))
    for v in ref.values():
        v.setflags(write=False)
    return ref


def d_conditions(pv, cov, status):
    """What makes D bite, of traces [steps, n]: the (step, half-wave) pairs whose 32 consecutive chains' q(pv) sum to
    exactly D_HALF_WAVE (chains grouped by chain // 32, full groups only), the share of the ok chain-seconds that sit
    exactly at Paco, the chains dead at construction and those that fault inside the window."""
    from tmhpvsim_amd import series
    pv, cov, status = np.asarray(pv), np.asarray(cov), np.asarray(status)
    ok = ~(np.isnan(pv) | (cov == 255))
    q = np.where(ok, series.quantize(pv), 0)
    full = pv.shape[1] // 32 * 32
    sums = q[:, :full].reshape(pv.shape[0], full // 32, 32).sum(axis=2)
    assert int(sums.max()) <= D_HALF_WAVE
    dead = status == 1
    return dict(pairs=int((sums == D_HALF_WAVE).sum()), share=float((q[ok] == D_Q).mean()), dead=int(dead.sum()),
                in_window=int(((cov[-1] == 255) & (cov[0] != 255)).sum()))


def assert_d_bites(pv, cov, status):
    c = d_conditions(pv, cov, status)
    assert c["pairs"] >= D_MIN_PAIRS and c["share"] >= D_MIN_SHARE and c["dead"] >= D_MIN_DEAD, c
    return c


# ---- the corner recipe
W = 1 << 12
CAP_TOP = (1 << 40) - 1
# observed on the oracle's 60-module traces of A at interval_s = 900; the tests assert half of each or more
CORNER_OBSERVED = dict(soc_top_cells=1336, ed_min_discharged=60, ec_min_charged=109, no_feed_in_curtailed=248,
                       pc_top_charged=136, partial_fill=69683, partial_empty=20946, curtail_full=73259, loss_chains=592)


def corners(n=A_N):
    """(params int64 [9, n], soc0 int64 [n]): each row drawn from the two ends of its range, one value next to an end
    and one ordinary value; rows 0-5 are the battery kind's.  soc0 is 0, C // 2, C - 1 or C."""
    rng = np.random.default_rng(23)
    pick = lambda vals: np.array(vals, dtype=np.int64)[rng.integers(0, len(vals), n)]
    effs = [1 << 15, (1 << 15) + 1, (1 << 16) - 1, 1 << 16]
    cap = pick([0, 1, 3686400, CAP_TOP])
    pc = pick([0, 1, 1000 * W, 1 << 27])
    pd = pick([0, 1, 3000 * W, 1 << 27])
    ec = pick(effs)
    ed = pick(effs)
    sb = pick([0, 1, 3 * W, 1 << 27])
    tc = pick([0, 1, 500 * W, 1 << 27])
    td = pick([0, 1, 2000 * W, 1 << 27])
    lim = pick([0, 1, 1000 * W, 1 << 27])
    sel = rng.integers(0, 4, n)
    soc0 = np.where(sel == 0, 0, np.where(sel == 1, cap // 2, np.where(sel == 2, np.maximum(cap - 1, 0), cap)))
    return np.stack([cap, pc, pd, ec, ed, sb, tc, td, lim]).astype(np.int64), soc0.astype(np.int64)


def corner_counts(table, events, params):
    """CORNER_OBSERVED's quantities of a dispatch table [n_intervals, 13, n], and the largest state of charge any cell
    holds; the three per-second counts with dispatch_util.run's events (None: the table's counts alone)."""
    soc = table[:, 8] & ((1 << 40) - 1)
    tot = table[:, [6, 7, 9, 10]].sum(axis=0)                              # (the sums; columns 8, 11 and 12 are keys)
    charged, discharged, loss, curtailed = tot
    out = dict(soc_top_cells=int((soc >= 1 << 39).sum()), soc_max=int(soc.max()),
               ed_min_discharged=int(((params[4] == 1 << 15) & (discharged > 0)).sum()),
               ec_min_charged=int(((params[3] == 1 << 15) & (charged > 0)).sum()),
               no_feed_in_curtailed=int(((params[8] == 0) & (curtailed > 0)).sum()),
               pc_top_charged=int(((params[1] == 1 << 27) & (charged > 0)).sum()), loss_chains=int((loss > 0).sum()))
    if events is not None:
        out.update({name: events[name] for name in ("partial_fill", "partial_empty", "curtail_full")})
    return out


def assert_corners_bite(counts):
    """Half of each observed count or more (of those `counts` holds), and a state of charge at 2^40 - 1 exactly."""
    for name, seen in CORNER_OBSERVED.items():
        assert name not in counts or 2 * counts[name] >= seen, (name, counts[name], seen)
    assert counts["soc_max"] == CAP_TOP, counts["soc_max"]


def tile(a, n):
    """The last axis of an A_N-chain array tiled to n chains."""
    reps = -(-n // a.shape[-1])
    return np.ascontiguousarray(np.tile(a, (1,) * (a.ndim - 1) + (reps,))[..., :n])


def rolled_corners(k, n, roll=37):
    """(params int64 [k, 9, n], soc0 int64 [k, n]): the corner recipe (tiled to n chains) rolled by v * roll chains."""
    par, soc0 = corners()
    par, soc0 = tile(par, n), tile(soc0, n)
    p = np.stack([np.roll(par, v * roll, axis=1) for v in range(k)]).astype(np.int64)
    s = np.stack([np.roll(soc0, v * roll) for v in range(k)]).astype(np.int64)
    return np.ascontiguousarray(p), np.ascontiguousarray(s)


# ---- the clamp pattern
def poison(params, ranges, shift=0, stagger=False):
    """params [rows, n] with chain i of every row replaced by hi + 1, -1, INT64_MAX, INT64_MIN or left as it is,
    chosen by (i + row) % 5; ranges: the rows' inclusive (lo, hi); shift: the rows before this array's in a larger
    tensor (a sweep's variant v: v * rows).  Rows five apart get the same case under that rule -- a chain's Tc is below
    0 only where its Pc clamps to 0, its Td only where its Pd does, so the lower clamps of rows 6 and 7 cannot show.
    stagger: (i + row + row // 5) % 5 instead, which sets rows 5-8 one chain off rows 0-3."""
    out = np.array(params, dtype=np.int64)
    i = np.arange(out.shape[1])
    for row, (_, hi) in enumerate(ranges):
        m = (i + row + shift + (row // 5 if stagger else 0)) % 5
        for case, v in enumerate((hi + 1, -1, INT64_MAX, INT64_MIN)):
            out[row, m == case] = v
    return out


def poison_soc(soc0, cap, row):
    """soc0 [n] with the same pattern against [0, cap] (cap [n]: the clamped capacities), as row `row`."""
    out = np.array(soc0, dtype=np.int64)
    m = (np.arange(out.shape[0]) + row) % 5
    out[m == 0] = cap[m == 0] + 1
    for case, v in ((1, -1), (2, INT64_MAX), (3, INT64_MIN)):
        out[m == case] = v
    return out


def clip(params, ranges):
    """np.clip of every row into its range: what a lane makes of the row."""
    lo = np.array([r[0] for r in ranges], dtype=np.int64)[:, None]
    hi = np.array([r[1] for r in ranges], dtype=np.int64)[:, None]
    return np.clip(np.asarray(params, dtype=np.int64), lo, hi)


@functools.lru_cache(maxsize=None)
def c60_oracle(n):
    """The oracle's fp64 traces of input C with 60 modules: (pv, meter, covered) [C_STEPS, n]."""
    from oracle import oracle as O
    ref = O.run(modules_params(), A_CHAIN0, n, C_STEPS, C_START, tz=A_TZ, n_threads=8, outputs=("covered", "pv", "meter"))
    for v in ref.values():
        v.setflags(write=False)
    return ref["pv"], ref["meter"], ref["covered"]
