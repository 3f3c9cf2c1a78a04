"""Shared by the battery-sweep tests: the variants.  Variant 0 is battery_util.recipe's fleet; variant k is the
recipe with its columns rolled by k * ROLL chains, so every chain meets K different batteries (some of them
none: C = 0) and the CPU and the GPU tests speak of the same ones.  Every battery starts at min(C, 0.25 Wh).
K = 5 is above the kernels' variants per launch (SWEEP_KV = 4) and no multiple of it: a full group of
launches, a short last group and the one-launch rule of the statistics all run."""
import numpy as np

from battery_util import QUARTER_WH, recipe
from series_util import A_N

K = 5
ROLL = 37


def variants(k=K, n=A_N, base_n=A_N):
    """(params int64 [k, 6, n], soc0 int64 [k, n]): variant v is the recipe of base_n chains rolled by v * ROLL
    columns, tiled to n chains past base_n and cut to n."""
    par, _ = recipe(base_n)
    reps = -(-n // base_n)
    out = np.stack([np.tile(np.roll(par, v * ROLL, axis=1), (1, reps))[:, :n] for v in range(k)]).astype(np.int64)
    return np.ascontiguousarray(out), np.minimum(out[:, 0], QUARTER_WH).astype(np.int64)


def pair_shares(col4, live):
    """For every pair of variants (u < v), the share of the live chains whose column-4 totals over the run
    differ between the two: {(u, v): share}.  col4: [K, n_intervals, n]."""
    tot = col4.sum(axis=1)
    return {(u, v): float((tot[u, live] != tot[v, live]).mean()) for u in range(tot.shape[0]) for v in range(u + 1, tot.shape[0])}
