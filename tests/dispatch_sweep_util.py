"""Shared by the dispatch-sweep tests: two sets of K = 5 variants, so the CPU and the GPU tests speak of the same ones.

rolled: variant v is dispatch_util.recipe's nine rows and start rolled by v * ROLL chains, so every chain meets five
    different households' batteries, thresholds and limits and variant 0 is the dispatch tests' own input
    (which="C": dispatch_util.tiled's boundary input rolled the same way).
rules: every variant has the recipe's battery and start (rows 0-5 unchanged); only (Tc, Td, L) differ, uniform over
    the chains -- the user's case: one household, five rules.  Variants 0 and 1 differ in L alone.

K = 5 is above every candidate for the kernels' variants per launch (2, 3 or 4) and leaves a short last group or a
group of one whichever is built."""
import numpy as np

from dispatch_util import NO_LIMIT, W, recipe, tiled
from series_util import A_N

K = 5
ROLL = 37
# (Tc, Td, L) in W of the rules set; None: no feed-in limit
RULES = ((0, 0, None), (0, 0, 1000), (500, 0, 1000), (500, 2000, 1000), (1000, 0, 500))
MIN_ROLLED_SHARE = 0.9   # every pair of rolled variants: live chains whose column-4 totals differ (94.2-95.1 % on the oracle's traces)
MIN_RULES_SHARE = 0.7    # every pair of rules: live chains that differ in column 4, 5 or 10 (>= 75.9 %; 23.9 % have C = 0)


def rolled(k=K, n=A_N, which="A"):
    """(params int64 [k, 9, n], soc0 int64 [k, n]): the recipe (tiled to n chains past A_N) rolled by v * ROLL chains."""
    par, soc0 = recipe(A_N, which) if n == A_N else tiled(n, which)
    p = np.stack([np.roll(par, v * ROLL, axis=1) for v in range(k)]).astype(np.int64)
    s = np.stack([np.roll(soc0, v * ROLL) for v in range(k)]).astype(np.int64)
    return np.ascontiguousarray(p), np.ascontiguousarray(s)


def rules(n=A_N, rule_set=RULES):
    """(params int64 [K, 9, n], soc0 int64 [K, n]): the recipe's batteries and start under each of RULES."""
    par, soc0 = recipe(A_N) if n == A_N else tiled(n, "A")
    out = np.stack([par] * len(rule_set)).astype(np.int64)
    for v, (tc, td, lim) in enumerate(rule_set):
        out[v, 6], out[v, 7], out[v, 8] = tc * W, td * W, NO_LIMIT if lim is None else lim * W
    return np.ascontiguousarray(out), np.ascontiguousarray(np.stack([soc0] * len(rule_set)).astype(np.int64))


def pair_shares(table, live, cols):
    """For every pair of variants (u < v), the share of the live chains whose run totals differ between the two in
    any of the columns `cols`: {(u, v): share}.  table: [K, n_intervals, 13, n]."""
    tot = table[:, :, list(cols)].sum(axis=1)                              # [K, len(cols), n]
    return {(u, v): float((tot[u][:, live] != tot[v][:, live]).any(axis=0).mean())
            for u in range(tot.shape[0]) for v in range(u + 1, tot.shape[0])}


def rules_equalities(table, soc, live):
    """Variants 0 and 1 of the rules set differ only in L: the limit touches nothing but what is fed in and what is
    curtailed, so columns 0-4, 6-9 and the state of charge are equal, [5] + [10] is equal, and column 5 differs for
    nearly every live chain (99.4 % on the oracle's traces).  Exact."""
    for col in (0, 1, 2, 3, 4, 6, 7, 8, 9):
        np.testing.assert_array_equal(table[0, :, col], table[1, :, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(soc[0], soc[1])
    np.testing.assert_array_equal(table[0, :, 5] + table[0, :, 10], table[1, :, 5] + table[1, :, 10])
    assert not table[0, :, 10].any()
    return float((table[0, :, 5].sum(axis=0)[live] != table[1, :, 5].sum(axis=0)[live]).mean())
