"""Shared by the schedule-sweep tests: two sets of K = 5 variants, so the CPU and the GPU tests speak of the same ones.

rolled: variant v is schedule_util.recipe's params and start rolled by v * ROLL chains, with the array np.roll(A_RULES, v):
    every chain meets five different households' batteries and rule sets under five shifted tariffs, and variant 0 is
    the schedule tests' own input (which="C": schedule_util.tiled's boundary input rolled the same way, with
    np.roll(c_rules(n_iv), v)).
tariffs: one household under five arrays -- the recipe's params and start unchanged in every variant; the arrays are
    A_RULES, rule 0 throughout, np.roll(A_RULES, 1), rule 2 (hold) throughout and A_RULES reversed.  Only the array
    differs, so a kernel that reads another variant's array row fails here and nowhere in columns 0-3.

K = 5 is above every candidate for the kernels' variants per launch (2, 3 or 4) and leaves a short last group or a
group of one whichever is built."""
import numpy as np

from schedule_util import A_RULES, c_rules, recipe, tiled
from series_util import A_N

K = 5
ROLL = 37
# shares of the live chains that differ between every pair of variants (conditions on the inputs; counted on the
# oracle's 60-module traces of input A: 976 of 1,000 chains live, 24.0 % of them with C = 0)
MIN_ROLLED_SHARE = 0.9     # rolled, run total of column 4: 94.3-95.1 %
MIN_TARIFFS_SHARE4 = 0.7   # tariffs, column 4: 75.9-76.0 % (chains without a battery cannot tell)
MIN_TARIFFS_SHARE = 0.9    # tariffs, columns 4, 5 or 10: >= 94.1 %


def rolled(k=K, n=A_N, which="A", n_iv=len(A_RULES)):
    """(params int64 [k, 6 + 4 R, n], arrays uint8 [k, n_iv], soc0 int64 [k, n]): the recipe (tiled to n chains past
    A_N) rolled by v * ROLL chains, the array rolled by v intervals."""
    par, soc0 = recipe(A_N, which) if n == A_N else tiled(n, which)
    base = A_RULES if which == "A" else c_rules(n_iv)
    assert len(base) == n_iv
    p = np.stack([np.roll(par, v * ROLL, axis=1) for v in range(k)]).astype(np.int64)
    s = np.stack([np.roll(soc0, v * ROLL) for v in range(k)]).astype(np.int64)
    a = np.stack([np.roll(base, v) for v in range(k)]).astype(np.uint8)
    return np.ascontiguousarray(p), np.ascontiguousarray(a), np.ascontiguousarray(s)


def tariff_arrays():
    """The tariffs set's five arrays, uint8 [K, 13]."""
    return np.ascontiguousarray(np.stack([A_RULES, np.zeros_like(A_RULES), np.roll(A_RULES, 1), np.full_like(A_RULES, 2),
                                          A_RULES[::-1]]).astype(np.uint8))


def tariffs(n=A_N):
    """(params int64 [K, 6 + 4 R, n], arrays uint8 [K, 13], soc0 int64 [K, n]): the recipe's households under each of
    tariff_arrays()."""
    par, soc0 = recipe(A_N) if n == A_N else tiled(n, "A")
    return (np.ascontiguousarray(np.stack([par] * K).astype(np.int64)), tariff_arrays(),
            np.ascontiguousarray(np.stack([soc0] * K).astype(np.int64)))


def pair_shares(table, live, cols):
    """For every pair of variants (u < v), the share of the live chains whose run totals differ between the two in
    any of the columns `cols`: {(u, v): share}.  table: [K, n_intervals, 13, n]."""
    tot = table[:, :, list(cols)].sum(axis=1)                              # [K, len(cols), n]
    return {(u, v): float((tot[u][:, live] != tot[v][:, live]).any(axis=0).mean())
            for u in range(tot.shape[0]) for v in range(u + 1, tot.shape[0])}


def limit_params(params, rules):
    """dispatch_util.identities' argument for one variant: the limit in force per interval in row 8."""
    lim = np.asarray(params)[8 + 4 * np.asarray(rules, dtype=np.int64)]
    fake = np.zeros((9,) + lim.shape, dtype=np.int64)
    fake[8] = lim
    return fake
