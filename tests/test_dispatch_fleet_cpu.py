"""The dispatch fleet series without a GPU: the contract in numpy (dispatch.fleet_from_traces and
schedule.fleet_from_traces, plain loops over the seconds) on the oracle's 60-module traces of base input A
(storage_util.a60_oracle, the GPU tests' input) with the dispatch and the schedule tests' households
(dispatch_util.recipe, schedule_util.recipe and A_RULES): against the fleet series, against the kinds' tables
summed over the chains (dispatch.from_traces; schedule_util.run, written apart from schedule.py), against a
per-chain loop over Python integers, the row identities, the reductions to the battery fleet series and of the
schedule to dispatch, the teeth of the input, fleet_to_watts and fleet_peaks, and the C-ABI's setter.  Integers:
every comparison is bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import dispatch_util
import schedule_util
from series_util import A_N, A_STEPS
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, battery, dispatch, schedule, series

D_PARAMS, D_SOC0 = dispatch_util.recipe()
S_PARAMS, S_SOC0 = schedule_util.recipe()
A_RULES = schedule_util.A_RULES
IV, GC = 900, 512
# fleet column -> table column (the sums both hold)
TABLE_COL = {0: 0, 1: 1, 2: 2, 3: 3, 4: 4, 5: 5, 7: 6, 8: 10}
# the teeth, counted on the oracle's traces (seconds of the one-group series); the tests assert half or more
OBSERVED = dict(curtails=4027, export_differs=5012, grid_buy_breaks_bound=2071)


@functools.lru_cache(maxsize=None)
def traces():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@functools.lru_cache(maxsize=None)
def d_fleet():
    pv, meter, cov, _ = traces()
    raw, end = dispatch.fleet_from_traces(pv, meter, cov, params=D_PARAMS, soc0=D_SOC0, group_chains=GC)
    raw.setflags(write=False)
    return raw, end


@functools.lru_cache(maxsize=None)
def s_fleet():
    pv, meter, cov, _ = traces()
    raw, end = schedule.fleet_from_traces(pv, meter, cov, IV, params=S_PARAMS, rule_of_interval=A_RULES, soc0=S_SOC0,
                                          group_chains=GC)
    raw.setflags(write=False)
    return raw, end


def _sum_b(r):
    """The fleet's net battery power of rows [..., 9], from the row identity."""
    return r[..., 4] - r[..., 5] - r[..., 8] - (r[..., 1] - r[..., 0])


def _groups(a):
    """[..., n] summed over the chains of each group: [2, ...]."""
    return np.stack([a[..., :GC].sum(axis=-1), a[..., GC:].sum(axis=-1)])


def test_columns_header_and_export():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_DISPATCH_FLEET_COLS 9" in hdr and len(dispatch.FLEET_COLUMNS) == 9
    assert "#define TMH_OUT_DISPATCH_FLEET 14" in hdr and "#define TMH_OUT_SCHEDULE_FLEET 15" in hdr
    assert _lib.OUT_DISPATCH_FLEET == 14 and _lib.OUT_SCHEDULE_FLEET == 15 == _lib.OUT_SITES - 1
    assert "#define TMH_ABI_VERSION 1" in hdr and "tmh_set_dispatch_fleet" in _lib.EXPORTS
    assert "int tmh_set_dispatch_fleet(struct tmh_engine* eng, const tmh_series* fleet);" in hdr
    assert dispatch.FLEET_COLUMNS == battery.FLEET_COLUMNS + ("curtailed",)


@pytest.mark.parametrize("kind", ["dispatch", "schedule"])
def test_first_four_columns_are_the_fleet_series(kind):
    pv, meter, cov, _ = traces()
    raw, _ = d_fleet() if kind == "dispatch" else s_fleet()
    assert raw.shape == (2, A_STEPS, 9) and raw.dtype == np.int64
    np.testing.assert_array_equal(raw[..., :4], series.from_traces(pv, meter, cov, GC))
    assert raw[0, :, 2].max() > 450 and raw[1, :, 3].max() > 0


def test_interval_sums_are_the_dispatch_table():
    """Summed over each metering interval's seconds, the rows are dispatch.from_traces summed over each group's
    chains; the end state is its."""
    pv, meter, cov, _ = traces()
    raw, end = d_fleet()
    table, tend = dispatch.from_traces(pv, meter, cov, IV, params=D_PARAMS, soc0=D_SOC0)
    np.testing.assert_array_equal(end, tend)
    for k in range(table.shape[0]):
        rows = raw[:, k * IV:(k + 1) * IV].sum(axis=1)
        for col, tcol in TABLE_COL.items():
            np.testing.assert_array_equal(rows[:, col], _groups(table[k, tcol]), err_msg=f"interval {k} column {col}")
        np.testing.assert_array_equal(_sum_b(rows), _groups(table[k, 6] - table[k, 7]))
    assert all(int(raw[..., c].sum()) > 0 for c in range(9))


def test_interval_sums_are_the_schedule_table():
    """The same against schedule_util.run, the schedule's contract written apart from schedule.py."""
    pv, meter, cov, _ = traces()
    raw, end = s_fleet()
    table, tend, _ = schedule_util.run(pv, meter, cov, IV, S_PARAMS, A_RULES, S_SOC0)
    np.testing.assert_array_equal(end, tend)
    for k in range(table.shape[0]):
        rows = raw[:, k * IV:(k + 1) * IV].sum(axis=1)
        for col, tcol in TABLE_COL.items():
            np.testing.assert_array_equal(rows[:, col], _groups(table[k, tcol]), err_msg=f"interval {k} column {col}")
        np.testing.assert_array_equal(_sum_b(rows), _groups(table[k, 6] - table[k, 7]))
    assert all(int(raw[..., c].sum()) > 0 for c in range(9))


def _loop_apart(pv, meter, cv, params, x0, rule_at):
    """All nine columns of traces [steps, m] by a per-chain loop over Python integers; params' rows 0-5 the battery,
    rule_at(t, i) -> (Tc, Td, L, G) of chain i at second t.  Returns ([steps, 9], end states)."""
    steps, m = pv.shape
    want, ends = np.zeros((steps, 9), dtype=np.int64), []
    for i in range(m):
        cap, pc, pd, ec, ed, sb = (int(v) for v in params[:6, i])
        kc, kd = -(-(1 << 32) // ec), -(-(1 << 32) // ed)
        x = min(max(int(x0[i]), 0), cap)
        for t in range(steps):
            if np.isnan(pv[t, i]) or np.isnan(meter[t, i]) or cv[t, i] == 255:
                continue
            tc, td, lim, grid = rule_at(t, i)
            qp, qm = round(float(pv[t, i]) * 4096), round(float(meter[t, i]) * 4096)
            d = qp - qm
            a = min(max(d - tc, 0), pc) if d >= 0 else -min(max(-d - td, 0), pd)
            if grid:
                a = min(max(a, 0) + grid, pc)
            s = (a * ec) >> 16 if a >= 0 else -((-a * kd + 65535) >> 16)
            x1 = min(max(x + s, 0), cap)
            g = x1 - x
            b = a if g == s else min(a, (g * kc + 65535) >> 16) if g > 0 else -min(-a, (-g * ed) >> 16) if g < 0 else 0
            x = max(x1 - sb, 0)
            r = d - b
            fed = min(max(r, 0), lim)
            want[t] += (qp, qm, 1, int(cv[t, i] == 1), max(-r, 0), fed, x, max(b, 0), max(r, 0) - fed)
        ends.append(x)
    return want, np.array(ends, dtype=np.int64)


@pytest.mark.parametrize("kind", ["dispatch", "schedule"])
def test_a_loop_written_apart(kind):
    """All nine columns, second by second, of a slice of chains (dead at construction, faulting inside the window,
    every feed-in limit) after sunrise and, for the schedule, across the rule changes at steps 6,300 and 7,200."""
    pv, meter, cov, status = traces()
    par = D_PARAMS if kind == "dispatch" else S_PARAMS
    dead = np.flatnonzero(status == 1)[:2]
    faulted = np.flatnonzero((cov[-1] == 255) & (cov[0] != 255))
    live = np.flatnonzero(cov[-1] != 255)
    lo, hi = 6200, 7300                                   # after sunrise; the first in-window fault is at 6429
    # chains that must curtail in the window: without a battery (C = 0), a surplus above the limit in force
    _, d = battery._ok_d(pv[lo:hi], meter[lo:hi], cov[lo:hi])
    lim = D_PARAMS[8][None] if kind == "dispatch" else schedule_util.limits(S_PARAMS, A_RULES)[np.arange(lo, hi) // IV]
    cut = np.flatnonzero((par[0] == 0) & (d > lim + 1).any(axis=0))[:3]
    assert len(cut) == 3
    chains = np.unique(np.r_[dead, faulted, cut, np.concatenate([live[D_PARAMS[8, live] == v][:2] for v in np.unique(D_PARAMS[8])])])
    assert len(chains) >= 12
    p, m, cv = (a[lo:hi, chains] for a in (pv, meter, cov))
    x0 = np.arange(len(chains), dtype=np.int64) * 100000  # (clamped into [0, C])
    if kind == "dispatch":
        got, end = dispatch.fleet_from_traces(p, m, cv, params=par[:, chains], soc0=x0)
        rule_at = lambda t, i: tuple(int(v) for v in par[6:9, chains[i]]) + (0,)
    else:
        got, end = schedule.fleet_from_traces(p, m, cv, IV, params=par[:, chains], rule_of_interval=A_RULES[:-(-hi // IV)],
                                              soc0=x0, origin=lo)
        rule_at = lambda t, i: tuple(int(v) for v in par[6 + 4 * int(A_RULES[(lo + t) // IV]):, chains[i]][:4])
        assert A_RULES[lo // IV] != A_RULES[(hi - 1) // IV]
    want, ends = _loop_apart(p, m, cv, par[:, chains], x0, rule_at)
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(end, ends)
    assert want[:, 2].min() < want[:, 2].max() == len(chains) - len(dead)
    assert (want[:, 4:] > 0).any(axis=0).all()


@pytest.mark.parametrize("kind", ["dispatch", "schedule"])
def test_row_identities(kind):
    pv, meter, cov, _ = traces()
    raw, _ = d_fleet() if kind == "dispatch" else s_fleet()
    par = D_PARAMS if kind == "dispatch" else S_PARAMS
    assert (raw[..., 4:] >= 0).all() and (raw[..., 2] >= raw[..., 3]).all()
    assert (raw[..., 6] <= _groups(par[0])[:, None]).all()
    sb = _sum_b(raw)
    assert (raw[..., 7] - sb >= 0).all()                                    # the discharging power
    ok, d = battery._ok_d(pv, meter, cov)
    np.testing.assert_array_equal(raw[..., 4] - raw[..., 5] - raw[..., 8], _groups(np.where(ok, -d, 0)) + sb)
    assert (raw[..., 5] + raw[..., 8] <= _groups(np.where(ok, np.maximum(d, 0), 0))).all()   # fed in + curtailed: of the surplus


def test_one_limit_bounds_the_feed_in():
    """Every chain under the same limit L: [5] <= n_ok * L on the oracle's traces; on hand-made ones (every chain
    1,000 W of PV against 100 W, no battery, one chain not ok) the bound is met: [5] == n_ok * L, the rest curtailed."""
    pv, meter, cov, _ = traces()
    lim = 20 << 12
    par = D_PARAMS.copy()
    par[8] = lim
    raw, _ = dispatch.fleet_from_traces(pv[9500:10800], meter[9500:10800], cov[9500:10800], params=par, soc0=D_SOC0, group_chains=GC)
    assert (raw[..., 5] <= raw[..., 2] * lim).all() and int(raw[..., 5].sum()) > 0 and int(raw[..., 8].sum()) > 0
    n, lim = 40, 300 << 12
    hp, hm, hc = np.full((10, n), 1000.0), np.full((10, n), 100.0), np.zeros((10, n), dtype=np.uint8)
    hp[4:, 7], hc[4:, 7] = np.nan, 255
    par = np.zeros((9, n), dtype=np.int64)
    par[3:5], par[8] = 1 << 16, lim
    raw, end = dispatch.fleet_from_traces(hp, hm, hc, params=par, soc0=0)
    np.testing.assert_array_equal(raw[0, :, 2], [n] * 4 + [n - 1] * 6)
    np.testing.assert_array_equal(raw[0, :, 5], raw[0, :, 2] * lim)
    np.testing.assert_array_equal(raw[0, :, 8], raw[0, :, 2] * (600 << 12))
    assert not raw[0, :, [4, 6, 7]].any() and not end.any()


def test_greedy_rule_gives_the_battery_fleet_series():
    """Tc = Td = 0 and L = 2^27: columns 0-7 are battery.fleet_from_traces' and column 8 is 0."""
    pv, meter, cov, _ = traces()
    par = D_PARAMS.copy()
    par[6:8] = 0
    par[8] = 1 << 27
    raw, end = dispatch.fleet_from_traces(pv, meter, cov, params=par, soc0=D_SOC0, group_chains=GC)
    want, wend = battery.fleet_from_traces(pv, meter, cov, params=par[:6], soc0=D_SOC0, group_chains=GC)
    np.testing.assert_array_equal(raw[..., :8], want)
    np.testing.assert_array_equal(end, wend)
    assert not raw[..., 8].any()


@pytest.mark.parametrize("case", ["one_rule", "equal_rules", "one_rule_throughout"])
def test_schedule_reduces_to_dispatch(case):
    """R = 1, R = 4 with equal rules, and an array naming rule 0 throughout: the dispatch fleet of rule 0."""
    pv, meter, cov, _ = (a[5400:7300] if a.ndim == 2 else a for a in traces())
    n_iv = -(-(5400 + 1900) // IV)
    rules0 = np.zeros(n_iv, np.uint8)
    par, rules = {"one_rule": (S_PARAMS[:10], rules0),
                  "equal_rules": (np.vstack([S_PARAMS[:6]] + [S_PARAMS[6:10]] * schedule_util.R), A_RULES[:n_iv]),
                  "one_rule_throughout": (S_PARAMS, rules0)}[case]
    got, end = schedule.fleet_from_traces(pv, meter, cov, IV, params=par, rule_of_interval=rules, soc0=S_SOC0, origin=5400,
                                          group_chains=GC)
    want, wend = dispatch.fleet_from_traces(pv, meter, cov, params=schedule.to_dispatch_params(S_PARAMS, 0), soc0=S_SOC0,
                                            group_chains=GC)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(end, wend)
    assert int(want[..., 8].sum()) > 0 and int(want[..., 7].sum()) > 0


def test_the_input_bites():
    """Conditions on the GPU tests' input, asserted of the references at half of what the oracle's traces give
    (OBSERVED): seconds at which the fleet curtails; seconds at which column 5 differs from the battery fleet
    series' export of the same batteries (the limit and the thresholds at work); and, under the schedule, seconds
    with grid buying at which [4] <= [1] + |[0]| -- the battery fleet's bound on the import -- fails, so a
    reference without the bought term could not pass."""
    pv, meter, cov, _ = traces()
    d, s = d_fleet()[0].sum(axis=0), s_fleet()[0].sum(axis=0)
    b = battery.fleet_from_traces(pv, meter, cov, params=D_PARAMS[:6], soc0=D_SOC0)[0][0]
    seen = dict(curtails=int((d[:, 8] > 0).sum()), export_differs=int((d[:, 5] != b[:, 5]).sum()),
                grid_buy_breaks_bound=int((s[:, 4] > s[:, 1] + np.abs(s[:, 0])).sum()))
    print(seen)
    for name, count in OBSERVED.items():
        assert 2 * seen[name] >= count, (name, seen[name], count)
    assert (d[:, 4] <= d[:, 1] + np.abs(d[:, 0])).all()                     # (plain dispatch keeps the bound)


def test_fleet_to_watts_and_peaks_by_hand():
    """A hand-made table of 7 seconds in bins of 3 (a partial last bin of one second)."""
    s = 4096
    rows = np.array([  # pv, meter, n_ok, cov, import, export, soc, charge, curtailed
        [10, 4, 2, 1, 1, 3, 7200, 5, 1],
        [12, 4, 2, 0, 0, 5, 3600, 4, 2],
        [8, 6, 2, 2, 2, 3, 0, 1, 0],
        [0, 9, 1, 0, 9, 0, 3600, 0, 0],
        [0, 0, 0, 0, 0, 0, 0, 0, 0],
        [2, 9, 1, 1, 9, 1, 0, 2, 1],
        [6, 2, 2, 0, 0, 4, 7200, 0, 0]], dtype=np.int64) * s
    rows[:, 2:4] //= s
    raw = rows[None]
    w = dispatch.fleet_to_watts(raw)
    assert set(w) == {"pv", "meter", "import_w", "export_w", "charge_w", "discharge_w", "curtailed_w", "soc_wh", "n_ok", "covered"}
    np.testing.assert_array_equal(w["curtailed_w"][0], [1, 2, 0, 0, np.nan, 1, 0])
    np.testing.assert_array_equal(w["export_w"][0], [3, 5, 3, 0, np.nan, 1, 4])
    # sum of b = import - export - curtailed - (meter - pv): 3, 1, 1, 0, -, 0, 0; discharge = charge - that
    np.testing.assert_array_equal(w["discharge_w"][0], [2, 3, 0, 0, np.nan, 2, 0])
    np.testing.assert_array_equal(w["soc_wh"][0], [2, 1, 0, 1, np.nan, 0, 2])
    w3 = dispatch.fleet_to_watts(raw, bin_s=3)
    assert all(v.shape == (1, 3) for v in w3.values())
    np.testing.assert_array_equal(w3["import_w"][0], [3, 18, 0])
    np.testing.assert_array_equal(w3["curtailed_w"][0], [3, 1, 0])
    np.testing.assert_array_equal(w3["n_ok"][0], [6, 2, 2])
    np.testing.assert_array_equal(w3["covered"][0], [3 / 6, 1 / 2, 0])
    np.testing.assert_array_equal(w3["soc_wh"][0], [1, 1 / 3, 2])              # the bin's mean: the last bin has one second
    m3 = dispatch.fleet_to_watts(raw, bin_s=3, mean=True)
    np.testing.assert_array_equal(m3["export_w"][0], [11 / 6, 1 / 2, 2])
    np.testing.assert_array_equal(m3["soc_wh"][0], [3 / 6, 1 / 2, 1])
    pk = dispatch.fleet_peaks(raw, 3)
    assert set(pk) == {"peak_w_import", "t_peak_import", "peak_w_export", "t_peak_export"}
    np.testing.assert_array_equal(pk["peak_w_import"][0], [2, 9, 0])
    np.testing.assert_array_equal(pk["t_peak_import"][0], [2, 0, 0])           # (the earliest second at the peak)
    np.testing.assert_array_equal(pk["peak_w_export"][0], [5, 1, 4])
    np.testing.assert_array_equal(pk["t_peak_export"][0], [1, 2, 0])
    pk1 = dispatch.fleet_peaks(raw, 1)
    np.testing.assert_array_equal(pk1["peak_w_import"][0], rows[:, 4] / s)
    assert not pk1["t_peak_export"].any() and pk["t_peak_import"].dtype == np.int64
    empty = dispatch.fleet_to_watts(np.zeros((1, 5, 9), dtype=np.int64))
    assert np.isnan(empty["curtailed_w"]).all() and (empty["n_ok"] == 0).all()
    for fn in (dispatch.fleet_to_watts, lambda r, **kw: dispatch.fleet_peaks(r, kw.get("bin_s", 1))):
        for bad in (raw[..., :8], raw[0, 0]):
            with pytest.raises(ValueError):
                fn(bad)
        with pytest.raises(ValueError):
            fn(raw, bin_s=0)


def test_peaks_are_not_the_chains_peaks():
    """What the series exists for: over each metering interval the fleet's coincident peak import is below the sum of
    the chains' own peaks (table column 11), and fleet_peaks finds the second."""
    pv, meter, cov, _ = traces()
    raw, _ = d_fleet()
    one = raw.sum(axis=0, keepdims=True)
    pk = dispatch.fleet_peaks(one, IV)
    table, _ = dispatch.from_traces(pv, meter, cov, IV, params=D_PARAMS, soc0=D_SOC0)
    own = (table[:, 11] >> 32).sum(axis=1) / 4096.0
    assert pk["peak_w_import"].shape == (1, 13) and (pk["peak_w_import"][0] < own).all()
    for k in (0, 7, 12):
        t = int(pk["t_peak_import"][0, k])
        assert one[0, k * IV + t, 4] == one[0, k * IV:(k + 1) * IV, 4].max() and (one[0, k * IV:k * IV + t, 4] < one[0, k * IV + t, 4]).all()


def test_bad_shapes():
    pv, meter, cov, _ = traces()
    pv, meter, cov = pv[:50, :20], meter[:50, :20], cov[:50, :20]
    dpar, spar = D_PARAMS[:, :20], S_PARAMS[:, :20]
    dispatch.fleet_from_traces(pv, meter, cov, params=dpar, soc0=0)
    for kw in (dict(params=dpar[:, :19], soc0=0), dict(params=dpar[:6], soc0=0), dict(params=dpar, soc0=0, group_chains=100)):
        with pytest.raises(ValueError):
            dispatch.fleet_from_traces(pv, meter, cov, **kw)
    rules = np.zeros(1, np.uint8)
    schedule.fleet_from_traces(pv, meter, cov, IV, params=spar, rule_of_interval=rules, soc0=0)
    for kw in (dict(params=spar[:, :19], rule_of_interval=rules), dict(params=spar, rule_of_interval=np.zeros(2, np.uint8)),
               dict(params=spar, rule_of_interval=rules + 4), dict(params=spar, rule_of_interval=rules, group_chains=100)):
        with pytest.raises(ValueError):
            schedule.fleet_from_traces(pv, meter, cov, IV, soc0=0, **kw)
    with pytest.raises(ValueError):
        schedule.fleet_from_traces(pv, meter, cov, 0, params=spar, rule_of_interval=rules, soc0=0)


def test_abi_setter_refusals():
    """Host-side only: what tmh_set_dispatch_fleet refuses before it touches an engine (an fp32 engine's refusal
    needs an engine, so a device: tests/test_gpu_dispatch_fleet.py)."""
    L = _lib.load()
    assert L.tmh_abi_version() == 1 and C.sizeof(_lib.Series) == 32             # tmh_series as it was
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data

    def refused(word, *args):
        assert L.tmh_set_dispatch_fleet(None, C.byref(_lib.Series(*args))) == -1
        msg = L.tmh_last_error().decode()
        assert "dispatch fleet series" in msg and word in msg, msg

    refused("buffer", None, 0, 8, 0, 1, 0)
    refused("n_steps", p, 0, 0, 0, 1, 0)
    refused("n_groups", p, 0, 8, 0, 0, 0)
    refused("8-byte aligned", p + 4, 0, 8, 0, 1, 0)
    refused("multiple of 512", p, 0, 8, 100, 1, 0)
    refused("multiple of 512", p, 0, 8, 0, 2, 0)
    assert L.tmh_set_dispatch_fleet(None, C.byref(_lib.Series(p, 0, 8, 0, 1, 0))) == -1
    assert b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_dispatch_fleet(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    assert not buf.any()
