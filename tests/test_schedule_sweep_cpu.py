"""The schedule sweep without a GPU: schedule.sweep_from_traces (one pass over the seconds with the state [K, n])
against K calls of schedule.from_traces and against schedule_util's sequential run, on the oracle's traces of base
input A with a 60-module system and schedule_sweep_util's two sets of five variants; the shares by which the
variants differ; the cells' identities under each variant's limit in force; the reductions (rule 0 throughout is
the dispatch kind, hold throughout moves no battery energy); the summary and the energy cost against sums by
hand; the quantisation and the checks of the parameters and of the arrays; the C-ABI's struct, codes and setter."""
import ctypes as C
import os

import numpy as np
import pytest

from dispatch_util import identities, soc_changes
from schedule_sweep_util import (K, MIN_ROLLED_SHARE, MIN_TARIFFS_SHARE, MIN_TARIFFS_SHARE4, limit_params, pair_shares, rolled,
                                 tariff_arrays, tariffs)
from schedule_util import A_RULES, NO_LIMIT, R, W, recipe, run
from series_util import A_N
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, dispatch, schedule

IV = 900
SETS = {"rolled": rolled(), "tariffs": tariffs()}


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@pytest.fixture(scope="module")
def tables():
    """{set: (table [K, 13, 13, n], end [K, n])} by sweep_from_traces."""
    pv, meter, cov, _ = _a()
    return {name: schedule.sweep_from_traces(pv, meter, cov, IV, params=p, rule_of_interval=a, soc0=s)
            for name, (p, a, s) in SETS.items()}


@pytest.mark.parametrize("name", ["rolled", "tariffs"])
def test_sweep_from_traces_equals_the_schedule_per_variant(tables, name):
    """Thirteen columns and the end state of every variant: from_traces of the variant's slice, and schedule_util's
    run, a third derivation; variant 0 of the rolled set is the schedule tests' own input."""
    pv, meter, cov, status = _a()
    par, arr, soc0 = SETS[name]
    got, end = tables[name]
    assert got.shape == (K, 13, 13, A_N) and end.shape == (K, A_N) and got.dtype == end.dtype == np.int64
    dead = status == 1
    assert dead.any()
    for v in range(K):
        want, wend = schedule.from_traces(pv, meter, cov, IV, params=par[v], rule_of_interval=arr[v], soc0=soc0[v])
        other, oend, _ = run(pv, meter, cov, IV, par[v], arr[v], soc0[v])
        for col in range(13):
            np.testing.assert_array_equal(got[v, :, col], want[:, col], err_msg=f"variant {v} column {col}")
            np.testing.assert_array_equal(got[v, :, col], other[:, col], err_msg=f"variant {v} column {col} (run)")
        np.testing.assert_array_equal(end[v], wend)
        np.testing.assert_array_equal(end[v], oend)
        assert not got[v][:, :, dead].any() and (end[v][dead] == soc0[v][dead]).all()
        identities(got[v], limit_params(par[v], arr[v]))
        soc_changes(got[v], soc0[v], end[v])
        np.testing.assert_array_equal(got[v, :, :4], got[0, :, :4])
    if name == "rolled":
        p0, s0 = recipe()
        np.testing.assert_array_equal(par[0], p0)
        np.testing.assert_array_equal(arr[0], A_RULES)
        np.testing.assert_array_equal(soc0[0], s0)


def test_the_variants_differ(tables):
    """Every pair of variants differs for most live chains (floors: conditions on the inputs)."""
    status = _a()[3]
    live = status == 0
    print("live after the run", int(live.sum()), "alive at construction", int((status != 1).sum()))
    assert int(live.sum()) > 900
    r4 = pair_shares(tables["rolled"][0], live, (4,))
    t4 = pair_shares(tables["tariffs"][0], live, (4,))
    t = pair_shares(tables["tariffs"][0], live, (4, 5, 10))
    print("rolled column 4", min(r4.values()), max(r4.values()), "tariffs column 4", min(t4.values()), max(t4.values()),
          "tariffs columns 4, 5, 10", min(t.values()), max(t.values()))
    assert min(r4.values()) >= MIN_ROLLED_SHARE
    assert min(t4.values()) >= MIN_TARIFFS_SHARE4
    assert min(t.values()) >= MIN_TARIFFS_SHARE


def test_tariffs_reduce_to_dispatch_and_to_hold(tables):
    """Rule 0 throughout (variant 1) is dispatch.from_traces under rule 0; hold throughout (variant 3) moves no
    battery energy: columns 6 and 7 are zero."""
    pv, meter, cov, _ = _a()
    par, arr, soc0 = SETS["tariffs"]
    got, end = tables["tariffs"]
    assert not arr[1].any() and (arr[3] == 2).all()
    want, wend = dispatch.from_traces(pv, meter, cov, IV, params=schedule.to_dispatch_params(par[1], 0), soc0=soc0[1])
    np.testing.assert_array_equal(got[1], want)
    np.testing.assert_array_equal(end[1], wend)
    assert not got[3, :, 6].any() and not got[3, :, 7].any()
    assert int(got[0, :, 6].sum()) > 0 and int(got[0, :, 7].sum()) > 0


def test_sweep_summary_and_energy_cost_by_hand(tables):
    par, arr, soc0 = SETS["rolled"]
    raw, _ = tables["rolled"]
    s = schedule.sweep_summary(raw, IV, par)
    e = float(1 << 12) * 3600.0
    want = dispatch.sweep_summary(raw, IV, np.concatenate([par[:, :6], np.zeros((K, 3, A_N), np.int64)], axis=1))
    assert set(s) == set(want)
    for key in want:
        np.testing.assert_array_equal(s[key], want[key], err_msg=key)
        assert s[key].shape == (K, A_N)
    np.testing.assert_array_equal(s["energy_wh_curtailed"], raw[:, :, 10].sum(axis=1) / e)
    np.testing.assert_array_equal(s["peak_w_export"], (raw[:, :, 12] >> 32).max(axis=1) / 4096.0)
    f = schedule.sweep_summary(raw, IV, par, fleet=True)
    np.testing.assert_array_equal(f["energy_wh_curtailed"], raw[:, :, 10].sum(axis=(1, 2)) / e)
    # the energy cost: sum over the intervals of price * import - feed-in price * export, in currency per kWh
    imp, exp = raw[:, :, 4].astype(np.float64) / (e * 1000.0), raw[:, :, 5].astype(np.float64) / (e * 1000.0)
    c = schedule.energy_cost(raw, 0.30, 0.08)
    assert c.shape == (K, A_N) and c.dtype == np.float64
    np.testing.assert_allclose(c, 0.30 * imp.sum(axis=1) - 0.08 * exp.sum(axis=1), rtol=1e-12, atol=1e-15)
    tou = np.where(A_RULES == 1, 0.20, 0.35)
    np.testing.assert_allclose(schedule.energy_cost(raw, tou, 0.08), (tou[None, :, None] * imp).sum(axis=1) - 0.08 * exp.sum(axis=1),
                               rtol=1e-12, atol=1e-15)
    per = np.where(arr == 1, 0.20, 0.35)
    np.testing.assert_allclose(schedule.energy_cost(raw, per, 0.0), (per[:, :, None] * imp).sum(axis=1), rtol=1e-12, atol=1e-15)
    one = schedule.energy_cost(raw[2], tou, 0.08)
    assert one.shape == (A_N,)
    np.testing.assert_array_equal(one, schedule.energy_cost(raw, tou, 0.08)[2])
    assert (c[:, _a()[3] == 0] > 0).any()
    for bad in (np.zeros(12), np.zeros((K + 1, 13)), np.zeros((K, 13, 1))):
        with pytest.raises(ValueError, match="import_price"):
            schedule.energy_cost(raw, bad, 0.0)
    with pytest.raises(ValueError, match="feed_in_price"):
        schedule.energy_cost(raw, 0.3, [0.1, 0.2])
    with pytest.raises(ValueError, match="raw table"):
        schedule.energy_cost(raw[:, :, :10], 0.3, 0.1)


def test_quantisation_of_scalars_lists_and_arrays():
    n = 6
    rules = [dict(charge_above_w=[0.0, 100.0, 200.0], feed_in_limit_w=[None, 500.0, None]),
             dict(discharge_above_w=250.0, feed_in_limit_w=None, grid_charge_w=np.arange(3 * n, dtype=np.float64).reshape(3, n))]
    p = schedule.quantize_sweep_params([5000.0, 2500.0, 0.0], 2500.0, np.full((3, n), 2000.0), 0.95, [0.9, 1.0, 0.95], 2.0,
                                       rules=rules, n=n)
    assert p.shape == (3, 14, n) and p.dtype == np.int64
    for v in range(3):
        one = schedule.quantize_params([5000.0, 2500.0, 0.0][v], 2500.0, 2000.0, 0.95, [0.9, 1.0, 0.95][v], 2.0, n=n,
                                       rules=[dict(charge_above_w=[0.0, 100.0, 200.0][v], feed_in_limit_w=[None, 500.0, None][v]),
                                              dict(discharge_above_w=250.0, grid_charge_w=np.arange(3 * n, dtype=np.float64)[v * n:(v + 1) * n])])
        np.testing.assert_array_equal(p[v], one)
    assert (p[0, 8] == NO_LIMIT).all() and (p[1, 8] == 500 * W).all() and (p[:, 12] == NO_LIMIT).all()
    assert p[2, 13].tolist() == [(2 * n + i) * W for i in range(n)]
    schedule.check_sweep_params(p, n_rules=2)
    soc = schedule.quantize_sweep_soc([100.0, 0.0, 0.0], p)
    assert soc.shape == (3, n) and (soc[0] == 100 * 3600 * W).all() and not soc[1:].any()
    assert schedule.quantize_sweep_params(1.0, 1.0, 1.0, rules=[{}], n=2, n_variants=4).shape == (4, 10, 2)
    for bad in (dict(capacity_wh=[1.0, 2.0]), dict(n_variants=2), dict(n_variants=17), dict(charge_eff=0.4),
                dict(rules=[dict(charge_above_w=[0.0, 1.0])]), dict(rules=[dict(grid_charge_w=-1.0)]), dict(rules=[]),
                dict(rules=[{}] * 9), dict(rules=[dict(charge_w=1.0)]), dict(rules=[dict(feed_in_limit_w=[None, -1.0, None])]),
                dict(standby_w=np.zeros((3, n + 1))), dict(charge_w=np.zeros((1, 1, 1)))):
        kw = dict(capacity_wh=[5000.0, 2500.0, 0.0], charge_w=2500.0, discharge_w=2000.0, rules=rules, n=n)
        kw.update(bad)
        with pytest.raises(ValueError):
            schedule.quantize_sweep_params(**kw)
    with pytest.raises(ValueError):
        schedule.quantize_sweep_soc(6000.0, p)


def test_check_sweep_params_and_rules():
    par, arr, _ = SETS["rolled"]
    assert schedule.check_sweep_params(par, n_rules=R) is par
    rows = (("capacity", 0, 1 << 40), ("p_charge", 1, (1 << 27) + 1), ("p_discharge", 2, (1 << 27) + 1),
            ("eff_charge", 3, (1 << 16) + 1), ("eff_discharge", 4, (1 << 16) + 1), ("standby", 5, (1 << 27) + 1))
    rows += tuple((f"rule {r} {name}", 6 + 4 * r + j, (1 << 27) + 1) for r in range(R) for j, name in enumerate(schedule.RULE_PARAMS))
    for name, row, above in rows:
        for value in (above, (1 << 15) - 1 if row in (3, 4) else -1):
            bad = par.copy()
            bad[3, row, 17] = value
            with pytest.raises(ValueError, match=name):
                schedule.check_sweep_params(bad)
    for bad in (par[:, :21], par[:, :6], par[0], par.astype(np.int32), np.concatenate([par] * 4)[:17]):
        with pytest.raises(ValueError):
            schedule.check_sweep_params(bad)
    with pytest.raises(ValueError, match="rules"):
        schedule.check_sweep_params(par, n_rules=3)
    got = schedule.check_sweep_rules(arr, R, 13, K)
    np.testing.assert_array_equal(got, arr)
    one = schedule.check_sweep_rules(A_RULES, R, 13, K)                    # [n_intervals]: every variant's
    assert one.shape == (K, 13) and one.flags.c_contiguous and one.dtype == np.uint8
    np.testing.assert_array_equal(one, np.stack([A_RULES] * K))
    for bad, word in ((arr[:4], "variants"), (arr[:, :12], "intervals"), (arr.astype(np.int64), "uint8"),
                      (arr[None], "uint8"), (A_RULES[:12], "intervals")):
        with pytest.raises(ValueError, match=word):
            schedule.check_sweep_rules(bad, R, 13, K)
    worse = arr.copy()
    worse[4, 7] = R
    with pytest.raises(ValueError, match=f"rule {R} of {R}"):
        schedule.check_sweep_rules(worse, R, 13, K)
    assert tariff_arrays().shape == (K, 13) and tariff_arrays()[4].tolist() == A_RULES[::-1].tolist()


def test_header_struct_codes_and_setter():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_SCHEDULE_SWEEP_MAX 16" in hdr and schedule.SWEEP_MAX == _lib.SCHEDULE_SWEEP_MAX == 16
    assert "#define TMH_OUT_SCHEDULE_SWEEP 64" in hdr and _lib.OUT_SCHEDULE_SWEEP == 64
    assert "#define TMH_ABI_VERSION 1" in hdr and "int tmh_set_schedule_sweep(" in hdr
    assert "tmh_set_schedule_sweep" in _lib.EXPORTS
    # every older code keeps its value; the new one lies above both flags and is no combination of them
    old = dict(OUT_ANY=0, OUT_TRACE3=1, OUT_STATS=2, OUT_SERIES=3, OUT_INTERVALS=4, OUT_REGISTERS=5, OUT_DEMAND=6, OUT_STORAGE=7,
               OUT_BATTERY=8, OUT_BATTERY_FLEET=9, OUT_BATTERY_SWEEP=10, OUT_DISPATCH=11, OUT_DISPATCH_SWEEP=12, OUT_SCHEDULE=13,
               OUT_DISPATCH_FLEET=14, OUT_SCHEDULE_FLEET=15, OUT_SITES=16, OUT_FP64=32)
    for name, value in old.items():
        assert getattr(_lib, name) == value and f"#define TMH_{name} {value}\n" in hdr, name
    assert _lib.OUT_SCHEDULE_SWEEP > (_lib.OUT_SITES | _lib.OUT_FP64) and not _lib.OUT_SCHEDULE_SWEEP & (_lib.OUT_SITES | _lib.OUT_FP64)
    # n_variants takes tmh_schedule's tail padding
    assert C.sizeof(_lib.ScheduleSweep) == C.sizeof(_lib.Schedule)
    assert _lib.ScheduleSweep.n_variants.offset == _lib.Schedule.n_rules.offset + 4 == C.sizeof(_lib.Schedule) - 4
    assert [f[0] for f in _lib.ScheduleSweep._fields_][:7] == [f[0] for f in _lib.Schedule._fields_]
    L = _lib.load()
    buf = np.zeros(2 * 13 * 4, dtype=np.int64)
    p = buf.ctypes.data
    tbl = _lib.Intervals(p, 0, 10, 10, 4)
    good = dict(table=tbl, soc=p, work=p, work_bytes=48, params=p, rule_of_interval=p, n_rules=2, n_variants=2)
    assert L.tmh_set_schedule_sweep(None, C.byref(_lib.ScheduleSweep(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_schedule_sweep(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    for kw, word in ((dict(soc=None), b"soc"), (dict(soc=p + 4), b"soc"), (dict(work=None), b"work"), (dict(work=p + 4), b"work"),
                     (dict(work_bytes=40), b"work buffer too small"), (dict(params=None), b"params"), (dict(params=p + 4), b"params"),
                     (dict(rule_of_interval=None), b"rule_of_interval"), (dict(n_rules=0), b"n_rules"), (dict(n_rules=9), b"n_rules"),
                     (dict(n_variants=0), b"n_variants"), (dict(n_variants=17), b"n_variants"),
                     (dict(table=_lib.Intervals(p, 0, 10, 1 << 23, 4)), b"2^23"),
                     (dict(table=_lib.Intervals(p + 4, 0, 10, 10, 4)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(p, 0, 10, 0, 4)), b"interval_s"), (dict(table=_lib.Intervals(p, 0, 0, 10, 4)), b"n_steps"),
                     (dict(table=_lib.Intervals(p, 0, 10, 10, 0)), b"ld"), (dict(table=_lib.Intervals(None, 0, 10, 10, 4)), b"buffer")):
        assert L.tmh_set_schedule_sweep(None, C.byref(_lib.ScheduleSweep(**{**good, **kw}))) == -1, kw
        assert word in L.tmh_last_error() and b"schedule sweep" in L.tmh_last_error(), (kw, L.tmh_last_error())
