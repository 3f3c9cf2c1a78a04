"""Scheduled dispatch without a GPU: the contract in numpy (tmhpvsim_amd.schedule) against schedule_util's
sequential run, written apart from it, on the oracle's traces of base input A with a 60-module system and
schedule_util.recipe's households and tariff; the events and shares the input must hold; the cells' identities;
the per-second maps the engine's map pass and scan fold; the reductions to dispatch.from_traces; the parameters'
and the rule array's checks; the daily tariff against a per-second zoneinfo computation; the C-ABI's struct and
setter; and the CLI's --period."""
import ctypes as C
import datetime as dt
import os
from zoneinfo import ZoneInfo

import numpy as np
import pytest

from battery_util import QUARTER_WH
from dispatch_util import identities, soc_changes
from schedule_util import A_FLOORS, A_RULES, HOLD, NO_LIMIT, R, W, c_rules, limits, recipe, run, tiled
from series_util import A_N, A_STEPS
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, battery, dispatch, schedule, storage

K = schedule.FRAC_BITS
PARAMS, SOC0 = recipe()
IV = 900


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@pytest.fixture(scope="module")
def a_table():
    pv, meter, cov, status = _a()
    return schedule.from_traces(pv, meter, cov, IV, params=PARAMS, rule_of_interval=A_RULES, soc0=SOC0) + (status,)


@pytest.fixture(scope="module")
def a_run():
    pv, meter, cov, _ = _a()
    return run(pv, meter, cov, IV, PARAMS, A_RULES, SOC0)


@pytest.fixture(scope="module")
def a_rule0():
    """Rule 0 throughout, by the dispatch kind's own loop."""
    pv, meter, cov, _ = _a()
    return dispatch.from_traces(pv, meter, cov, IV, params=schedule.to_dispatch_params(PARAMS, 0), soc0=SOC0)


def _limit_params(params, rules):
    """dispatch_util.identities' argument with the limit in force per interval in row 8."""
    lim = limits(params, rules)
    fake = np.zeros((9,) + lim.shape, dtype=np.int64)
    fake[8] = lim
    return fake


def test_units_columns_header_and_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_SCHEDULE 13" in hdr and _lib.OUT_SCHEDULE == 13 < _lib.OUT_SITES
    assert "#define TMH_SCHEDULE_RULES_MAX 8" in hdr and schedule.RULES_MAX == _lib.SCHEDULE_RULES_MAX == 8
    assert "#define TMH_SCHEDULE_RULE_PARAMS 4" in hdr and len(schedule.RULE_PARAMS) == 4
    assert "#define TMH_ABI_VERSION 1" in hdr and "#define TMH_DISPATCH_COLS 13" in hdr
    assert schedule.COLUMNS == dispatch.COLUMNS and schedule.to_watts is dispatch.to_watts
    assert schedule.RULE_PARAMS == ("charge_above", "discharge_above", "feed_in_limit", "grid_charge")
    assert schedule.NO_LIMIT == NO_LIMIT == schedule.HOLD == HOLD == 1 << 27
    assert PARAMS.shape == (6 + 4 * R, A_N) and PARAMS.dtype == np.int64 and schedule.n_rules_of(PARAMS) == R == 4
    np.testing.assert_array_equal(schedule.to_dispatch_params(PARAMS, 0), __import__("dispatch_util").recipe()[0])
    assert not PARAMS[9].any() and not PARAMS[17].any() and not PARAMS[21].any()            # G = 0 but in rule 1
    assert sorted(set(PARAMS[13].tolist())) == [0, 20 * W, 100 * W, 400 * W]
    assert (PARAMS[14:16] == HOLD).all() and A_RULES.dtype == np.uint8 and A_RULES.shape == (13,)
    assert c_rules(8).tolist() == [0, 1, 2, 0, 1, 2, 0, 1] and c_rules(40).dtype == np.uint8   # (5 k = k mod 4: k mod 3)
    np.testing.assert_array_equal(tiled(1300, "C")[0][:, 1000:], recipe(A_N, "C")[0][:, :300])
    schedule.check_params(PARAMS, n_rules=R)
    schedule.check_rules(A_RULES, R, 13)
    # the C-ABI: tmh_dispatch's fields, then the array and the count; the setter refuses by name
    assert C.sizeof(_lib.Schedule) == C.sizeof(_lib.Dispatch) + 16
    assert [f[0] for f in _lib.Schedule._fields_][:5] == [f[0] for f in _lib.Dispatch._fields_]
    L = _lib.load()
    buf = np.zeros(13 * 4, dtype=np.int64)
    tbl = _lib.Intervals(buf.ctypes.data, 0, 10, 10, 4)
    good = dict(table=tbl, soc=buf.ctypes.data, work=buf.ctypes.data, work_bytes=24, params=buf.ctypes.data,
                rule_of_interval=buf.ctypes.data, n_rules=2)
    assert L.tmh_set_schedule(None, C.byref(_lib.Schedule(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_schedule(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    for kw, word in ((dict(soc=None), b"soc"), (dict(soc=buf.ctypes.data + 4), b"soc"), (dict(work=None), b"work"),
                     (dict(work=buf.ctypes.data + 4), b"work"), (dict(work_bytes=16), b"work buffer too small"),
                     (dict(params=None), b"params"), (dict(params=buf.ctypes.data + 4), b"params"),
                     (dict(rule_of_interval=None), b"rule_of_interval"),
                     (dict(n_rules=0), b"n_rules"), (dict(n_rules=9), b"n_rules"),
                     (dict(table=_lib.Intervals(buf.ctypes.data, 0, 10, 1 << 23, 4)), b"2^23"),
                     (dict(table=_lib.Intervals(buf.ctypes.data + 4, 0, 10, 10, 4)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(buf.ctypes.data, 0, 10, 0, 4)), b"interval_s"),
                     (dict(table=_lib.Intervals(buf.ctypes.data, 0, 0, 10, 4)), b"n_steps"),
                     (dict(table=_lib.Intervals(buf.ctypes.data, 0, 10, 10, 0)), b"ld"),
                     (dict(table=_lib.Intervals(None, 0, 10, 10, 4)), b"buffer")):
        assert L.tmh_set_schedule(None, C.byref(_lib.Schedule(**{**good, **kw}))) == -1, kw
        assert word in L.tmh_last_error() and b"schedule" in L.tmh_last_error(), (kw, L.tmh_last_error())


def test_from_traces_equals_the_independent_loop(a_table, a_run):
    """schedule.from_traces against schedule_util.run, two derivations of the header's text: every column and the
    end state; and the input holds the events (floors: conditions on the input)."""
    want, end, status = a_table
    got, gend, ev = a_run
    print(ev)
    for col in range(13):
        np.testing.assert_array_equal(want[:, col], got[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(end, gend)
    for name, floor in A_FLOORS.items():
        assert ev[name] >= floor, (name, ev[name], floor)
    dead = status == 1
    assert dead.any() and not want[:, :, dead].any() and (end[dead] == SOC0[dead]).all()
    assert want.shape == (13, 13, A_N) and want[12, 2].max() == 3 and want[:12, 2].max() == IV


def test_the_schedule_bites(a_table, a_rule0):
    """Against rule 0 throughout (the dispatch kind): at least 2,000 differing cells in each of columns 4-7, 9 and 10
    and another run total of the import for at least 0.6 of the chains alive at construction; intervals 2-4 (dark,
    the small batteries empty) do not differ."""
    want, _, status = a_table
    base, _ = a_rule0
    cells = {col: int((want[:, col] != base[:, col]).sum()) for col in (4, 5, 6, 7, 9, 10)}
    live = status != 1
    moved = int(((want[:, 4].sum(axis=0) != base[:, 4].sum(axis=0)) & live).sum())
    print(cells, "chains", moved, "of", int(live.sum()))
    assert all(v >= 2000 for v in cells.values()), cells
    assert moved >= 0.6 * int(live.sum())
    np.testing.assert_array_equal(want[:, :4], base[:, :4])
    np.testing.assert_array_equal(want[2:5], base[2:5])
    assert (want[1] != base[1]).any()       # (rule 0 itself, but after a grid-charging interval: the state differs)


def test_identities_and_soc_changes(a_table):
    want, end, _ = a_table
    identities(want, _limit_params(PARAMS, A_RULES))
    soc_changes(want, SOC0, end)
    lim = limits(PARAMS, A_RULES)
    bound = (want[:, 12] >> 32) == lim                                              # cells whose feed-in peak is the limit
    assert int(bound.sum()) >= 1000 and (want[:, 10][~bound & (want[:, 2] > 0)] == 0).all()
    grid = PARAMS[9 + 4 * A_RULES.astype(np.int64)] > 0                             # [n_intervals, n]: a grid-charging rule
    assert not want[:, 7][grid].any() and int(want[:, 6][grid].sum()) > 0           # it never discharges
    hold = (A_RULES == 2)
    assert not want[hold, 6].any() and not want[hold, 7].any()                      # hold: the battery rests


@pytest.mark.parametrize("split", [5001, 5120])
def test_second_maps_compose_to_the_end_state(a_table, split):
    """The engine's structure: the seconds' maps composed per 128-s block, blocks applied in order from the window's
    start -- the end state of two windows split at `split` (off and on the block grid) is from_traces'."""
    _, end, _ = a_table
    pv, meter, cov, _ = _a()
    x = np.clip(SOC0, 0, PARAMS[0])
    for a, b in ((0, split), (split, A_STEPS)):
        ma, mlo, mhi = schedule.second_maps(pv[a:b], meter[a:b], cov[a:b], IV, params=PARAMS,
                                            rule_of_interval=A_RULES[:-(-b // IV)], origin=a)
        for j0 in range(0, b - a, 128):
            f = storage.IDENTITY
            for j in range(j0, min(j0 + 128, b - a)):
                f = schedule.compose(f, (ma[j], mlo[j], mhi[j]))
            x = schedule.apply(f, x)
    np.testing.assert_array_equal(x, end)


def test_reductions_to_the_dispatch_kind(a_rule0):
    """R = 1; all rules equal with G = 0; one rule throughout: dispatch.from_traces' thirteen columns and state."""
    pv, meter, cov, _ = _a()
    base, bend = a_rule0
    one = PARAMS[:10]
    got, end = schedule.from_traces(pv, meter, cov, IV, params=one, rule_of_interval=np.zeros(13, np.uint8), soc0=SOC0)
    np.testing.assert_array_equal(got, base)
    np.testing.assert_array_equal(end, bend)
    same = np.vstack([PARAMS[:6]] + [PARAMS[6:10]] * R)
    got, end = schedule.from_traces(pv, meter, cov, IV, params=same, rule_of_interval=A_RULES, soc0=SOC0)
    np.testing.assert_array_equal(got, base)
    np.testing.assert_array_equal(end, bend)
    for r in (0, 3):                                                                # rules without grid charging
        want, wend = dispatch.from_traces(pv, meter, cov, IV, params=schedule.to_dispatch_params(PARAMS, r), soc0=SOC0)
        got, end = schedule.from_traces(pv, meter, cov, IV, params=PARAMS, rule_of_interval=np.full(13, r, np.uint8), soc0=SOC0)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(end, wend)
    assert (schedule.to_dispatch_params(PARAMS, 3) != schedule.to_dispatch_params(PARAMS, 0)).any()


def test_origin_and_small_intervals():
    """An origin inside an interval and intervals shorter than a block, on the boundary recipe: the two derivations."""
    pv, meter, cov, _ = _a()
    par, soc0 = recipe(A_N, "C")
    sl = slice(7000, 7600)
    for iv, origin in ((7, 3), (128, 3)):
        rules = c_rules(-(-(600 + origin) // iv))
        got, end = schedule.from_traces(pv[sl], meter[sl], cov[sl], iv, params=par, rule_of_interval=rules, soc0=soc0,
                                        origin=origin)
        want, wend, _ = run(pv[sl], meter[sl], cov[sl], iv, par, rules, soc0, origin=origin)
        np.testing.assert_array_equal(got, want)
        np.testing.assert_array_equal(end, wend)
        identities(got, _limit_params(par, rules))


def test_quantize_and_check_params():
    rules = [dict(charge_above_w=250.0, discharge_above_w=[0.0, 2000.0], feed_in_limit_w=1500.0),
             dict(grid_charge_w=400.0, feed_in_limit_w=[None, 70.0]), dict()]
    q = schedule.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0, rules=rules)
    assert q.dtype == np.int64 and q.shape == (18, 2)
    np.testing.assert_array_equal(q[:6], battery.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0))
    assert q[6:10].tolist() == [[250 << K] * 2, [0, 2000 << K], [1500 << K] * 2, [0, 0]]
    assert q[10:14].tolist() == [[0, 0], [0, 0], [NO_LIMIT, 70 << K], [400 << K] * 2]
    assert q[14:].tolist() == [[0, 0], [0, 0], [NO_LIMIT] * 2, [0, 0]]
    np.testing.assert_array_equal(schedule.to_dispatch_params(q, 0),
                                  dispatch.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0, 250.0, [0.0, 2000.0], 1500.0))
    assert schedule.quantize_params(1.0, 1.0, 1.0, rules=[dict(grid_charge_w=0.0003662109375)], n=3)[9].tolist() == [2] * 3
    top = 2.0 ** 27 / 2 ** K
    assert schedule.quantize_params(1.0, 1.0, 1.0, rules=[dict(charge_above_w=top, discharge_above_w=top,
                                                               feed_in_limit_w=top, grid_charge_w=top)])[6:].tolist() == [[1 << 27]] * 4
    good = dict(capacity_wh=1.0, charge_w=1.0, discharge_w=1.0)
    for key in ("charge_above_w", "discharge_above_w", "feed_in_limit_w", "grid_charge_w"):
        for bad in (-1.0, top + 1, float("nan"), [1.0, 2.0, 3.0]):
            with pytest.raises(ValueError, match="schedule"):
                schedule.quantize_params(**good, rules=[dict(), {key: bad}], n=2)
    for bad in ([], [dict()] * 9, [dict(charge_w=1.0)]):
        with pytest.raises(ValueError, match="schedule"):
            schedule.quantize_params(**good, rules=bad)
    with pytest.raises(ValueError):
        schedule.quantize_params(1.0, 1.0, 1.0, charge_eff=0.4, rules=[dict()])
    ranges = battery.RANGES + ((0, 1 << 27),) * 8
    for r, (lo, hi) in enumerate(ranges):                                           # check_params: each row, each side
        for v in (lo - 1, hi + 1):
            p = schedule.quantize_params(1.0, 1.0, 1.0, rules=[dict(), dict()], n=3)
            p[r, 1] = v
            with pytest.raises(ValueError, match="schedule"):
                schedule.check_params(p)
    for bad in (PARAMS[:6], PARAMS[:9], PARAMS[:11], np.zeros((6 + 4 * 9, 2), np.int64), PARAMS.astype(np.int32), PARAMS[0]):
        with pytest.raises(ValueError, match="schedule"):
            schedule.check_params(bad)
    with pytest.raises(ValueError, match="rules"):
        schedule.check_params(PARAMS, n_rules=3)
    with pytest.raises(ValueError, match="rule"):
        schedule.to_dispatch_params(PARAMS, 4)
    assert schedule.quantize_soc(0.25, q[:6]).tolist() == [QUARTER_WH] * 2


def test_check_rules():
    assert schedule.check_rules(A_RULES, 4, 13) is not None
    for bad, n_rules, n_iv in ((A_RULES, 3, 13), (A_RULES, 4, 12), (A_RULES, 4, 14), (A_RULES.astype(np.int64), 4, 13),
                               (A_RULES.reshape(1, 13), 4, 13), (np.full(13, 255, np.uint8), 8, 13)):
        with pytest.raises(ValueError, match="schedule"):
            schedule.check_rules(bad, n_rules, n_iv)
    pv, meter, cov, _ = _a()
    with pytest.raises(ValueError, match="schedule"):
        schedule.from_traces(pv[:900], meter[:900], cov[:900], IV, params=PARAMS, rule_of_interval=A_RULES[:2], soc0=SOC0)
    with pytest.raises(ValueError, match="schedule"):
        schedule.from_traces(pv[:900], meter[:900], cov[:900], IV, params=PARAMS[:, :5], rule_of_interval=A_RULES[:1], soc0=SOC0[:5])


def _daily_by_zoneinfo(start, tz, n_steps, interval_s, starts, step0=0):
    """An interval's rule from the wall-clock time of its first second, second by second with zoneinfo."""
    z = ZoneInfo(tz)
    t0 = dt.datetime.fromisoformat(start).replace(tzinfo=z)
    utc0 = t0.astimezone(dt.timezone.utc)
    pts = sorted(starts)
    out = []
    for k in range(-(-n_steps // interval_s)):
        loc = (utc0 + dt.timedelta(seconds=step0 + k * interval_s)).astimezone(z)
        tod = loc.hour * 3600 + loc.minute * 60 + loc.second
        rule = pts[-1][1]
        for s, r in pts:
            if s <= tod:
                rule = r
        out.append(rule)
    return np.array(out, dtype=np.uint8)


@pytest.mark.parametrize("start, n_steps, interval_s, step0", [
    ("2019-09-05 05:30:00", 10803, 900, 0),
    ("2019-09-05 05:30:00", 86400 * 2, 900, -3),
    ("2019-10-27 00:10:00", 5 * 3600, 900, 0),          # 02:00-03:00 runs twice: the edge at 02:30 is crossed twice
    ("2019-10-27 00:10:00", 5 * 3600, 420, 7),
    ("2019-03-31 00:10:00", 5 * 3600, 900, 0),          # 02:00-03:00 is skipped, its edge with it
    ("2019-03-31 00:10:00", 5 * 3600, 1000, 0),
])
def test_daily(start, n_steps, interval_s, step0):
    starts = [(0, 0), (2 * 3600 + 1800, 1), (6 * 3600, 2), (17 * 3600 + 60, 3), (22 * 3600, 1)]
    got = schedule.daily(start, "Europe/Berlin", n_steps, interval_s, starts, step0=step0)
    want = _daily_by_zoneinfo(start, "Europe/Berlin", n_steps, interval_s, starts, step0=step0)
    assert got.dtype == np.uint8 and got.shape == (-(-n_steps // interval_s),)
    np.testing.assert_array_equal(got, want)
    if start.startswith("2019-10-27") and interval_s == 900 and step0 == 0:
        # 00:10 + k * 15 min: rule 0 until 02:25, rule 1 from 02:40, rule 0 again at 02:10 the second time round
        assert got.tolist()[:16] == [0] * 10 + [1, 1] + [0, 0] + [1, 1]
    if start.startswith("2019-03-31") and interval_s == 900:
        assert got.tolist()[:9] == [0] * 8 + [1]        # 01:55 -> 03:10: the edge at 02:30 lies in the skipped hour


def test_daily_edges_and_refusals():
    # an interval that contains a period edge belongs wholly to the earlier period
    got = schedule.daily("2019-09-05 05:30:00", "Europe/Berlin", 3600, 900, [(0, 0), (5 * 3600 + 50 * 60, 1)])
    assert got.tolist() == [0, 0, 1, 1]
    # before the day's first start: the last period, over midnight
    assert schedule.daily("2019-09-05 05:30:00", None, 1800, 900, [(6 * 3600, 0), (22 * 3600, 1)]).tolist() == [1, 1]
    for bad in ([], [(86400, 0)], [(-1, 0)], [(0, 8)], [(0, 0), (0, 1)]):
        with pytest.raises(ValueError, match="schedule"):
            schedule.daily("2019-09-05 05:30:00", None, 1800, 900, bad)
    with pytest.raises(ValueError, match="schedule"):
        schedule.daily("2019-09-05 05:30:00", None, 0, 900, [(0, 0)])


def test_cli_period_parsing():
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import TABLE_CSV, main, parse_period
    assert parse_period("06:30,20,100,none,0") == (23400, dict(charge_above_w=20.0, discharge_above_w=100.0,
                                                               feed_in_limit_w=None, grid_charge_w=0.0))
    assert parse_period("22:00, 0, 0, 60, 400") == (79200, dict(charge_above_w=0.0, discharge_above_w=0.0,
                                                                feed_in_limit_w=60.0, grid_charge_w=400.0))
    for bad in ("24:00,0,0,0,0", "06:60,0,0,0,0", "0600,0,0,0,0", "06:00,0,0,0", "06:00,0,0,0,0,0", "06:00,a,0,0,0",
                "06:00,0,0,nothing,0", ""):
        with pytest.raises(ValueError, match="--period"):
            parse_period(bad)
    assert TABLE_CSV["schedule"] == TABLE_CSV["dispatch"]
    base = ["schedule", "x.csv", "--batch", "4", "--no-realtime", "--capacity-wh", "1", "--charge-w", "1", "--discharge-w", "1"]
    r = CliRunner().invoke(main, base)
    assert r.exit_code != 0 and "--period" in r.output
    r = CliRunner().invoke(main, base + ["--period", "25:00,1,1,1,1"])
    assert r.exit_code != 0 and "HH:MM" in r.output
    r = CliRunner().invoke(main, base + ["--period", "0%d:00,1,1,1,1" % 0] * 9)
    assert r.exit_code != 0 and "outside [1, 8]" in r.output
    r = CliRunner().invoke(main, ["schedule", "x.csv", "--no-realtime", "--capacity-wh", "1", "--charge-w", "1",
                                  "--discharge-w", "1", "--period", "00:00,1,1,1,1"])
    assert r.exit_code != 0 and "--batch" in r.output
