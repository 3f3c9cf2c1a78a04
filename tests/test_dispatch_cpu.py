"""Battery dispatch without a GPU: the contract in numpy (tmhpvsim_amd.dispatch) against dispatch_util's
sequential run, written apart from it, on the oracle's traces of base input A with a 60-module system and
dispatch_util.recipe's households; the per-second maps the engine's map pass and scan fold; the reductions to
the battery kind, the demand registers and the import / export registers; the cells' identities; the
parameters' quantisation; the watt views; and the C-ABI's struct and setter."""
import ctypes as C
import os

import numpy as np
import pytest

from battery_util import QUARTER_WH, WH
from dispatch_util import A_FLOORS, NO_LIMIT, W, identities, recipe, run, soc_changes, tiled
from series_util import A_N, A_STEPS
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, battery, demand, dispatch, registers, storage

K = dispatch.FRAC_BITS
PARAMS, SOC0 = recipe()
IV = 900


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@pytest.fixture(scope="module")
def a_table():
    pv, meter, cov, status = _a()
    return dispatch.from_traces(pv, meter, cov, IV, params=PARAMS, soc0=SOC0) + (status,)


@pytest.fixture(scope="module")
def a_run():
    pv, meter, cov, _ = _a()
    return run(pv, meter, cov, IV, PARAMS, SOC0)


def test_units_columns_and_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_DISPATCH 11" in hdr and _lib.OUT_DISPATCH == 11 < _lib.OUT_SITES
    assert "#define TMH_DISPATCH_COLS 13" in hdr and len(dispatch.COLUMNS) == 13
    assert "#define TMH_DISPATCH_PARAMS 9" in hdr and len(dispatch.PARAMS) == len(dispatch.RANGES) == 9
    assert "#define TMH_ABI_VERSION 1" in hdr
    assert dispatch.COLUMNS[:10] == battery.COLUMNS and dispatch.COLUMNS[10:] == ("curtailed", "peak_import", "peak_export")
    assert dispatch.PARAMS[:6] == battery.PARAMS and dispatch.RANGES[:6] == battery.RANGES
    assert dispatch.RANGES[6:] == ((0, 1 << 27),) * 3 and dispatch.NO_LIMIT == NO_LIMIT == 1 << 27
    assert PARAMS.shape == (9, A_N) and PARAMS.dtype == np.int64
    assert sorted(set(PARAMS[6].tolist())) == [0, 250 * W, 500 * W, 1000 * W]
    assert sorted(set(PARAMS[7].tolist())) == [0, 2000 * W, 4000 * W, 6000 * W]
    assert sorted(set(PARAMS[8].tolist())) == [250 * W, 500 * W, 1500 * W, NO_LIMIT]
    assert sorted(set(recipe(A_N, "C")[0][8].tolist())) == [50 * W, 100 * W, 300 * W, NO_LIMIT]
    np.testing.assert_array_equal(tiled(1300, "C")[0][:, 1000:], recipe(A_N, "C")[0][:, :300])
    dispatch.check_params(PARAMS)
    # the C-ABI: the struct is tmh_battery's, the setter refuses a NULL engine and bad structs by name
    assert C.sizeof(_lib.Dispatch) == C.sizeof(_lib.Battery)
    L = _lib.load()
    buf = np.zeros(13 * 4, dtype=np.int64)
    tbl = _lib.Intervals(buf.ctypes.data, 0, 10, 10, 4)
    good = dict(table=tbl, soc=buf.ctypes.data, work=buf.ctypes.data, work_bytes=8, params=buf.ctypes.data)
    assert L.tmh_set_dispatch(None, C.byref(_lib.Dispatch(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    for kw, word in ((dict(soc=None), b"soc"), (dict(work=None), b"work"), (dict(params=None), b"params"),
                     (dict(params=buf.ctypes.data + 4), b"params"),
                     (dict(table=_lib.Intervals(buf.ctypes.data, 0, 10, 1 << 23, 4)), b"2^23"),
                     (dict(table=_lib.Intervals(None, 0, 10, 10, 4)), b"buffer")):
        assert L.tmh_set_dispatch(None, C.byref(_lib.Dispatch(**{**good, **kw}))) == -1
        assert word in L.tmh_last_error() and b"dispatch" in L.tmh_last_error()


def test_quantize_params():
    q = dispatch.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0, 250.0, [0.0, 2000.0], 1500.0)
    assert q.dtype == np.int64 and q.shape == (9, 2)
    np.testing.assert_array_equal(q[:6], battery.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0))
    assert q[6:].tolist() == [[250 << K] * 2, [0, 2000 << K], [1500 << K] * 2]
    assert dispatch.quantize_params(1.0, 1.0, 1.0)[6:].tolist() == [[0], [0], [NO_LIMIT]]             # None: no limit
    assert dispatch.quantize_params(1.0, 1.0, 1.0, feed_in_limit_w=[None, 70.0])[8].tolist() == [NO_LIMIT, 70 << K]
    assert dispatch.quantize_params(1.0, 1.0, 1.0, feed_in_limit_w=0.0, n=3)[8].tolist() == [0] * 3   # 0: feeds nothing in
    assert dispatch.quantize_params(1.0, 1.0, 1.0, charge_above_w=0.0001220703125)[6].tolist() == [0]  # 0.5: half to even
    assert dispatch.quantize_params(1.0, 1.0, 1.0, charge_above_w=0.0003662109375)[6].tolist() == [2]  # 1.5: half to even
    top = 2.0 ** 27 / 2 ** K
    assert dispatch.quantize_params(1.0, 1.0, 1.0, 1.0, 1.0, 0.0, top, top, top)[6:].tolist() == [[1 << 27]] * 3
    good = dict(capacity_wh=1.0, charge_w=1.0, discharge_w=1.0)
    for key, bad in (("charge_above_w", -1.0), ("charge_above_w", top + 1), ("discharge_above_w", -1.0),
                     ("discharge_above_w", top + 1), ("feed_in_limit_w", -1.0), ("feed_in_limit_w", top + 1),
                     ("feed_in_limit_w", float("nan")), ("charge_above_w", [1.0, 2.0, 3.0]), ("capacity_wh", -1.0),
                     ("charge_eff", 0.4), ("feed_in_limit_w", [1.0, -1.0])):
        with pytest.raises(ValueError):
            dispatch.quantize_params(**{**good, key: bad}, n=2)
    for r, (lo, hi) in enumerate(dispatch.RANGES):                                  # check_params: each row, each side
        for v in (lo - 1, hi + 1):
            p = dispatch.quantize_params(1.0, 1.0, 1.0, n=3)
            p[r, 1] = v
            with pytest.raises(ValueError, match="dispatch"):
                dispatch.check_params(p)
    with pytest.raises(ValueError):
        dispatch.check_params(PARAMS[:6])
    with pytest.raises(ValueError):
        dispatch.check_params(PARAMS.astype(np.int32))
    assert dispatch.quantize_soc(0.25, q).tolist() == [QUARTER_WH] * 2


def test_from_traces_equals_the_independent_loop(a_table, a_run):
    """dispatch.from_traces against dispatch_util.run, two derivations of the header's text: every column and
    the end state; and the input bites (the floors of the main tests)."""
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


def test_identities_and_floors_of_the_table(a_table):
    want, end, _ = a_table
    identities(want, PARAMS)
    soc_changes(want, SOC0, end)
    lim = PARAMS[8]
    tot = want.sum(axis=0)
    assert int((tot[10] > 0).sum()) >= A_FLOORS["curtail_chains"]
    assert not tot[10, lim == NO_LIMIT].any()                                       # no limit: nothing curtailed
    assert int(tot[10].sum()) > 0 and int(tot[5].sum()) > 0 and int(tot[6].sum()) > 0 and int(tot[7].sum()) > 0
    bound = (want[:, 12] >> 32) == lim                                              # cells whose feed-in peak is the limit
    assert int(bound.sum()) >= 1000 and (want[:, 10][~bound & (want[:, 2] > 0)] == 0).all()
    # a chain with thresholds moves less energy through its battery than the same chain without them
    greedy = PARAMS.copy()
    greedy[6:8] = 0
    pv, meter, cov, _ = _a()
    some = np.flatnonzero((PARAMS[6] > 0) & (PARAMS[7] > 0) & (PARAMS[0] > 0))[:40]
    g, _ = dispatch.from_traces(pv[:, some], meter[:, some], cov[:, some], IV, params=greedy[:, some], soc0=SOC0[some])
    assert int(want[:, 6][:, some].sum()) < int(g[:, 6].sum()) and int(want[:, 7][:, some].sum()) < int(g[:, 7].sum())


@pytest.mark.parametrize("split", [5001, 5120])
def test_second_maps_compose_to_the_end_state(a_table, split):
    """The engine's structure: the seconds' maps composed per 128-s block, blocks applied in order from the window's
    start -- the end state of two windows split at `split` (off and on the block grid) is from_traces'."""
    _, end, _ = a_table
    pv, meter, cov, _ = _a()
    x = np.clip(SOC0, 0, PARAMS[0])
    for a, b in ((0, split), (split, A_STEPS)):
        ma, mlo, mhi = dispatch.second_maps(pv[a:b], meter[a:b], cov[a:b], params=PARAMS)
        for j0 in range(0, b - a, 128):
            f = storage.IDENTITY
            for j in range(j0, min(j0 + 128, b - a)):
                f = dispatch.compose(f, (ma[j], mlo[j], mhi[j]))
            x = dispatch.apply(f, x)
    np.testing.assert_array_equal(x, end)


def test_reduces_to_the_battery_kind():
    """Tc = Td = 0 and no limit: columns 0-9 and the state of charge are battery.from_traces' bit for bit, column
    10 is 0, and the peaks are those of the battery's import_b and export_b."""
    pv, meter, cov, _ = _a()
    par = PARAMS.copy()
    par[6:8], par[8] = 0, NO_LIMIT
    got, end = dispatch.from_traces(pv, meter, cov, IV, params=par, soc0=SOC0)
    want, wend = battery.from_traces(pv, meter, cov, IV, params=par[:6], soc0=SOC0)
    np.testing.assert_array_equal(got[:, :10], want)
    np.testing.assert_array_equal(end, wend)
    assert not got[:, 10].any() and int(want[:, 9].sum()) > 0
    np.testing.assert_array_equal(dispatch.to_battery(got), want)
    ma = dispatch.second_maps(pv[:2000], meter[:2000], cov[:2000], params=par)
    mb = battery.second_maps(pv[:2000], meter[:2000], cov[:2000], params=par[:6])
    for u, v in zip(ma, mb):
        np.testing.assert_array_equal(u, v)


def test_without_a_battery_reduces_to_demand_and_registers():
    """C = 0: no limit gives the demand registers' peaks (columns 11, 12 = demand's 6, 7) and the registers'
    columns; any limit splits the registers' export into [5] + [10] and caps the peak.  Exact with a lossless
    charger.  With ec < 1 the battery kind's rule takes an ask of exactly one unit (2^-12 W) although it stores
    nothing of it (s = 0 = g, so b = a): the reduction then holds up to those seconds, counted here."""
    pv, meter, cov, _ = _a()
    zero = np.zeros(A_N, dtype=np.int64)
    lossy = PARAMS.copy()
    lossy[0] = 0
    ok, d = battery._ok_d(pv, meter, cov)
    one = ok & (d - lossy[6] == 1) & (lossy[1] >= 1) & (lossy[3] < 65536)            # asks of one unit, lost
    ones = np.add.reduceat(one.astype(np.int64), np.arange(0, A_STEPS, IV), axis=0)
    got, _ = dispatch.from_traces(pv, meter, cov, IV, params=lossy, soc0=zero)
    reg = registers.from_traces(pv, meter, cov, IV)
    assert 0 < int(ones.sum()) < 100
    np.testing.assert_array_equal(got[:, 5] + got[:, 10] + ones, reg[:, 5])
    np.testing.assert_array_equal(got[:, 4], reg[:, 4])
    np.testing.assert_array_equal(got[:, 6], ones)
    par = PARAMS.copy()
    par[0], par[8] = 0, NO_LIMIT
    par[3:5] = 65536
    got, end = dispatch.from_traces(pv, meter, cov, IV, params=par, soc0=zero)
    dem = demand.from_traces(pv, meter, cov, IV)
    np.testing.assert_array_equal(got[:, 11:13], dem[:, 6:8])
    np.testing.assert_array_equal(got[:, :6], dem[:, :6])
    assert not got[:, 6:8].any() and not got[:, 9:11].any() and not end.any()
    par[8] = PARAMS[8]
    lim, _ = dispatch.from_traces(pv, meter, cov, IV, params=par, soc0=zero)
    reg = registers.from_traces(pv, meter, cov, IV)
    np.testing.assert_array_equal(lim[:, 5] + lim[:, 10], reg[:, 5])
    np.testing.assert_array_equal(lim[:, 4], reg[:, 4])
    np.testing.assert_array_equal(lim[:, 11], dem[:, 6])
    np.testing.assert_array_equal(lim[:, 12] >> 32, np.minimum(dem[:, 7] >> 32, PARAMS[8]))
    assert int(lim[:, 10].sum()) > 0
    identities(lim, par)


def test_origin_and_small_intervals():
    """A window that begins inside an interval (origin) with 7-second intervals: from_traces against the
    independent run on a slice of the chains."""
    pv, meter, cov, _ = _a()
    sl = slice(100, 160)
    a, b = 6000, 6500
    got, end = dispatch.from_traces(pv[a:b, sl], meter[a:b, sl], cov[a:b, sl], 7, params=PARAMS[:, sl], soc0=SOC0[sl], origin=3)
    want, wend, _ = run(pv[a:b, sl], meter[a:b, sl], cov[a:b, sl], 7, PARAMS[:, sl], SOC0[sl], origin=3)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(end, wend)
    off = demand.unpack(got[0, 11])[1]
    assert (off[got[0, 2] > 0] >= 3).all()
    with pytest.raises(ValueError):
        dispatch.from_traces(pv[a:b, sl], meter[a:b, sl], cov[a:b, sl], 7, params=PARAMS, soc0=0)
    with pytest.raises(ValueError):
        dispatch.from_traces(pv[a:b, sl], meter[a:b, sl], cov[a:b, sl], 1 << 23, params=PARAMS[:, sl], soc0=0)


def test_to_watts(a_table):
    want, _, _ = a_table
    out = dispatch.to_watts(want, IV, n_steps=A_STEPS)
    bat = battery.to_watts(want[:, :10], IV, n_steps=A_STEPS)
    e = 3600.0 * 2 ** K
    for key, v in bat.items():
        if key != "self_consumption":
            np.testing.assert_array_equal(out[key], v, err_msg=key)
    np.testing.assert_array_equal(out["energy_wh_curtailed"], want[:, 10] / e)
    has_pv = want[:, 0] > 0
    den = np.where(has_pv, want[:, 0], 1).astype(np.float64)
    np.testing.assert_array_equal(out["curtailed_share"][has_pv], (want[:, 10] / den)[has_pv])
    assert np.isnan(out["curtailed_share"][~has_pv]).all() and np.nanmax(out["curtailed_share"]) <= 1.0
    np.testing.assert_array_equal(out["self_consumption"][has_pv],
                                  ((want[:, 0] - want[:, 5] - want[:, 10]) / den)[has_pv])
    nocut = has_pv & (want[:, 10] == 0)
    np.testing.assert_array_equal(out["self_consumption"][nocut], bat["self_consumption"][nocut])
    for name, col in (("import", 11), ("export", 12)):
        v, o = demand.unpack(want[:, col])
        np.testing.assert_array_equal(out["peak_w_" + name], v / 2.0 ** K)
        okc = want[:, 2] > 0
        np.testing.assert_array_equal(out["t_peak_" + name][okc], o[okc].astype(np.float64))
        assert np.isnan(out["t_peak_" + name][~okc]).all()
    assert (out["peak_w_export"] <= PARAMS[8] / 2.0 ** K).all()
    assert set(out) == set(bat) | {"energy_wh_curtailed", "curtailed_share", "peak_w_import", "peak_w_export",
                                   "t_peak_import", "t_peak_export"}
    with pytest.raises(ValueError):
        dispatch.to_watts(want[:, :10], IV)
    with pytest.raises(ValueError):
        dispatch.to_battery(want[:, :12])
