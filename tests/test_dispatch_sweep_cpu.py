"""The dispatch sweep without a GPU: the contract's own loop (dispatch.sweep_from_traces, the second's rule on
[K, n] arrays) against K calls of dispatch.from_traces and against dispatch_util's sequential run, on the oracle's
traces of base input A with a 60-module system and dispatch_sweep_util's two variant sets; that the variants differ
where they should and agree where they must; the summary, the quantisation of the arguments, the C-ABI's struct and
setter, and the CLI's list parsing."""
import ctypes as C
import os

import numpy as np
import pytest

from battery_util import QUARTER_WH, WH
from dispatch_sweep_util import (K, MIN_ROLLED_SHARE, MIN_RULES_SHARE, ROLL, RULES, pair_shares, rolled, rules,
                                 rules_equalities)
from dispatch_util import NO_LIMIT, W, identities, recipe, run, soc_changes, tiled
from series_util import A_N, A_STEPS
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, battery, dispatch

FB = dispatch.FRAC_BITS
IV = 900
SETS = {"rolled": rolled(), "rules": rules()}


@pytest.fixture(scope="module")
def a_sweeps():
    """{set: (table [K, 13, 13, n], end [K, n])} by sweep_from_traces, and the oracle's traces."""
    ref = a60_oracle()
    return {name: dispatch.sweep_from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=par, soc0=soc0)
            for name, (par, soc0) in SETS.items()}, ref


def test_variants_header_and_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_ABI_VERSION 1" in hdr and "#define TMH_OUT_DISPATCH_SWEEP 12" in hdr
    assert "#define TMH_DISPATCH_SWEEP_MAX 16" in hdr and "typedef struct tmh_dispatch_sweep" in hdr
    assert "int tmh_set_dispatch_sweep(struct tmh_engine*" in hdr
    assert _lib.OUT_DISPATCH_SWEEP == 12 < _lib.OUT_SITES and _lib.DISPATCH_SWEEP_MAX == dispatch.SWEEP_MAX == 16
    par0, soc0 = recipe()
    par, soc = SETS["rolled"]
    assert par.shape == (K, 9, A_N) and par.dtype == np.int64 and soc.shape == (K, A_N) and K == 5
    np.testing.assert_array_equal(par[0], par0)                              # variant 0: the dispatch tests' household
    np.testing.assert_array_equal(soc[0], soc0)
    for v in range(1, K):
        np.testing.assert_array_equal(par[v], np.roll(par0, v * ROLL, axis=1))
        np.testing.assert_array_equal(soc[v], np.roll(soc0, v * ROLL))
    pc, sc = rolled(K, 1300, "C")
    tp, ts = tiled(1300, "C")
    assert pc.shape == (K, 9, 1300) and sc.shape == (K, 1300)
    np.testing.assert_array_equal(pc[0], tp)
    np.testing.assert_array_equal(pc[2], np.roll(tp, 2 * ROLL, axis=1))
    np.testing.assert_array_equal(sc[2], np.roll(ts, 2 * ROLL))
    par, soc = SETS["rules"]
    assert par.shape == (K, 9, A_N) and len(RULES) == K
    for v, (tc, td, lim) in enumerate(RULES):
        np.testing.assert_array_equal(par[v, :6], par0[:6])                  # the recipe's battery, rows 0-5 unchanged
        np.testing.assert_array_equal(soc[v], soc0)
        assert (par[v, 6] == tc * W).all() and (par[v, 7] == td * W).all()
        assert (par[v, 8] == (NO_LIMIT if lim is None else lim * W)).all()
    assert RULES == ((0, 0, None), (0, 0, 1000), (500, 0, 1000), (500, 2000, 1000), (1000, 0, 500))
    for p, _ in SETS.values():
        dispatch.check_sweep_params(p)


@pytest.mark.parametrize("name", ["rolled", "rules"])
def test_sweep_equals_k_dispatch_runs(a_sweeps, name):
    """The sweep's loop against from_traces and against dispatch_util.run variant by variant: thirteen columns and the
    end state, bit for bit; the cells' identities and the intervals' SoC changes per variant."""
    (table, end), ref = a_sweeps[0][name], a_sweeps[1]
    par, soc0 = SETS[name]
    assert table.shape == (K, 13, 13, A_N) and table.dtype == np.int64 and end.shape == (K, A_N)
    for v in range(K):
        want, wend = dispatch.from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=par[v], soc0=soc0[v])
        for col in range(13):
            np.testing.assert_array_equal(table[v, :, col], want[:, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(end[v], wend, err_msg=f"variant {v}")
        other, oend, _ = run(ref["pv"], ref["meter"], ref["covered"], IV, par[v], soc0[v])
        np.testing.assert_array_equal(table[v], other, err_msg=f"variant {v}")
        np.testing.assert_array_equal(end[v], oend, err_msg=f"variant {v}")
        identities(table[v], par[v])
        soc_changes(table[v], soc0[v], end[v])
        np.testing.assert_array_equal(table[v, :, :4], table[0, :, :4])


def test_origin_clamped_start_and_refusals(a_sweeps):
    """A soc0 above C is clamped, a scalar is every battery's, an origin shifts the intervals; bad shapes are refused."""
    ref = a_sweeps[1]
    par, _ = SETS["rolled"]
    pv, meter, cov = ref["pv"][:600], ref["meter"][:600], ref["covered"][:600]
    t2, e2 = dispatch.sweep_from_traces(pv, meter, cov, 250, params=par[:2], soc0=1 << 39, origin=3)
    for v in range(2):
        want, wend = dispatch.from_traces(pv, meter, cov, 250, params=par[v], soc0=par[v, 0], origin=3)
        np.testing.assert_array_equal(t2[v], want)
        np.testing.assert_array_equal(e2[v], wend)
    with pytest.raises(ValueError):
        dispatch.sweep_from_traces(pv, meter, cov, IV, params=par[:, :, :5], soc0=0)
    with pytest.raises(ValueError):
        dispatch.sweep_from_traces(pv, meter, cov, IV, params=par[0], soc0=0)
    with pytest.raises(ValueError):
        dispatch.sweep_from_traces(pv, meter, cov, IV, params=par[:, :6], soc0=0)      # the battery sweep's six rows


def test_the_inputs_have_teeth(a_sweeps):
    """rolled: every pair of variants differs in column 4 for at least 0.9 of the live chains.  rules: every pair differs
    in column 4, 5 or 10 for at least 0.7, and variants 0 and 1, which differ in the limit alone, are equal in
    everything the limit must not touch."""
    sweeps, ref = a_sweeps
    live = ref["status"] == 0
    table, end = sweeps["rolled"]
    s4, s5, s = (pair_shares(table, live, cols) for cols in ((4,), (5,), (4, 5, 10)))
    print("live chains", int(live.sum()), "rolled: column 4", {k: round(x, 4) for k, x in s4.items()})
    print("column 5", {k: round(x, 4) for k, x in s5.items()}, "columns 4, 5, 10", {k: round(x, 4) for k, x in s.items()})
    assert len(s4) == K * (K - 1) // 2 and min(s4.values()) >= MIN_ROLLED_SHARE
    assert min(s5.values()) >= MIN_ROLLED_SHARE and min(s.values()) >= MIN_ROLLED_SHARE
    for col in range(4, 13):
        assert all((table[0, :, col] != table[v, :, col]).any() for v in range(1, K)), col
    table, end = sweeps["rules"]
    s = pair_shares(table, live, (4, 5, 10))
    print("rules: columns 4, 5, 10", {k: round(x, 4) for k, x in s.items()})
    assert min(s.values()) >= MIN_RULES_SHARE
    share5 = rules_equalities(table, end, live)
    print("rules 0 against 1: column 5 differs for", round(share5, 4))
    assert share5 >= 0.9
    assert int(table[1, :, 10].sum()) > 0 and (table[2, :, 6] != table[1, :, 6]).any() and (table[3, :, 7] != table[2, :, 7]).any()


def test_sweep_summary(a_sweeps):
    """sweep_summary against sums done by hand."""
    table, end = a_sweeps[0]["rolled"]
    par, _ = SETS["rolled"]
    s = dispatch.sweep_summary(table, IV, par)
    assert set(s) == set(battery.sweep_summary(table[:, :, :10], IV, par[:, :6])) | {
        "energy_wh_curtailed", "curtailed_share", "peak_w_import", "peak_w_export"}
    e, tot = float(WH), table.sum(axis=1)
    for key, col in (("energy_wh_pv", 0), ("energy_wh_meter", 1), ("energy_wh_import", 4), ("energy_wh_export", 5),
                     ("energy_wh_charge", 6), ("energy_wh_discharge", 7), ("energy_wh_loss", 9), ("energy_wh_curtailed", 10)):
        assert s[key].shape == (K, A_N)
        np.testing.assert_array_equal(s[key], tot[:, col] / e, err_msg=key)       # integer sums first
    for v in range(K):
        w = dispatch.to_watts(table[v], IV, n_steps=A_STEPS)
        np.testing.assert_allclose(s["energy_wh_curtailed"][v], np.nansum(w["energy_wh_curtailed"], axis=0), rtol=1e-12, atol=1e-9)
        np.testing.assert_array_equal(s["peak_w_import"][v], np.nan_to_num(w["peak_w_import"]).max(axis=0))
        np.testing.assert_array_equal(s["peak_w_export"][v], np.nan_to_num(w["peak_w_export"]).max(axis=0))
    np.testing.assert_array_equal(s["peak_w_export"], (table[:, :, 12] >> 32).max(axis=1) / float(1 << FB))
    assert (s["peak_w_export"] * (1 << FB) <= par[:, 8]).all() and s["peak_w_import"].max() > 0
    has_pv, has_c = tot[:, 0] != 0, par[:, 0] != 0
    with np.errstate(invalid="ignore", divide="ignore"):                          # (the expected ratios' 0 / 0, masked below)
        sc = (tot[:, 0] - tot[:, 5] - tot[:, 10]) / tot[:, 0].astype(float)
        cs, fc = tot[:, 10] / tot[:, 0].astype(float), tot[:, 7] / par[:, 0].astype(float)
    np.testing.assert_array_equal(s["self_consumption"][has_pv], sc[has_pv])
    np.testing.assert_array_equal(s["curtailed_share"][has_pv], cs[has_pv])
    assert np.isnan(s["curtailed_share"][~has_pv]).all() and (~has_pv).any() and np.nanmax(s["curtailed_share"]) > 0
    np.testing.assert_array_equal(s["full_cycles"][has_c], fc[has_c])
    assert np.isnan(s["full_cycles"][~has_c]).all() and (~has_c).any()
    f = dispatch.sweep_summary(table, IV, par, fleet=True)
    assert f["energy_wh_curtailed"].shape == (K,)
    np.testing.assert_array_equal(f["energy_wh_curtailed"], tot[:, 10].sum(axis=1) / e)
    np.testing.assert_array_equal(f["energy_wh_import"], tot[:, 4].sum(axis=1) / e)
    np.testing.assert_array_equal(f["curtailed_share"], tot[:, 10].sum(axis=1) / tot[:, 0].sum(axis=1).astype(float))
    np.testing.assert_array_equal(f["self_consumption"],
                                  (tot[:, 0] - tot[:, 5] - tot[:, 10]).sum(axis=1) / tot[:, 0].sum(axis=1).astype(float))
    np.testing.assert_array_equal(f["peak_w_import"], s["peak_w_import"].max(axis=1))
    np.testing.assert_array_equal(f["peak_w_export"], s["peak_w_export"].max(axis=1))
    for bad in (table[:, :, :10], table[:3], table[0]):
        with pytest.raises(ValueError):
            dispatch.sweep_summary(bad, IV, par)
    with pytest.raises(ValueError):
        dispatch.sweep_summary(table, IV, par[:, :6])


def test_quantize_sweep_params():
    """Scalars, one value per variant, [K, n] arrays and None limits."""
    q = dispatch.quantize_sweep_params([0.25, 0.5, 0.0], 500.0, [1000.0], 0.95, [0.9, 1.0, 1.0], 1.0,
                                       [0.0, 250.0, 500.0], 2000.0, [None, 1000.0, None], n=4)
    assert q.shape == (3, 9, 4) and q.dtype == np.int64
    for v, (cap, ed, tc, lim) in enumerate(((QUARTER_WH, 58982, 0, NO_LIMIT), (2 * QUARTER_WH, 65536, 250 << FB, 1000 << FB),
                                            (0, 65536, 500 << FB, NO_LIMIT))):
        assert q[v].tolist() == [[cap] * 4, [500 << FB] * 4, [1000 << FB] * 4, [62259] * 4, [ed] * 4, [1 << FB] * 4,
                                 [tc] * 4, [2000 << FB] * 4, [lim] * 4]
        np.testing.assert_array_equal(q[v], dispatch.quantize_params(cap / WH, 500.0, 1000.0, 0.95, ed / 65536, 1.0, tc / (1 << FB),
                                                                     2000.0, None if lim == NO_LIMIT else lim / (1 << FB), n=4))
    np.testing.assert_array_equal(q[:, :6], battery.quantize_sweep_params([0.25, 0.5, 0.0], 500.0, [1000.0], 0.95,
                                                                          [0.9, 1.0, 1.0], 1.0, n=4))
    kn = np.arange(8, dtype=np.float64).reshape(2, 4) * 100.0
    q = dispatch.quantize_sweep_params(1.0, 1.0, 1.0, charge_above_w=kn, feed_in_limit_w=[[None, 1.0, 2.0, None]] * 2, n=4)
    assert q.shape == (2, 9, 4) and q[:, 6].tolist() == (np.arange(8).reshape(2, 4) * (100 << FB)).tolist()
    assert q[:, 8].tolist() == [[NO_LIMIT, 1 << FB, 2 << FB, NO_LIMIT]] * 2 and not q[:, 7].any()
    one = dispatch.quantize_sweep_params(1.0, 1.0, 1.0, n=3)                               # all scalars: one variant, no limit
    assert one.shape == (1, 9, 3) and (one[0, 8] == NO_LIMIT).all() and not one[0, 6:8].any()
    assert dispatch.quantize_sweep_params(1.0, 1.0, 1.0, feed_in_limit_w=500.0, n=3, n_variants=4)[:, 8].tolist() == [[500 << FB] * 3] * 4
    base = dict(capacity_wh=1.0, charge_w=1.0, discharge_w=1.0, n=4)
    for bad in (dict(capacity_wh=[1.0, 2.0], charge_above_w=[1.0, 2.0, 3.0]),               # two lengths
                dict(feed_in_limit_w=[1.0] * 17), dict(feed_in_limit_w=[None, 1.0], n_variants=3),
                dict(discharge_above_w=np.ones((2, 5))), dict(charge_above_w=[1.0, -1.0]), dict(feed_in_limit_w=[1.0, -1.0]),
                dict(feed_in_limit_w=40000.0), dict(discharge_above_w=float("nan")), dict(charge_eff=[0.4, 1.0]),
                dict(charge_above_w=np.ones((2, 2, 4)))):
        with pytest.raises(ValueError):
            dispatch.quantize_sweep_params(**{**base, **bad})
    q = dispatch.quantize_sweep_params([0.25, 0.5], 1.0, 1.0, n=3)
    assert dispatch.quantize_sweep_soc(0.25, q).tolist() == [[QUARTER_WH] * 3] * 2
    assert dispatch.quantize_sweep_soc([0.25, 0.5], q).tolist() == [[QUARTER_WH] * 3, [2 * QUARTER_WH] * 3]
    assert dispatch.quantize_sweep_soc(np.full((2, 3), 0.25), q).tolist() == [[QUARTER_WH] * 3] * 2
    with pytest.raises(ValueError):
        dispatch.quantize_sweep_soc(0.5, q)                                                  # above variant 0's capacity


def test_check_sweep_params_each_row_and_side():
    q = dispatch.quantize_sweep_params([0.25, 0.5], 1.0, 1.0, n=3)
    for bad in (q[0], q.astype(np.int32), np.concatenate([q] * 9), q[:, :6], q[:0]):
        with pytest.raises(ValueError, match="dispatch sweep"):
            dispatch.check_sweep_params(bad)
    for row, (name, (lo, hi)) in enumerate(zip(dispatch.PARAMS, dispatch.RANGES)):
        for value in (lo - 1, hi + 1):
            worse = q.copy()
            worse[1, row, 2] = value
            with pytest.raises(ValueError, match=name):
                dispatch.check_sweep_params(worse)
        for value in (lo, hi):
            fine = q.copy()
            fine[1, row, 2] = value
            dispatch.check_sweep_params(fine)


def test_abi_sizes_and_setter_refusals():
    """Host-side only: the struct (the battery sweep's layout) and what tmh_set_dispatch_sweep refuses before it touches
    an engine, each in a message that names the dispatch sweep."""
    L = _lib.load()
    assert "tmh_set_dispatch_sweep" in _lib.EXPORTS and L.tmh_abi_version() == 1
    iv = C.sizeof(_lib.Intervals)
    assert C.sizeof(_lib.DispatchSweep) == C.sizeof(_lib.BatterySweep) == iv + 5 * 8
    for f in ("table", "soc", "work", "work_bytes", "params", "n_variants"):
        assert getattr(_lib.DispatchSweep, f).offset == getattr(_lib.BatterySweep, f).offset
    assert C.sizeof(_lib.Dispatch) == iv + 4 * 8 and C.sizeof(_lib.Battery) == iv + 4 * 8   # the other kinds' ABI as it was
    assert L.tmh_scratch_bytes(4096, 86400) == 155575808                                   # unchanged by the kind
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    good = dict(table=_lib.Intervals(p, 0, 500, 60, 4), soc=p, work=p, work_bytes=512, params=p, n_variants=3)

    def refused(word, **kw):
        sw = _lib.DispatchSweep(**{**good, **kw})
        assert L.tmh_set_dispatch_sweep(None, C.byref(sw)) == -1
        msg = L.tmh_last_error().decode()
        assert "dispatch sweep" in msg and word in msg, msg

    refused("buffer", table=_lib.Intervals(None, 0, 500, 60, 4))
    refused("8-byte aligned", table=_lib.Intervals(p + 4, 0, 500, 60, 4))
    refused("interval_s", table=_lib.Intervals(p, 0, 500, 0, 4))
    refused("n_steps", table=_lib.Intervals(p, 0, 0, 60, 4))
    refused("ld", table=_lib.Intervals(p, 0, 500, 60, 0))
    refused("2^23", table=_lib.Intervals(p, 0, 500, 1 << 23, 4))
    refused("n_variants", n_variants=0)
    refused("n_variants", n_variants=17)
    refused("soc", soc=None)
    refused("soc", soc=p + 4)
    refused("work", work=None)
    refused("work", work=p + 2)
    refused("params", params=None)
    refused("params", params=p + 4)
    refused("too small", work_bytes=3 * 24 - 8)
    assert L.tmh_set_dispatch_sweep(None, C.byref(_lib.DispatchSweep(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_dispatch_sweep(None, None) == -1


def test_cli_lists_and_refusals(tmp_path):
    """A list is one value per variant: one length K or length 1, limits `none` included; anything else and a run
    without --batch are refused before an engine is built."""
    import click
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import DISPATCH_SWEEP_OPTIONS, dispatch_sweep_fleet_rows, dispatch_sweep_lists, main
    k, opts = dispatch_sweep_lists(capacity_wh=[1.0], charge_w=[500.0], discharge_w=[1.0], charge_eff=[1.0],
                                   discharge_eff=[0.9], standby_w=[0.0], soc0_wh=[0.0, 0.5, 1.0],
                                   charge_above_w=[0.0, 250.0, 500.0], discharge_above_w=[100.0], feed_in_limit_w=[None, 700.0, None])
    assert k == 3 and set(opts) == set(DISPATCH_SWEEP_OPTIONS)
    assert opts["capacity_wh"] == [1.0] * 3 and opts["charge_above_w"] == [0.0, 250.0, 500.0]
    assert opts["feed_in_limit_w"] == [None, 700.0, None] and opts["discharge_above_w"] == [100.0] * 3
    assert dispatch_sweep_lists(capacity_wh=[1.0], feed_in_limit_w=[None]) == (1, dict(capacity_wh=[1.0], feed_in_limit_w=[None]))
    with pytest.raises(click.ClickException, match="dispatch-sweep: --feed-in-limit-w"):
        dispatch_sweep_lists(capacity_wh=[1.0, 2.0, 3.0], feed_in_limit_w=[1.0, None])
    f = tmp_path / "ds.csv"
    base = ["dispatch-sweep", str(f), "--no-realtime", "--capacity-wh", "1", "--charge-w", "500", "--discharge-w", "500",
            "--feed-in-limit-w", "none,700,500"]
    r = CliRunner().invoke(main, base + ["--batch", "4", "--charge-above-w", "1,2"])       # lengths 3 and 2
    assert r.exit_code != 0 and "charge-above-w" in r.output and "one value per variant" in r.output
    r = CliRunner().invoke(main, base + ["--batch", "4", "--feed-in-limit-w", "x"])
    assert r.exit_code != 0 and "feed-in-limit-w" in r.output
    r = CliRunner().invoke(main, base)                                                       # no --batch
    assert r.exit_code != 0 and "--batch" in r.output
    r = CliRunner().invoke(main, base + ["--batch", "4", "--realtime"])
    assert r.exit_code != 0 and "--no-realtime" in r.output
    r = CliRunner().invoke(main, ["dispatch-sweep", str(f), "--batch", "4", "--no-realtime"])
    assert r.exit_code != 0 and "capacity-wh" in r.output
    assert not f.exists()
    raw = np.zeros((2, 3, 13, 4), dtype=np.int64)
    raw[:, :, 0], raw[:, :, 1], raw[:, :, 4], raw[1, :, 7], raw[1, :, 10] = 8 * WH, 4 * WH, WH, 2 * WH, 2 * WH
    raw[1, 1, 12, 2] = (700 << FB) << 32 | 0xFFFFFFFF
    par = dispatch.quantize_sweep_params([1.0, 2.0], 1.0, 1.0, n=4)
    rows = dispatch_sweep_fleet_rows(raw, 900, par)
    assert [r["energy_wh_import"] for r in rows] == [12.0, 12.0] and rows[1]["energy_wh_discharge"] == 24.0
    assert rows[1]["full_cycles"] == 3.0 and rows[0]["self_sufficiency"] == 0.75
    assert [r["energy_wh_curtailed"] for r in rows] == [0.0, 24.0] and [r["curtailed_share"] for r in rows] == [0.0, 0.25]
    assert [r["self_consumption"] for r in rows] == [1.0, 0.75] and [r["peak_w_export"] for r in rows] == [0.0, 700.0]
