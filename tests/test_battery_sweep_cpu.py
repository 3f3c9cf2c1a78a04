"""The battery sweep without a GPU: the contract's own loop (battery.sweep_from_traces, the second's rule on
[K, n] arrays) against K calls of battery.from_traces on the oracle's traces of base input A with a 60-module
system and sweep_util's variants; that the variants differ where they should and agree where they must; the
summary, the quantisation of the arguments, the C-ABI's struct and setter, and the CLI's list parsing."""
import ctypes as C
import os

import numpy as np
import pytest

from battery_util import QUARTER_WH, WH, recipe
from series_util import A_N, A_STEPS
from storage_util import a60_oracle
from sweep_util import K, ROLL, pair_shares, variants
from tmhpvsim_amd import _lib, battery

FB = battery.FRAC_BITS
PARAMS, SOC0 = variants()
IV = 900
# the smallest share of the live chains whose column-4 totals differ between two variants, as the reference gives it
# for this input (sweep_from_traces on the oracle's traces: 0.9424 for the closest of the ten pairs, printed below); a pair of
# variants that met the same batteries, or a table that ignored its variant's parameters, would give 0
MIN_PAIR_SHARE = 0.9


@pytest.fixture(scope="module")
def a_sweep():
    ref = a60_oracle()
    table, end = battery.sweep_from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=PARAMS, soc0=SOC0)
    return table, end, ref


def test_variants_header_and_abi():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_ABI_VERSION 1" in hdr and "#define TMH_OUT_BATTERY_SWEEP 10" in hdr
    assert "#define TMH_BATTERY_SWEEP_MAX 16" in hdr and "typedef struct tmh_battery_sweep" in hdr
    assert "int tmh_set_battery_sweep(struct tmh_engine*" in hdr and "size_t tmh_battery_sweep_work_bytes(" in hdr
    assert _lib.OUT_BATTERY_SWEEP == 10 < _lib.OUT_SITES and _lib.BATTERY_SWEEP_MAX == battery.SWEEP_MAX == 16
    par0, soc0 = recipe()
    assert PARAMS.shape == (K, 6, A_N) and PARAMS.dtype == np.int64 and SOC0.shape == (K, A_N) and K == 5
    np.testing.assert_array_equal(PARAMS[0], par0)
    np.testing.assert_array_equal(SOC0[0], soc0)
    for v in range(1, K):
        np.testing.assert_array_equal(PARAMS[v], np.roll(par0, v * ROLL, axis=1))
    assert (SOC0 == np.minimum(PARAMS[:, 0], QUARTER_WH)).all()
    none = PARAMS[:, 0] == 0
    assert none.any(axis=1).all() and (none.any(axis=0) & ~none.all(axis=0)).sum() > A_N // 2   # a battery in one variant, none in another
    assert len({tuple(PARAMS[v, :, 0]) for v in range(K)}) > 1                                   # chain 0 meets different batteries
    battery.check_sweep_params(PARAMS)
    par, soc = variants(2, 1300)
    assert par.shape == (2, 6, 1300) and (par[1, :, A_N:] == par[1, :, :300]).all() and soc.shape == (2, 1300)


def test_sweep_equals_k_battery_runs(a_sweep):
    """The sweep's loop against from_traces variant by variant: the table and the end state, bit for bit."""
    table, end, ref = a_sweep
    assert table.shape == (K, 13, 10, A_N) and table.dtype == np.int64 and end.shape == (K, A_N)
    for v in range(K):
        want, wend = battery.from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=PARAMS[v], soc0=SOC0[v])
        np.testing.assert_array_equal(table[v], want, err_msg=f"variant {v}")
        np.testing.assert_array_equal(end[v], wend, err_msg=f"variant {v}")
    # a soc0 above C or below 0 is clamped, a scalar is every battery's
    t2, e2 = battery.sweep_from_traces(ref["pv"][:600], ref["meter"][:600], ref["covered"][:600], 250, params=PARAMS[:2],
                                       soc0=1 << 39, origin=3)
    for v in range(2):
        want, wend = battery.from_traces(ref["pv"][:600], ref["meter"][:600], ref["covered"][:600], 250, params=PARAMS[v],
                                         soc0=PARAMS[v, 0], origin=3)
        np.testing.assert_array_equal(t2[v], want)
        np.testing.assert_array_equal(e2[v], wend)
    with pytest.raises(ValueError):
        battery.sweep_from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=PARAMS[:, :, :5], soc0=0)
    with pytest.raises(ValueError):
        battery.sweep_from_traces(ref["pv"], ref["meter"], ref["covered"], IV, params=PARAMS[0], soc0=0)


def test_the_input_has_teeth(a_sweep):
    """Every pair of variants differs in column 4 for most live chains; columns 0-3 are the same in every variant."""
    table, end, ref = a_sweep
    live = ref["status"] == 0
    shares = pair_shares(table[:, :, 4], live)
    print("live chains", int(live.sum()), "column-4 shares", {k: round(s, 4) for k, s in shares.items()})
    assert len(shares) == K * (K - 1) // 2 and min(shares.values()) >= MIN_PAIR_SHARE
    for col in (5, 6, 7, 8, 9):
        assert all((table[0, :, col] != table[v, :, col]).any() for v in range(1, K))
    for v in range(1, K):
        np.testing.assert_array_equal(table[v, :, :4], table[0, :, :4])
    assert int(table[0, :, 2].sum()) > 0 and (end != SOC0).any()


def test_sweep_summary(a_sweep):
    table, end, ref = a_sweep
    s = battery.sweep_summary(table, IV, PARAMS)
    names = {"pv": "energy_wh_pv", "meter": "energy_wh_meter", "import": "energy_wh_import", "export": "energy_wh_export",
             "charge": "energy_wh_charge", "discharge": "energy_wh_discharge", "loss": "energy_wh_loss"}
    assert set(s) == set(names.values()) | {"self_consumption", "self_sufficiency", "full_cycles"}
    for v in range(K):
        w = battery.to_watts(table[v], IV, n_steps=A_STEPS)
        for key in names.values():
            assert s[key].shape == (K, A_N)
            np.testing.assert_allclose(s[key][v], np.nansum(w[key], axis=0), rtol=1e-12, atol=1e-9, err_msg=key)
    e = float(WH)
    tot = table.sum(axis=1)
    np.testing.assert_array_equal(s["energy_wh_import"], tot[:, 4] / e)                    # integer sums first
    has_pv, has_c = tot[:, 0] != 0, PARAMS[:, 0] != 0
    with np.errstate(invalid="ignore", divide="ignore"):                                   # (the expected ratios' 0 / 0, masked below)
        sc, fc = (tot[:, 0] - tot[:, 5]) / tot[:, 0].astype(float), tot[:, 7] / PARAMS[:, 0].astype(float)
    np.testing.assert_array_equal(s["self_consumption"][has_pv], sc[has_pv])
    assert np.isnan(s["self_consumption"][~has_pv]).all() and (~has_pv).any()              # dead chains
    np.testing.assert_array_equal(s["full_cycles"][has_c], fc[has_c])
    assert np.isnan(s["full_cycles"][~has_c]).all() and (~has_c).any() and np.nanmax(s["full_cycles"]) > 0
    live = ref["status"] == 0
    assert (s["self_sufficiency"][:, live] >= 0).all() and (s["self_sufficiency"][:, live] <= 1).all()
    f = battery.sweep_summary(table, IV, PARAMS, fleet=True)
    assert f["energy_wh_import"].shape == (K,)
    np.testing.assert_array_equal(f["energy_wh_import"], tot[:, 4].sum(axis=1) / e)
    np.testing.assert_array_equal(f["full_cycles"], tot[:, 7].sum(axis=1) / PARAMS[:, 0].sum(axis=1).astype(float))
    np.testing.assert_array_equal(f["self_sufficiency"],
                                  (tot[:, 1].sum(axis=1) - tot[:, 4].sum(axis=1)) / tot[:, 1].sum(axis=1).astype(float))
    for bad in (table[:, :, :9], table[:3], table[0]):
        with pytest.raises(ValueError):
            battery.sweep_summary(bad, IV, PARAMS)


def test_quantize_sweep_params():
    """Scalars, one value per variant and [K, n] arrays."""
    q = battery.quantize_sweep_params([0.25, 0.5, 0.0], 500.0, [1000.0], 0.95, [0.9, 1.0, 1.0], 1.0, n=4)
    assert q.shape == (3, 6, 4) and q.dtype == np.int64
    for v, (cap, ed) in enumerate(((QUARTER_WH, 58982), (2 * QUARTER_WH, 65536), (0, 65536))):
        assert q[v].tolist() == [[cap] * 4, [500 << FB] * 4, [1000 << FB] * 4, [62259] * 4, [ed] * 4, [1 << FB] * 4]
        np.testing.assert_array_equal(q[v], battery.quantize_params(cap / WH, 500.0, 1000.0, 0.95, ed / 65536, 1.0, n=4))
    kn = np.arange(8, dtype=np.float64).reshape(2, 4) * 0.25
    q = battery.quantize_sweep_params(kn, [100.0, 200.0], 300.0, n=4)
    assert q.shape == (2, 6, 4) and q[:, 0].tolist() == (np.arange(8).reshape(2, 4) * QUARTER_WH).tolist()
    assert q[:, 1].tolist() == [[100 << FB] * 4, [200 << FB] * 4] and (q[:, 3:5] == 65536).all() and not q[:, 5].any()
    assert battery.quantize_sweep_params(1.0, 1.0, 1.0, n=3).shape == (1, 6, 3)             # all scalars: one variant
    assert battery.quantize_sweep_params(1.0, 1.0, 1.0, n=3, n_variants=4).shape == (4, 6, 3)
    for bad in (dict(capacity_wh=[1.0, 2.0], charge_w=[1.0, 2.0, 3.0]),                    # two lengths
                dict(capacity_wh=[1.0] * 17), dict(capacity_wh=[1.0, 2.0], n_variants=3),
                dict(capacity_wh=np.ones((2, 5))), dict(capacity_wh=[1.0, -1.0]), dict(charge_eff=[0.4, 1.0]),
                dict(capacity_wh=np.ones((2, 2, 4)))):
        with pytest.raises(ValueError):
            battery.quantize_sweep_params(**{**dict(capacity_wh=1.0, charge_w=1.0, discharge_w=1.0, n=4), **bad})
    q = battery.quantize_sweep_params([0.25, 0.5], 1.0, 1.0, n=3)
    assert battery.quantize_sweep_soc(0.25, q).tolist() == [[QUARTER_WH] * 3] * 2
    assert battery.quantize_sweep_soc([0.25, 0.5], q).tolist() == [[QUARTER_WH] * 3, [2 * QUARTER_WH] * 3]
    with pytest.raises(ValueError):
        battery.quantize_sweep_soc(0.5, q)                                                   # above variant 0's capacity
    for bad in (q[0], q.astype(np.int32), np.concatenate([q] * 9)):
        with pytest.raises(ValueError):
            battery.check_sweep_params(bad)
    worse = q.copy()
    worse[1, 3, 2] = 70000
    with pytest.raises(ValueError, match="eff_charge"):
        battery.check_sweep_params(worse)


def test_abi_sizes_and_setter_refusals():
    """Host-side only: the struct, the work buffer's size and what tmh_set_battery_sweep refuses before it touches an
    engine."""
    L = _lib.load()
    assert "tmh_set_battery_sweep" in _lib.EXPORTS and "tmh_battery_sweep_work_bytes" in _lib.EXPORTS
    assert L.tmh_abi_version() == 1
    iv = C.sizeof(_lib.Intervals)
    assert C.sizeof(_lib.BatterySweep) == iv + 5 * 8 and _lib.BatterySweep.n_variants.offset == iv + 32
    assert _lib.BatterySweep.soc.offset == iv and _lib.BatterySweep.params.offset == iv + 24
    assert C.sizeof(_lib.Battery) == iv + 4 * 8                                            # the battery kind's ABI as it was
    for n, steps, k in ((1000, 129, 5), (64, 1, 1), (65536, 86400, 16)):
        assert L.tmh_battery_sweep_work_bytes(n, steps, k) == k * L.tmh_storage_work_bytes(n, steps)
    assert L.tmh_battery_sweep_work_bytes(1000, 129, 5) == 5 * 2 * 1000 * 24
    assert L.tmh_scratch_bytes(4096, 86400) == 155575808                                   # unchanged by the kind
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    good = dict(table=_lib.Intervals(p, 0, 500, 60, 4), soc=p, work=p, work_bytes=512, params=p, n_variants=3)

    def refused(word, **kw):
        sw = _lib.BatterySweep(**{**good, **kw})
        assert L.tmh_set_battery_sweep(None, C.byref(sw)) == -1
        msg = L.tmh_last_error().decode()
        assert "battery sweep" in msg and word in msg, msg

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
    assert L.tmh_set_battery_sweep(None, C.byref(_lib.BatterySweep(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_battery_sweep(None, None) == -1


def test_cli_lists_and_refusals(tmp_path):
    """A list is one value per variant: one length K or length 1; anything else and a run without --batch are refused
    before an engine is built."""
    import click
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import SWEEP_OPTIONS, main, sweep_fleet_rows, sweep_lists
    k, opts = sweep_lists(capacity_wh=[1.0, 2.0, 3.0], charge_w=[500.0], discharge_w=[1.0, 2.0, 3.0], charge_eff=[1.0],
                          discharge_eff=[0.9], standby_w=[0.0], soc0_wh=[0.0, 0.5, 1.0])
    assert k == 3 and set(opts) == set(SWEEP_OPTIONS)
    assert opts["capacity_wh"] == [1.0, 2.0, 3.0] and opts["charge_w"] == [500.0] * 3 and opts["soc0_wh"] == [0.0, 0.5, 1.0]
    assert sweep_lists(capacity_wh=[1.0], charge_w=[2.0])[0] == 1
    with pytest.raises(click.ClickException, match="charge-w"):
        sweep_lists(capacity_wh=[1.0, 2.0, 3.0], charge_w=[1.0, 2.0])
    f = tmp_path / "sw.csv"
    base = ["battery-sweep", str(f), "--no-realtime", "--capacity-wh", "1,2,3", "--charge-w", "500", "--discharge-w", "500"]
    r = CliRunner().invoke(main, base + ["--batch", "4", "--standby-w", "1,2"])            # lengths 3 and 2
    assert r.exit_code != 0 and "standby-w" in r.output and "one value per variant" in r.output
    r = CliRunner().invoke(main, base + ["--batch", "4", "--charge-eff", "x"])
    assert r.exit_code != 0 and "charge-eff" in r.output
    r = CliRunner().invoke(main, base)                                                       # no --batch
    assert r.exit_code != 0 and "--batch" in r.output
    r = CliRunner().invoke(main, base + ["--batch", "4", "--realtime"])
    assert r.exit_code != 0 and "--no-realtime" in r.output
    r = CliRunner().invoke(main, ["battery-sweep", str(f), "--batch", "4", "--no-realtime"])
    assert r.exit_code != 0 and "capacity-wh" in r.output
    assert not f.exists()
    raw = np.zeros((2, 3, 10, 4), dtype=np.int64)
    raw[:, :, 1], raw[:, :, 4], raw[1, :, 7] = 4 * WH, WH, 2 * WH
    par = battery.quantize_sweep_params([1.0, 2.0], 1.0, 1.0, n=4)
    rows = sweep_fleet_rows(raw, 900, par)
    assert [r["energy_wh_import"] for r in rows] == [12.0, 12.0] and rows[1]["energy_wh_discharge"] == 24.0
    assert rows[1]["full_cycles"] == 3.0 and rows[0]["self_sufficiency"] == 0.75 and np.isnan(rows[0]["self_consumption"])
