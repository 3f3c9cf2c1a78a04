"""The import / export registers without a GPU: the contract in numpy (tmhpvsim_amd.registers)
against a plain loop on the oracle's traces of base input A, that A's net hides the
registers (the test's teeth), the watt / watt-hour conversion, the C-ABI's struct and setter,
and the `registers` command's refusal without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from series_util import A_N, A_STEPS, a_has_teeth, a_oracle
from tmhpvsim_amd import _lib, intervals, registers, series

K = registers.FRAC_BITS


def test_units_and_columns():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_REGISTERS 5" in hdr and _lib.OUT_REGISTERS == 5
    assert "#define TMH_REGISTERS_COLS 6" in hdr
    assert (K, registers.MAX_W) == (series.FRAC_BITS, series.MAX_W)
    assert registers.COLUMNS == ("pv", "meter", "n_ok", "covered", "import", "export")
    assert registers.COLUMNS[:4] == intervals.COLUMNS
    assert [registers.n_intervals(s, 900) for s in (0, 1, 900, 901, A_STEPS)] == [0, 1, 1, 2, 13]


def _loop(pv, meter, cov, interval_s, origin, chains):
    """The contract as a plain per-chain, per-second loop (Python integers)."""
    n_steps = pv.shape[0]
    out = np.zeros((-(-(origin + n_steps) // interval_s), 6, len(chains)), dtype=np.int64)
    for a, i in enumerate(chains):
        for s in range(n_steps):
            if np.isnan(pv[s, i]) or np.isnan(meter[s, i]) or cov[s, i] == 255:
                continue
            k = (origin + s) // interval_s
            qp = round(float(pv[s, i]) * 2 ** K)       # Python's round: half to even
            qm = round(float(meter[s, i]) * 2 ** K)
            out[k, 0, a] += qp
            out[k, 1, a] += qm
            out[k, 2, a] += 1
            out[k, 3, a] += int(cov[s, i] == 1)
            out[k, 4, a] += max(qm - qp, 0)
            out[k, 5, a] += max(qp - qm, 0)
    return out


@pytest.mark.parametrize("interval_s,origin", [(7, 0), (60, 0), (900, 0), (60, 17), (900, 3)])
def test_from_traces_on_input_a(interval_s, origin):
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    a_has_teeth(pv, cov, ref["status"])
    raw = registers.from_traces(pv, meter, cov, interval_s, origin=origin)
    assert raw.dtype == np.int64 and raw.shape == (-(-(A_STEPS + origin) // interval_s), 6, A_N)
    # the subset of test_intervals_cpu: two chains dead at construction, three that fault inside the window, 0, 1, last
    bad = cov == 255
    dead, faulting = np.flatnonzero(bad[0])[:2], np.flatnonzero(bad[-1] & ~bad[0])[:3]
    chains = sorted(set(dead) | set(faulting) | {0, 1, A_N - 1})
    assert len(dead) == 2 and len(faulting) == 3
    np.testing.assert_array_equal(raw[:, :, chains], _loop(pv, meter, cov, interval_s, origin, chains))
    # columns 0-3 are the interval table
    iv = intervals.from_traces(pv, meter, cov, interval_s, origin=origin)
    np.testing.assert_array_equal(raw[:, :4], iv)
    np.testing.assert_array_equal(registers.to_intervals(raw), iv)
    # import - export == meter - pv in every cell; both registers are sums of non-negative terms
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0])
    assert (raw[:, 4] >= 0).all() and (raw[:, 5] >= 0).all()
    assert (raw[:, 5] > 0).any() and (raw[:, 4] > 0).any()
    # chains dead at construction are all zeros
    assert not raw[:, :, np.flatnonzero(bad[0])].any()


def test_sum_over_chains_is_the_per_second_quantities_binned():
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    ok = cov != 255
    d = np.where(ok, series.quantize(meter) - series.quantize(pv), 0)
    im, ex = np.maximum(d, 0).sum(axis=1), np.maximum(-d, 0).sum(axis=1)          # per second, over the chains
    ser = series.from_traces(pv, meter, cov)[0]                                    # [steps, 4]
    for interval_s in (7, 900):
        raw = registers.from_traces(pv, meter, cov, interval_s)
        edges = np.arange(0, A_STEPS, interval_s)
        np.testing.assert_array_equal(raw[:, :4].sum(axis=2), np.add.reduceat(ser, edges, axis=0))
        np.testing.assert_array_equal(raw[:, 4].sum(axis=1), np.add.reduceat(im, edges))
        np.testing.assert_array_equal(raw[:, 5].sum(axis=1), np.add.reduceat(ex, edges))


def test_the_net_hides_the_registers_on_input_a():
    """The teeth: on the oracle's A (default 250 W module) 8,732 chain-seconds export, and 3,615
    of the 13,000 cells at 900 s have export > 0 although their net is import -- cells no
    interval table can split."""
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    ok = cov != 255
    export_s = int((ok & (series.quantize(pv) > series.quantize(meter))).sum())
    raw = registers.from_traces(pv, meter, cov, 900)
    hidden = int(((raw[:, 5] > 0) & (raw[:, 1] - raw[:, 0] > 0)).sum())
    print(f"export seconds {export_s}, cells with export > 0 and net import > 0: {hidden} of {raw.shape[0] * A_N}")
    assert export_s >= 4000 and hidden >= 1500


def test_to_watts():
    raw = np.zeros((3, 6, 2), dtype=np.int64)
    # chain 0, interval 0: 2 ok seconds -- (pv 4 W, meter 1 W) exports 3 W s, (pv 0, meter 5 W) imports 5 W s
    raw[0, :, 0] = [4 << K, 6 << K, 2, 1, 5 << K, 3 << K]
    # chain 1, interval 1: 900 ok seconds, pv 3600 W s, meter 7200 W s, 1800 W s exported
    raw[1, :, 1] = [3600 << K, 7200 << K, 900, 900, 5400 << K, 1800 << K]
    # chain 0, interval 1: night -- no PV energy, 900 W s drawn
    raw[1, :, 0] = [0, 900 << K, 900, 0, 900 << K, 0]
    out = registers.to_watts(raw, 900, n_steps=2000)
    base = intervals.to_watts(raw[:, :4], 900, n_steps=2000)
    assert set(out) == set(base) | {"energy_wh_import", "energy_wh_export", "energy_wh_self", "self_consumption",
                                    "self_sufficiency"}
    assert set(base) == {"pv", "meter", "residual", "energy_wh_pv", "energy_wh_meter", "energy_wh_residual", "n_ok",
                         "covered"}
    assert all(v.shape == (3, 2) and v.dtype == np.float64 for v in out.values())
    for key in base:
        np.testing.assert_array_equal(out[key], base[key])
    assert out["energy_wh_import"][0, 0] == 5 / 3600.0 and out["energy_wh_export"][0, 0] == 3 / 3600.0
    assert out["energy_wh_self"][0, 0] == 1 / 3600.0
    assert out["self_consumption"][0, 0] == 0.25 and out["self_sufficiency"][0, 0] == 1 / 6
    assert (out["energy_wh_import"][1, 1], out["energy_wh_export"][1, 1], out["energy_wh_self"][1, 1]) == (1.5, 0.5, 0.5)
    assert out["self_consumption"][1, 1] == 0.5 and out["self_sufficiency"][1, 1] == 0.25
    # sum of pv = 0: no self-consumption share; the consumption is all import
    assert np.isnan(out["self_consumption"][1, 0]) and out["self_sufficiency"][1, 0] == 0.0
    assert out["energy_wh_self"][1, 0] == 0.0 and out["energy_wh_import"][1, 0] == 0.25
    # a cell without an ok second: NaN ratios, zero energies
    for key in ("self_consumption", "self_sufficiency", "pv", "covered"):
        assert np.isnan(out[key][0, 1]) and np.isnan(out[key][2]).all()
    for key in ("energy_wh_import", "energy_wh_export", "energy_wh_self", "n_ok"):
        assert out[key][0, 1] == 0 and not out[key][2].any()
    with pytest.raises(ValueError):
        registers.to_watts(raw, 900, n_steps=2701)                # four intervals, not three
    with pytest.raises(ValueError):
        registers.to_watts(raw[:, :4], 900)                       # an interval table is no registers table
    # on input A: the energies are the sums in Wh, import - export is the residual energy
    ref = a_oracle()
    r = registers.from_traces(ref["pv"], ref["meter"], ref["covered"], 900)
    w = registers.to_watts(r, 900, n_steps=A_STEPS)
    np.testing.assert_array_equal(w["energy_wh_import"], r[:, 4] / 2.0 ** K / 3600.0)
    np.testing.assert_array_equal(w["energy_wh_self"], (r[:, 1] - r[:, 4]) / 2.0 ** K / 3600.0)
    np.testing.assert_allclose(w["energy_wh_import"] - w["energy_wh_export"], w["energy_wh_residual"], rtol=0, atol=1e-12)
    sc = w["self_consumption"][r[:, 0] > 0]
    assert (sc >= 0).all() and (sc <= 1).all() and (sc < 1).any()


def test_registers_abi():
    L = _lib.load()
    assert C.sizeof(_lib.Registers) == 32
    buf = (C.c_int64 * 12)()
    a = C.addressof(buf)
    good = _lib.Registers(a, 0, 10, 5, 1)
    assert L.tmh_set_registers(None, C.byref(good)) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_registers(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    # the struct is judged before the engine: each bad field is named
    assert L.tmh_set_registers(None, C.byref(_lib.Registers(a + 4, 0, 10, 5, 1))) == -1
    assert b"8-byte aligned" in L.tmh_last_error()
    assert L.tmh_set_registers(None, C.byref(_lib.Registers(None, 0, 10, 5, 1))) == -1
    assert b"buffer" in L.tmh_last_error()
    assert L.tmh_set_registers(None, C.byref(_lib.Registers(a, 0, 10, 0, 1))) == -1
    assert b"interval_s" in L.tmh_last_error()
    assert L.tmh_set_registers(None, C.byref(_lib.Registers(a, 0, 10, 5, 0))) == -1
    assert b"ld" in L.tmh_last_error()
    assert L.tmh_set_registers(None, C.byref(_lib.Registers(a, 0, 0, 5, 1))) == -1
    assert b"n_steps" in L.tmh_last_error()


def test_registers_command_needs_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    f, z = tmp_path / "rg.csv", tmp_path / "rg.npz"
    r = CliRunner().invoke(main, ["registers", str(f), "--batch", "8", "--no-realtime", "--seconds", "60",
                                  "--interval", "15", "--all-chains", str(z)])
    assert r.exit_code != 0 and "no GPU is visible" in r.output
    assert not f.exists() and not z.exists()
    r = CliRunner().invoke(main, ["registers", str(f), "--batch", "8"])   # realtime: refused as for pvsim
    assert r.exit_code != 0 and "--no-realtime" in r.output
    assert not f.exists()
