"""Interval metering without a GPU: the contract in numpy (tmhpvsim_amd.intervals) on the
oracle's traces of base input A, the watt / watt-hour conversion, the C-ABI's struct and
setter, and the `intervals` command's refusal without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from series_util import A_N, A_STEPS, a_has_teeth, a_oracle
from tmhpvsim_amd import _lib, intervals, series

K = intervals.FRAC_BITS


def test_units_are_the_series():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert f"#define TMH_SERIES_FRAC_BITS {K}" in hdr
    assert "#define TMH_OUT_INTERVALS 4" in hdr and _lib.OUT_INTERVALS == 4
    assert (K, intervals.MAX_W) == (series.FRAC_BITS, series.MAX_W)
    assert intervals.COLUMNS == ("pv", "meter", "n_ok", "covered")
    assert [intervals.n_intervals(s, 900) for s in (0, 1, 900, 901, A_STEPS)] == [0, 1, 1, 2, 13]
    with pytest.raises(ValueError):
        intervals.n_intervals(10, 0)


def _loop(pv, meter, cov, interval_s, origin, chains):
    """The contract as a plain per-chain, per-second loop (Python integers)."""
    n_steps = pv.shape[0]
    out = np.zeros((-(-(origin + n_steps) // interval_s), 4, len(chains)), dtype=np.int64)
    for a, i in enumerate(chains):
        for s in range(n_steps):
            if np.isnan(pv[s, i]) or np.isnan(meter[s, i]) or cov[s, i] == 255:
                continue
            k = (origin + s) // interval_s
            out[k, 0, a] += round(float(pv[s, i]) * 2 ** K)       # Python's round: half to even
            out[k, 1, a] += round(float(meter[s, i]) * 2 ** K)
            out[k, 2, a] += 1
            out[k, 3, a] += int(cov[s, i] == 1)
    return out


@pytest.mark.parametrize("interval_s,origin", [(7, 0), (60, 0), (900, 0), (60, 17), (900, 3)])
def test_from_traces_on_input_a(interval_s, origin):
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    steps, first_day = a_has_teeth(pv, cov, ref["status"])
    raw = intervals.from_traces(pv, meter, cov, interval_s, origin=origin)
    assert raw.dtype == np.int64 and raw.shape == (-(-(A_STEPS + origin) // interval_s), 4, A_N)
    # a subset: chains faulted at construction, chains that fault inside the window, ordinary ones
    bad = cov == 255
    dead, faulting = np.flatnonzero(bad[0])[:2], np.flatnonzero(bad[-1] & ~bad[0])[:3]
    chains = sorted(set(dead) | set(faulting) | {0, 1, A_N - 1})
    assert len(dead) == 2 and len(faulting) == 3
    np.testing.assert_array_equal(raw[:, :, chains], _loop(pv, meter, cov, interval_s, origin, chains))
    # NaN / 255 seconds add nothing: a chain faulted at construction is all zeros, a chain
    # that faults inside the window has fewer ok seconds than the window
    assert not raw[:, :, dead].any()
    n_ok = raw[:, 2].sum(axis=0)
    np.testing.assert_array_equal(n_ok, (~bad).sum(axis=0))
    assert (0 < n_ok[faulting]).all() and (n_ok[faulting] < A_STEPS).all()
    assert (raw[:, 0] == 0).any() and (raw[:, 0] > 0).any()        # night and daylight
    if interval_s == 900 and origin == 0:    # the last partial interval is kept: 10,803 = 12 x 900 + 3
        assert raw.shape[0] == 13 and raw[12, 2].max() == 3 and raw[11, 2].max() == 900


def test_sum_over_chains_is_the_series_binned():
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    ser = series.from_traces(pv, meter, cov)[0]                   # [steps, 4]
    for interval_s in (7, 900):
        raw = intervals.from_traces(pv, meter, cov, interval_s)
        want = np.add.reduceat(ser, np.arange(0, A_STEPS, interval_s), axis=0)   # [n_intervals, 4]
        np.testing.assert_array_equal(raw.sum(axis=2), want)


def test_to_watts():
    raw = np.zeros((3, 4, 2), dtype=np.int64)
    # chain 0: 2 ok seconds of 1 W pv and 3 W meter, one covered; chain 1: nothing in interval 0
    raw[0, :, 0] = [2 << K, 6 << K, 2, 1]
    raw[1, :, 1] = [3600 << K, 7200 << K, 900, 900]
    out = intervals.to_watts(raw, 900, n_steps=2000)
    assert set(out) == {"pv", "meter", "residual", "energy_wh_pv", "energy_wh_meter", "energy_wh_residual", "n_ok",
                        "covered"}
    assert all(v.shape == (3, 2) and v.dtype == np.float64 for v in out.values())
    assert (out["pv"][0, 0], out["meter"][0, 0], out["residual"][0, 0], out["covered"][0, 0]) == (1.0, 3.0, 2.0, 0.5)
    assert out["energy_wh_pv"][1, 1] == 1.0 and out["energy_wh_meter"][1, 1] == 2.0
    assert out["energy_wh_residual"][1, 1] == 1.0 and out["covered"][1, 1] == 1.0
    assert out["pv"][1, 1] == 4.0 and out["n_ok"][1, 1] == 900
    # a cell without an ok second: NaN means and fraction, zero energies
    for key in ("pv", "meter", "residual", "covered"):
        assert np.isnan(out[key][0, 1]) and np.isnan(out[key][2]).all()
    for key in ("energy_wh_pv", "energy_wh_meter", "energy_wh_residual", "n_ok"):
        assert out[key][0, 1] == 0 and not out[key][2].any()
    with pytest.raises(ValueError):
        intervals.to_watts(raw, 900, n_steps=2701)                # four intervals, not three
    # on input A: residual = meter - pv, energies are the sums in Wh
    ref = a_oracle()
    r = intervals.from_traces(ref["pv"], ref["meter"], ref["covered"], 900)
    w = intervals.to_watts(r, 900, n_steps=A_STEPS)
    np.testing.assert_array_equal(w["energy_wh_residual"], (r[:, 1] - r[:, 0]) / 2.0 ** K / 3600.0)
    ok = r[:, 2] > 0
    np.testing.assert_array_equal(w["residual"][ok], (r[:, 1] - r[:, 0])[ok] / (r[:, 2][ok] * 2.0 ** K))
    np.testing.assert_allclose(w["energy_wh_pv"][ok], (w["pv"] * w["n_ok"] / 3600.0)[ok], rtol=1e-14)


def test_intervals_abi():
    L = _lib.load()
    assert C.sizeof(_lib.Intervals) == 8 + 8 + 4 + 4 + 8
    buf = (C.c_int64 * 8)()
    a = C.addressof(buf)
    good = _lib.Intervals(a, 0, 10, 5, 1)
    assert L.tmh_set_intervals(None, C.byref(good)) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_intervals(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    # the struct is judged before the engine: each bad field is named
    assert L.tmh_set_intervals(None, C.byref(_lib.Intervals(a + 4, 0, 10, 5, 1))) == -1
    assert b"8-byte aligned" in L.tmh_last_error()
    assert L.tmh_set_intervals(None, C.byref(_lib.Intervals(None, 0, 10, 5, 1))) == -1
    assert b"buffer" in L.tmh_last_error()
    assert L.tmh_set_intervals(None, C.byref(_lib.Intervals(a, 0, 10, 0, 1))) == -1
    assert b"interval_s" in L.tmh_last_error()
    assert L.tmh_set_intervals(None, C.byref(_lib.Intervals(a, 0, 10, 5, 0))) == -1


def test_intervals_command_needs_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    f = tmp_path / "iv.csv"
    r = CliRunner().invoke(main, ["intervals", str(f), "--batch", "8", "--no-realtime", "--seconds", "60",
                                  "--interval", "15"])
    assert r.exit_code != 0 and "no GPU is visible" in r.output
    assert not f.exists()
    r = CliRunner().invoke(main, ["intervals", str(f), "--batch", "8"])   # realtime: refused as for pvsim
    assert r.exit_code != 0 and "--no-realtime" in r.output
