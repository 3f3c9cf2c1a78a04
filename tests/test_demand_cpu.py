"""The demand registers without a GPU: the contract in numpy (tmhpvsim_amd.demand) against a
plain loop on the oracle's traces of base input A, the properties of the packed keys (the
peak, its earliest second), that the peaks say what no sum says (the test's teeth), the
watt conversion, the C-ABI's struct and setter, and the `demand` command's refusals."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from series_util import A_N, A_STEPS, a_has_teeth, a_oracle
from tmhpvsim_amd import _lib, demand, registers, series

K = demand.FRAC_BITS
CASES = [(7, 0), (60, 0), (900, 0), (60, 17), (900, 3)]


def test_units_and_columns():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_DEMAND 6" in hdr and _lib.OUT_DEMAND == 6
    assert "#define TMH_DEMAND_COLS 8" in hdr
    assert (K, demand.MAX_W) == (series.FRAC_BITS, series.MAX_W)
    assert demand.COLUMNS[:6] == registers.COLUMNS and demand.COLUMNS[6:] == ("peak_import", "peak_export")
    assert [demand.n_intervals(s, 900) for s in (0, 1, 900, 901, A_STEPS)] == [0, 1, 1, 2, 13]


def test_pack_unpack():
    assert int(demand.pack(0, 0)) == 0xFFFFFFFF and int(demand.pack(1, 0)) == (1 << 32) | 0xFFFFFFFF
    assert int(demand.pack(5, 3)) == (5 << 32) | 0xFFFFFFFC
    v = np.array([0, 1, 12345, (1 << 27) - 1, 0, 7], dtype=np.int64)
    o = np.array([0, 899, 17, (1 << 32) - 2, (1 << 32) - 2, 0], dtype=np.int64)
    key = demand.pack(v, o)
    assert key.dtype == np.int64 and (key > 0).all()
    gv, go = demand.unpack(key)
    np.testing.assert_array_equal(gv, v)
    np.testing.assert_array_equal(go, o)
    # the order: a larger value wins, then the earlier second
    assert demand.pack(2, 800) > demand.pack(1, 0) and demand.pack(2, 3) > demand.pack(2, 4)
    # 0: no ok second
    gv, go = demand.unpack(np.zeros((2, 3), dtype=np.int64))
    assert not gv.any() and (go == -1).all() and go.shape == (2, 3)
    assert [int(x) for x in demand.unpack(0)] == [0, -1]


def _loop(pv, meter, cov, interval_s, origin, chains):
    """The contract as a plain per-chain, per-second loop (Python integers)."""
    n_steps = pv.shape[0]
    out = np.zeros((-(-(origin + n_steps) // interval_s), 8, len(chains)), dtype=np.int64)
    for a, i in enumerate(chains):
        for s in range(n_steps):
            if np.isnan(pv[s, i]) or np.isnan(meter[s, i]) or cov[s, i] == 255:
                continue
            k = (origin + s) // interval_s
            o = origin + s - k * interval_s
            qp = round(float(pv[s, i]) * 2 ** K)       # Python's round: half to even
            qm = round(float(meter[s, i]) * 2 ** K)
            out[k, 0, a] += qp
            out[k, 1, a] += qm
            out[k, 2, a] += 1
            out[k, 3, a] += int(cov[s, i] == 1)
            out[k, 4, a] += max(qm - qp, 0)
            out[k, 5, a] += max(qp - qm, 0)
            out[k, 6, a] = max(int(out[k, 6, a]), (max(qm - qp, 0) << 32) | (0xFFFFFFFF - o))
            out[k, 7, a] = max(int(out[k, 7, a]), (max(qp - qm, 0) << 32) | (0xFFFFFFFF - o))
    return out


def _subset(cov):
    """test_registers_cpu's chains: two dead at construction, three that fault inside the window, 0, 1, last."""
    bad = cov == 255
    dead, faulting = np.flatnonzero(bad[0])[:2], np.flatnonzero(bad[-1] & ~bad[0])[:3]
    assert len(dead) == 2 and len(faulting) == 3
    return sorted(set(dead) | set(faulting) | {0, 1, A_N - 1}), np.flatnonzero(bad[0])


@pytest.mark.parametrize("interval_s,origin", CASES)
def test_from_traces_on_input_a(interval_s, origin):
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    a_has_teeth(pv, cov, ref["status"])
    raw = demand.from_traces(pv, meter, cov, interval_s, origin=origin)
    assert raw.dtype == np.int64 and raw.shape == (-(-(A_STEPS + origin) // interval_s), 8, A_N)
    chains, dead = _subset(cov)
    np.testing.assert_array_equal(raw[:, :, chains], _loop(pv, meter, cov, interval_s, origin, chains))
    rg = registers.from_traces(pv, meter, cov, interval_s, origin=origin)
    np.testing.assert_array_equal(raw[:, :6], rg)
    np.testing.assert_array_equal(demand.to_registers(raw), rg)
    assert not raw[:, :, dead].any()                    # dead at construction: all zeros, the peak columns included
    assert (raw[:, 6:] >= 0).all() and (raw[:, 6] > 0).any() and (raw[:, 7] >> 32 > 0).any()


@pytest.mark.parametrize("interval_s,origin", CASES)
def test_key_properties_on_input_a(interval_s, origin):
    """Every non-zero cell names an ok second of its interval with the value it states; no ok
    second of the cell has a larger value and no earlier one an equal value; peak x n_ok >= the
    sum; where nothing is exported the key names the cell's first ok second."""
    ref = a_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    raw = demand.from_traces(pv, meter, cov, interval_s, origin=origin)
    nk = raw.shape[0]
    ok = cov != 255
    d = np.where(ok, series.quantize(meter) - series.quantize(pv), 0).astype(np.int64)
    # the traces on the intervals' grid [nk, interval_s, n]; seconds outside the traces are not ok
    pad = (origin, nk * interval_s - origin - A_STEPS)
    okg = np.pad(ok, (pad, (0, 0))).reshape(nk, interval_s, A_N)
    first_ok = np.where(okg.any(axis=1), okg.argmax(axis=1), -1)                   # [nk, n]
    tie_cells = 0
    for col, sign in ((6, 1), (7, -1)):
        vg = np.pad(np.maximum(sign * d, 0), (pad, (0, 0))).reshape(nk, interval_s, A_N)
        v, o = demand.unpack(raw[:, col])
        has = raw[:, col] != 0
        np.testing.assert_array_equal(has, raw[:, 2] > 0)                          # a key iff an ok second
        assert (o[has] < interval_s).all() and (o[has] >= 0).all() and (o[~has] == -1).all() and not v[~has].any()
        oc = np.where(has, o, 0)[:, None, :]
        assert np.take_along_axis(okg, oc, axis=1)[:, 0][has].all()                # at a second that is ok ...
        np.testing.assert_array_equal(np.take_along_axis(vg, oc, axis=1)[:, 0][has], v[has])   # ... with that value
        np.testing.assert_array_equal(np.where(okg, vg, -1).max(axis=1)[has], v[has])          # no ok second has a larger one
        earlier = np.arange(interval_s)[None, :, None] < oc
        assert not (okg & earlier & (vg == v[:, None, :]))[:, :, :].any(axis=1)[has].any()     # no earlier ok second an equal one
        assert (v * raw[:, 2] >= raw[:, 4 if col == 6 else 5]).all()               # peak x n_ok >= the sum
        if col == 7:
            zero = has & (v == 0)
            tie_cells = int(zero.sum())
            np.testing.assert_array_equal(o[zero], first_ok[zero])                 # the first ok second of the cell
            # among them a cell whose first second is not its interval's (the traces begin at `origin`)
            if origin:
                assert zero[0].any() and (o[0][zero[0]] == origin).all()
    assert tie_cells > 0
    # a chain that faults inside an interval: its last cell ends early, and its keys lie before the fault
    faulting = np.flatnonzero(~ok[-1] & ok[0])
    assert len(faulting) >= 3
    for i in faulting[:3]:
        s_f = int(np.argmin(ok[:, i]))
        k_f = (origin + s_f) // interval_s
        if raw[k_f, 2, i]:
            assert demand.unpack(raw[k_f, 6:, i])[1].max() < origin + s_f - k_f * interval_s
        assert not raw[k_f + 1:, :, i].any()


def test_the_sums_hide_the_peaks_on_input_a():
    """The teeth, from the oracle's traces only: at 900 s the peak import exceeds the mean import
    in every cell with more than one ok second, and cells with feed-in exist whose peak export
    is more than twice their mean export over the ok seconds -- what no sum column states."""
    ref = a_oracle()
    raw = demand.from_traces(ref["pv"], ref["meter"], ref["covered"], 900)
    n_ok, im, ex = raw[:, 2], raw[:, 4], raw[:, 5]
    pi, pe = demand.unpack(raw[:, 6])[0], demand.unpack(raw[:, 7])[0]
    multi = n_ok > 1
    above = pi * n_ok > im
    spiky = (ex > 0) & (pe * n_ok > 2 * ex)
    ratio = (pi[multi] * n_ok[multi] / np.maximum(im[multi], 1))
    print(f"cells with > 1 ok second: {int(multi.sum())}, peak import above the mean in {int((above & multi).sum())}; "
          f"median peak / mean import {np.median(ratio):.2f}; cells with export > 0: {int((ex > 0).sum())}, "
          f"peak export > 2 x mean in {int(spiky.sum())}")
    assert multi.sum() > 10000
    assert above[multi].all()
    assert spiky.any()


def test_to_watts():
    raw = np.zeros((3, 8, 2), dtype=np.int64)
    # chain 0, interval 0: 2 ok seconds -- (pv 4 W, meter 1 W) exports 3 W at second 0, (pv 0, meter 5 W) imports 5 W at second 1
    raw[0, :, 0] = [4 << K, 6 << K, 2, 1, 5 << K, 3 << K, demand.pack(5 << K, 1), demand.pack(3 << K, 0)]
    # chain 1, interval 1: 900 ok seconds, 5400 W s imported with a peak of 12 W at second 899, 1800 W s exported, peak 4.5 W at 30
    raw[1, :, 1] = [3600 << K, 7200 << K, 900, 900, 5400 << K, 1800 << K, demand.pack(12 << K, 899),
                    demand.pack(9 << (K - 1), 30)]
    # chain 0, interval 1: night from second 2 on -- no export (key(0, first ok second)), 1 W drawn throughout
    raw[1, :, 0] = [0, 898 << K, 898, 0, 898 << K, 0, demand.pack(1 << K, 2), demand.pack(0, 2)]
    out = demand.to_watts(raw, 900, n_steps=2000)
    base = registers.to_watts(raw[:, :6], 900, n_steps=2000)
    assert set(out) == set(base) | {"peak_import", "peak_export", "t_peak_import", "t_peak_export", "load_factor"}
    assert all(v.shape == (3, 2) and v.dtype == np.float64 for v in out.values())
    for key in base:
        np.testing.assert_array_equal(out[key], base[key])
    assert (out["peak_import"][0, 0], out["t_peak_import"][0, 0]) == (5.0, 1.0)
    assert (out["peak_export"][0, 0], out["t_peak_export"][0, 0]) == (3.0, 0.0)
    assert out["load_factor"][0, 0] == 0.5                               # mean import 2.5 W of a 5 W peak
    assert (out["peak_import"][1, 1], out["t_peak_import"][1, 1]) == (12.0, 899.0)
    assert (out["peak_export"][1, 1], out["t_peak_export"][1, 1]) == (4.5, 30.0)
    assert out["load_factor"][1, 1] == 0.5                               # 6 W of 12 W
    assert (out["peak_export"][1, 0], out["t_peak_export"][1, 0]) == (0.0, 2.0)
    assert out["load_factor"][1, 0] == 1.0
    # a cell without an ok second: zero peaks, NaN times and load factor
    for key in ("t_peak_import", "t_peak_export", "load_factor"):
        assert np.isnan(out[key][0, 1]) and np.isnan(out[key][2]).all()
    for key in ("peak_import", "peak_export"):
        assert out[key][0, 1] == 0 and not out[key][2].any()
    # a peak import of 0 (pv covered the meter throughout): no load factor
    raw[2, :, 0] = [10 << K, 5 << K, 5, 0, 0, 5 << K, demand.pack(0, 0), demand.pack(1 << K, 0)]
    out2 = demand.to_watts(raw, 900)
    assert np.isnan(out2["load_factor"][2, 0]) and out2["t_peak_import"][2, 0] == 0.0
    with pytest.raises(ValueError):
        demand.to_watts(raw, 900, n_steps=2701)                          # four intervals, not three
    with pytest.raises(ValueError):
        demand.to_watts(raw[:, :6], 900)                                 # a registers table is no demand table
    with pytest.raises(ValueError):
        demand.to_registers(raw[:, :6])
    # on input A: the peaks are the keys' high words in W, and no mean exceeds its peak
    ref = a_oracle()
    r = demand.from_traces(ref["pv"], ref["meter"], ref["covered"], 900)
    w = demand.to_watts(r, 900, n_steps=A_STEPS)
    np.testing.assert_array_equal(w["peak_import"], (r[:, 6] >> 32) / 2.0 ** K)
    np.testing.assert_array_equal(w["peak_export"], (r[:, 7] >> 32) / 2.0 ** K)
    lf = w["load_factor"][r[:, 6] >> 32 > 0]
    assert (lf > 0).all() and (lf <= 1).all() and (lf < 1).any()
    np.testing.assert_array_equal(np.isnan(w["t_peak_import"]), r[:, 2] == 0)


def test_demand_abi():
    L = _lib.load()
    assert C.sizeof(_lib.Demand) == 32
    assert "tmh_set_demand" in _lib.EXPORTS
    buf = (C.c_int64 * 16)()
    a = C.addressof(buf)
    good = _lib.Demand(a, 0, 10, 5, 1)
    assert L.tmh_set_demand(None, C.byref(good)) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_demand(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    # the struct is judged before the engine: each bad field is named, and so is the table
    assert L.tmh_set_demand(None, C.byref(_lib.Demand(a + 4, 0, 10, 5, 1))) == -1
    assert b"8-byte aligned" in L.tmh_last_error() and b"demand" in L.tmh_last_error()
    assert L.tmh_set_demand(None, C.byref(_lib.Demand(None, 0, 10, 5, 1))) == -1
    assert b"buffer" in L.tmh_last_error() and b"demand" in L.tmh_last_error()
    assert L.tmh_set_demand(None, C.byref(_lib.Demand(a, 0, 10, 0, 1))) == -1
    assert b"interval_s" in L.tmh_last_error() and b"demand" in L.tmh_last_error()
    assert L.tmh_set_demand(None, C.byref(_lib.Demand(a, 0, 10, 5, 0))) == -1
    assert b"ld" in L.tmh_last_error()
    assert L.tmh_set_demand(None, C.byref(_lib.Demand(a, 0, 0, 5, 1))) == -1
    assert b"n_steps" in L.tmh_last_error()


def test_demand_command_needs_a_gpu(tmp_path, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from click.testing import CliRunner
    from tmhpvsim_amd.cli import main
    f, z = tmp_path / "dm.csv", tmp_path / "dm.npz"
    r = CliRunner().invoke(main, ["demand", str(f), "--batch", "8", "--no-realtime", "--seconds", "60",
                                  "--interval", "15", "--all-chains", str(z)])
    assert r.exit_code != 0 and "no GPU is visible" in r.output
    assert not f.exists() and not z.exists()
    r = CliRunner().invoke(main, ["demand", str(f), "--batch", "8"])   # realtime: refused as for pvsim
    assert r.exit_code != 0 and "--no-realtime" in r.output
    assert not f.exists()
