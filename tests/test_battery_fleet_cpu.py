"""The battery fleet series without a GPU: the contract in numpy (battery.fleet_from_traces, a plain loop over
the seconds sharing battery.from_traces' per-second code) on the oracle's traces of base input A -- with the
one-module system (series_util.a_oracle) and with the 60-module system of the battery tests
(storage_util.a60_oracle, the GPU tests' input) -- and per-chain batteries (battery_util.recipe): against the
fleet series, against the battery table summed over the chains, against a loop written apart, the row
identities, the groups, the teeth of the input, fleet_to_watts, and the C-ABI's setter.  Integers: every
comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from battery_util import QUARTER_WH, recipe, uniform
from series_util import A_N, A_STEPS, a_has_teeth, a_oracle
from storage_util import a60_oracle
from tmhpvsim_amd import _lib, battery, registers, series
from tmhpvsim_amd.battery import fleet_from_traces, fleet_to_watts

PARAMS, SOC0 = recipe()
IV = 900
INPUTS = {"a": a_oracle, "a60": a60_oracle}


@pytest.fixture(scope="module", params=sorted(INPUTS))
def inp(request):
    """One input's traces, its one-group fleet table and the SoC after it."""
    ref = INPUTS[request.param]()
    raw, end = fleet_from_traces(ref["pv"], ref["meter"], ref["covered"], params=PARAMS, soc0=SOC0)
    assert raw.shape == (1, A_STEPS, 8) and raw.dtype == np.int64 and end.shape == (A_N,)
    raw.setflags(write=False)
    return dict(name=request.param, pv=ref["pv"], meter=ref["meter"], cov=ref["covered"], status=ref["status"], raw=raw,
                end=end)


def _sum_b(r):
    """The fleet's net battery power of rows [..., 8], from the row identity."""
    return r[..., 4] - r[..., 5] - (r[..., 1] - r[..., 0])


def test_columns_and_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_BATTERY_FLEET_COLS 8" in hdr and len(battery.FLEET_COLUMNS) == 8
    assert "#define TMH_OUT_BATTERY_FLEET 9" in hdr and _lib.OUT_BATTERY_FLEET == 9 < _lib.OUT_SITES
    assert "#define TMH_ABI_VERSION 1" in hdr and "tmh_set_battery_fleet" in _lib.EXPORTS
    assert battery.FLEET_COLUMNS[:4] == series.COLUMNS
    assert battery.FLEET_COLUMNS[4:] == ("import", "export", "soc", "charge")


def test_first_four_columns_are_the_fleet_series(inp):
    np.testing.assert_array_equal(inp["raw"][..., :4], series.from_traces(inp["pv"], inp["meter"], inp["cov"]))
    assert inp["raw"][0, :, 2].max() > 900 and inp["raw"][0, :, 3].max() > 0


def test_interval_sums_are_the_battery_table(inp):
    """Summed over each metering interval, import, export and charge are the battery table's summed over the
    chains, the net battery power is its [6] - [7], and the row of an interval's last second holds the table's
    end-of-interval state of charge of the chains that are ok at that second; soc_end is from_traces' own."""
    table, end = battery.from_traces(inp["pv"], inp["meter"], inp["cov"], IV, params=PARAMS, soc0=SOC0)
    np.testing.assert_array_equal(inp["end"], end)
    r = inp["raw"][0]
    soc, off = battery.unpack_soc(table[:, 8])
    for k in range(table.shape[0]):
        rows = r[k * IV:(k + 1) * IV]
        for col, tcol in ((4, 4), (5, 5), (7, 6)):
            assert int(rows[:, col].sum()) == int(table[k, tcol].sum()), (k, col)
        assert int(_sum_b(rows).sum()) == int(table[k, 6].sum() - table[k, 7].sum())
        at_end = off[k] == len(rows) - 1                                   # ok at the interval's last second
        assert at_end.sum() > 900 and int(rows[-1, 6]) == int(soc[k, at_end].sum()), k
        assert int(rows[-1, 2]) == int(at_end.sum())


def test_a_loop_written_apart(inp):
    """All eight columns, second by second, of a slice of chains (dead at construction, faulting inside the
    window, every capacity) against a per-chain loop over Python integers."""
    cov, status = inp["cov"], inp["status"]
    dead = np.flatnonzero(status == 1)[:2]
    faulted = np.flatnonzero((cov[-1] == 255) & (cov[0] != 255))
    live = np.flatnonzero(cov[-1] != 255)
    chains = np.unique(np.r_[dead, faulted, np.concatenate([live[PARAMS[0, live] == c * QUARTER_WH][:2] for c in range(4)])])
    assert len(chains) >= 12
    lo, hi = 5400, 6600                                   # across sunrise; the first in-window fault is at 6429
    pv, meter, cv = (a[lo:hi, chains] for a in (inp["pv"], inp["meter"], cov))
    x0 = np.arange(len(chains), dtype=np.int64) * 100000  # (clamped into [0, C])
    got, end = fleet_from_traces(pv, meter, cv, params=PARAMS[:, chains], soc0=x0)
    want = np.zeros((hi - lo, 8), dtype=np.int64)
    K = battery.FRAC_BITS
    for i, c in enumerate(chains):
        cap, pc, pd, ec, ed, sb = (int(v) for v in PARAMS[:, c])
        kc, kd = -(-(1 << 32) // ec), -(-(1 << 32) // ed)
        x = min(max(int(x0[i]), 0), cap)
        for t in range(hi - lo):
            if np.isnan(pv[t, i]) or np.isnan(meter[t, i]) or cv[t, i] == 255:
                continue
            qp, qm = round(float(pv[t, i]) * 2 ** K), round(float(meter[t, i]) * 2 ** K)
            d = qp - qm
            a = min(max(d, -pd), pc)
            s = (a * ec) >> 16 if a >= 0 else -((-a * kd + 65535) >> 16)
            x1 = min(max(x + s, 0), cap)
            g = x1 - x
            b = a if g == s else min(a, (g * kc + 65535) >> 16) if g > 0 else -min(-a, (-g * ed) >> 16) if g < 0 else 0
            x = max(x1 - sb, 0)
            want[t] += (qp, qm, 1, int(cv[t, i] == 1), max(b - d, 0), max(d - b, 0), x, max(b, 0))
        assert int(end[i]) == x
    np.testing.assert_array_equal(got[0], want)
    assert want[:, 2].min() < want[:, 2].max() == len(chains) - len(dead)
    active = (want[:, 4:] > 0).any(axis=0)                # (one module's sunrise never exceeds these chains' meters)
    assert active.all() if inp["name"] == "a60" else active[0], active


def test_row_identities(inp):
    r = inp["raw"][0]
    assert (r[:, 4:] >= 0).all() and int(r[:, 6].max()) <= int(PARAMS[0].sum())
    sb = _sum_b(r)
    assert ((r[:, 7] - sb) >= 0).all()                                      # the discharging power
    ok, d = battery._ok_d(inp["pv"], inp["meter"], inp["cov"])
    np.testing.assert_array_equal(r[:, 4] - r[:, 5], np.where(ok, -d, 0).sum(axis=1) + sb)
    assert (np.abs(sb) <= np.where(ok, np.abs(d), 0).sum(axis=1)).all()    # b lies between 0 and d
    # the bounds the kernel's 32-bit half-wave partials rest on, per chain-second
    q = battery.quantize
    assert int(q(np.nan_to_num(inp["meter"])).max()) < 1 << 26 and int(np.abs(q(np.nan_to_num(inp["pv"]))).max()) < 1 << 26
    assert int(PARAMS[0].max()) < 1 << 40


def test_no_battery_gives_the_registers(inp):
    """capacity = 0 for every chain.  With lossless conversion the rows' import and export are the import /
    export registers' per-second sums and columns 6 and 7 are 0.  With the recipe's efficiencies an ask of one
    unit stores floor(ec / 2^16) = 0 units and counts as not clipped (tmh_battery's rule: b = a = 1 when g == s
    == 0), so exactly the ok chain-seconds with d == 1 and ec < 2^16 move one unit from the export to the
    charge column; nothing else differs and the state of charge stays 0."""
    pv, meter, cov = inp["pv"], inp["meter"], inp["cov"]
    ok, d = battery._ok_d(pv, meter, cov)
    want_im, want_ex = np.where(ok, np.maximum(-d, 0), 0).sum(axis=1), np.where(ok, np.maximum(d, 0), 0).sum(axis=1)
    reg = registers.from_traces(pv, meter, cov, IV)
    for k in range(reg.shape[0]):                                           # (the per-second sums are the registers')
        assert int(want_im[k * IV:(k + 1) * IV].sum()) == int(reg[k, 4].sum())
        assert int(want_ex[k * IV:(k + 1) * IV].sum()) == int(reg[k, 5].sum())
    none = PARAMS.copy()
    none[0] = 0
    lossless = uniform(A_N, 0, 1000 << 12, 1000 << 12)
    raw, end = fleet_from_traces(pv, meter, cov, params=lossless, soc0=SOC0)
    np.testing.assert_array_equal(raw[0, :, 4], want_im)
    np.testing.assert_array_equal(raw[0, :, 5], want_ex)
    assert not raw[0, :, 6:].any() and not end.any()
    raw, end = fleet_from_traces(pv, meter, cov, params=none, soc0=SOC0)
    one = (ok & (d == 1) & (none[3] < 65536)).sum(axis=1)
    np.testing.assert_array_equal(raw[0, :, 4], want_im)
    np.testing.assert_array_equal(raw[0, :, 5], want_ex - one)
    np.testing.assert_array_equal(raw[0, :, 7], one)
    assert not raw[0, :, 6].any() and not end.any() and int(one.sum()) <= 10


def test_groups_sum_to_the_one_group_table(inp):
    raw, end = fleet_from_traces(inp["pv"], inp["meter"], inp["cov"], params=PARAMS, soc0=SOC0, group_chains=512)
    assert raw.shape == (2, A_STEPS, 8)
    np.testing.assert_array_equal(raw.sum(axis=0), inp["raw"][0])
    np.testing.assert_array_equal(end, inp["end"])
    assert raw[0, :, 2].max() <= 512 and raw[1, :, 2].max() <= A_N - 512 and raw[1].any()
    part, _ = fleet_from_traces(inp["pv"][:, 512:], inp["meter"][:, 512:], inp["cov"][:, 512:], params=PARAMS[:, 512:],
                                soc0=SOC0[512:])
    np.testing.assert_array_equal(part[0], raw[1])


def test_the_input_bites():
    """Conditions on the GPU tests' input (the 60-module system), asserted of the reference, each threshold a
    round number well below what the oracle's traces give: 4,929 seconds at which the fleet imports and exports
    at once, at each of which the import differs from max(net, 0); 2,515 seconds at which the stored energy
    rises and 2,554 at which it falls; and a peak import that the batteries lower.  Over the whole window the
    peak is a second before sunrise (step 4,435), by when every battery has run empty, and is the same with and
    without batteries; over the window's last hour, in daylight, the batteries take 10,657 W off the peak (both
    at step 7,369).  With the one-module system the batteries stay empty all morning: no teeth there."""
    ref = a60_oracle()
    pv, meter, cov = ref["pv"], ref["meter"], ref["covered"]
    _, first = a_has_teeth(pv, cov, ref["status"])
    r = fleet_from_traces(pv, meter, cov, params=PARAMS, soc0=SOC0)[0][0]
    none = PARAMS.copy()
    none[0] = 0
    r0 = fleet_from_traces(pv, meter, cov, params=none, soc0=0)[0][0]
    both = (r[:, 4] > 0) & (r[:, 5] > 0)
    net = r[:, 1] - r[:, 0] + _sum_b(r)
    d6 = np.diff(r[:, 6])
    hour = slice(A_STEPS - 3600, A_STEPS)
    pk, pk0 = int(r[hour, 4].max()), int(r0[hour, 4].max())
    print(dict(both=int(both.sum()), not_net=int((r[:, 4] != np.maximum(net, 0)).sum()), rises=int((d6 > 0).sum()),
               falls=int((d6 < 0).sum()), peak_w=pk / 4096, peak_none_w=pk0 / 4096, whole=int(r[:, 4].max()),
               whole_none=int(r0[:, 4].max()), first_daylight=first))
    assert int(both.sum()) >= 2000
    assert int((r[:, 4] != np.maximum(net, 0)).sum()) >= 2000
    assert int((d6 > 0).sum()) >= 1000 and int((d6 < 0).sum()) >= 1000
    assert first < A_STEPS - 3600 and pk0 - pk >= 5000 << 12                 # 5 kW
    assert int(r[:, 4].argmax()) < first                                     # (the whole window's peak: at night)


def test_fleet_to_watts(inp):
    raw = inp["raw"]
    w1, w60 = fleet_to_watts(raw), fleet_to_watts(raw, bin_s=60)
    assert set(w1) == {"pv", "meter", "import_w", "export_w", "charge_w", "discharge_w", "soc_wh", "n_ok", "covered"}
    s = 4096.0
    r = raw[0].astype(np.int64)
    np.testing.assert_array_equal(w1["import_w"][0], r[:, 4] / s)
    np.testing.assert_array_equal(w1["soc_wh"][0], r[:, 6] / s / 3600.0)
    np.testing.assert_array_equal(w1["discharge_w"][0], (r[:, 7] - _sum_b(r)) / s)
    nb = -(-A_STEPS // 60)
    assert all(v.shape == (1, nb) for v in w60.values()) and A_STEPS % 60 == 3
    for b in (0, 7, 93, nb - 1):                                            # by hand: integers first, one division
        rows = r[60 * b:60 * b + 60]
        t = rows.sum(axis=0)
        assert w60["pv"][0, b] == t[0] / s and w60["meter"][0, b] == t[1] / s and w60["n_ok"][0, b] == t[2]
        assert w60["covered"][0, b] == t[3] / t[2]
        assert w60["import_w"][0, b] == t[4] / s and w60["export_w"][0, b] == t[5] / s and w60["charge_w"][0, b] == t[7] / s
        assert w60["discharge_w"][0, b] == (t[7] - (t[4] - t[5] - (t[1] - t[0]))) / s
        assert w60["soc_wh"][0, b] == t[6] / (s * len(rows) * 3600.0)
    m = fleet_to_watts(raw, bin_s=60, mean=True)
    t = r[:60].sum(axis=0)
    assert m["import_w"][0, 0] == t[4] / (t[2] * s) and m["soc_wh"][0, 0] == t[6] / (t[2] * s * 3600.0)
    empty = fleet_to_watts(np.zeros((1, 5, 8), dtype=np.int64))
    assert np.isnan(empty["import_w"]).all() and (empty["n_ok"] == 0).all()
    for bad in (raw[..., :4], raw[0, 0]):
        with pytest.raises(ValueError):
            fleet_to_watts(bad)
    with pytest.raises(ValueError):
        fleet_to_watts(raw, bin_s=0)


def test_bad_shapes(inp):
    pv, meter, cov = (inp[k][:50, :20] for k in ("pv", "meter", "cov"))
    par, x0 = PARAMS[:, :20], SOC0[:20]
    fleet_from_traces(pv, meter, cov, params=par, soc0=x0)
    for kw in (dict(params=par[:, :19], soc0=0), dict(params=par[:5], soc0=0), dict(params=par.astype(np.int32), soc0=0),
               dict(params=par, soc0=x0, group_chains=100), dict(params=par, soc0=x0, group_chains=-512)):
        with pytest.raises(ValueError):
            fleet_from_traces(pv, meter, cov, **kw)
    with pytest.raises(ValueError):
        fleet_from_traces(pv, meter[:, :19], cov, params=par, soc0=x0)
    worse = par.copy()
    worse[3, 5] = 70000
    with pytest.raises(ValueError, match="eff_charge"):
        fleet_from_traces(pv, meter, cov, params=worse, soc0=x0)


def test_abi_setter_refusals():
    """Host-side only: what tmh_set_battery_fleet refuses before it touches an engine (an fp32 engine's refusal
    needs an engine, so a device: tests/test_gpu_battery_fleet.py)."""
    L = _lib.load()
    assert L.tmh_abi_version() == 1 and C.sizeof(_lib.Series) == 32             # tmh_series as it was
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data

    def refused(word, *args):
        assert L.tmh_set_battery_fleet(None, C.byref(_lib.Series(*args))) == -1
        msg = L.tmh_last_error().decode()
        assert "battery fleet" in msg and word in msg, msg

    refused("buffer", None, 0, 8, 0, 1, 0)
    refused("n_steps", p, 0, 0, 0, 1, 0)
    refused("n_groups", p, 0, 8, 0, 0, 0)
    refused("8-byte aligned", p + 4, 0, 8, 0, 1, 0)
    refused("multiple of 512", p, 0, 8, 100, 1, 0)
    refused("multiple of 512", p, 0, 8, 0, 2, 0)
    assert L.tmh_set_battery_fleet(None, C.byref(_lib.Series(p, 0, 8, 0, 1, 0))) == -1
    assert b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_battery_fleet(None, None) == -1 and b"NULL engine" in L.tmh_last_error()
    assert not buf.any()
