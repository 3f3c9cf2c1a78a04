"""The battery kind without a GPU: the contract in numpy (tmhpvsim_amd.battery) against a scalar loop over
Python integers on the oracle's traces of base input A with a 60-module system and per-chain batteries
(battery_util.recipe), the lossless case against tmhpvsim_amd.storage, the per-second invariants and the
cells' identities, the per-second maps the engine's map pass and scan fold, and the C-ABI's struct and
setter."""
import ctypes as C
import os

import numpy as np
import pytest

from battery_util import QUARTER_WH, WH, events, recipe, uniform
from series_util import A_N, A_STEPS, a_has_teeth
from storage_util import A_BATTERY, a60_oracle
from storage_util import battery as storage_battery
from tmhpvsim_amd import _lib, battery, intervals, storage

K = battery.FRAC_BITS
PARAMS, SOC0 = recipe()


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


@pytest.fixture(scope="module")
def a_table():
    pv, meter, cov, status = _a()
    return battery.from_traces(pv, meter, cov, 900, params=PARAMS, soc0=SOC0) + (status,)


def test_units_columns_and_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_BATTERY 8" in hdr and _lib.OUT_BATTERY == 8 < _lib.OUT_SITES
    assert "#define TMH_BATTERY_COLS 10" in hdr and len(battery.COLUMNS) == 10
    assert "#define TMH_ABI_VERSION 1" in hdr
    assert battery.COLUMNS[:9] == storage.COLUMNS and battery.COLUMNS[9] == "loss"
    assert battery.PARAMS == ("capacity", "p_charge", "p_discharge", "eff_charge", "eff_discharge", "standby")
    assert battery.RANGES == ((0, (1 << 40) - 1), (0, 1 << 27), (0, 1 << 27), (1 << 15, 1 << 16), (1 << 15, 1 << 16),
                              (0, 1 << 27))
    assert PARAMS.shape == (6, A_N) and PARAMS.dtype == np.int64 and (SOC0 == np.minimum(PARAMS[0], QUARTER_WH)).all()
    assert sorted(set(PARAMS[0].tolist())) == [0, QUARTER_WH, 2 * QUARTER_WH, 3 * QUARTER_WH]
    assert (PARAMS[3, ::7] == 65536).all() and (PARAMS[4, ::11] == 65536).all() and PARAMS[3].min() >= 58000
    battery.check_params(PARAMS)


def test_quantize_params():
    q = battery.quantize_params(0.25, [500.0, 1000.0], 1000.0, 0.95, 0.9, 1.0)
    assert q.dtype == np.int64 and q.shape == (6, 2)
    assert q.tolist() == [[QUARTER_WH] * 2, [500 << K, 1000 << K], [1000 << K] * 2, [62259] * 2, [58982] * 2, [1 << K] * 2]
    assert 0.95 * 65536 == 62259.2 and 0.9 * 65536 == 58982.4                      # rounded to nearest
    assert battery.quantize_params(1.0, 1.0, 1.0, 0.50000762939453125, 1.0).tolist()[3] == [32768]   # 32768.5: half to even
    assert battery.quantize_params(1.0, 1.0, 1.0, 0.50002288818359375, 1.0).tolist()[3] == [32770]   # 32769.5: half to even
    assert battery.quantize_params(0.0, 0.0, 0.0, n=3).tolist() == [[0] * 3, [0] * 3, [0] * 3, [65536] * 3, [65536] * 3, [0] * 3]
    top_wh, top_w = (2.0 ** 40 - 1) / WH, 2.0 ** 27 / 2 ** K
    assert battery.quantize_params(top_wh, top_w, top_w, 0.5, 0.5, top_w).tolist() == [
        [(1 << 40) - 1], [1 << 27], [1 << 27], [1 << 15], [1 << 15], [1 << 27]]
    good = dict(capacity_wh=1.0, charge_w=1.0, discharge_w=1.0, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0)
    for key, bad in (("capacity_wh", -1.0), ("capacity_wh", 2.0 ** 40 / WH), ("charge_w", -1.0), ("charge_w", top_w + 1),
                     ("discharge_w", -1.0), ("discharge_w", top_w + 1), ("charge_eff", 0.49), ("charge_eff", 1.01),
                     ("discharge_eff", 0.49), ("discharge_eff", 1.01), ("standby_w", -1.0), ("standby_w", top_w + 1),
                     ("charge_eff", float("nan")), ("capacity_wh", [1.0, -1.0]), ("charge_w", [1.0, 2.0, 3.0])):
        with pytest.raises(ValueError):
            battery.quantize_params(**{**good, key: bad}, n=2)
    assert battery.quantize_soc(0.25, q).tolist() == [QUARTER_WH] * 2
    for bad in (-0.1, 0.26):
        with pytest.raises(ValueError):
            battery.quantize_soc(bad, q)
    for r, (lo, hi) in enumerate(battery.RANGES):                                   # check_params: each row, each side
        for v in (lo - 1, hi + 1):
            p = uniform(3, WH, 5, 5)
            p[r, 1] = v
            with pytest.raises(ValueError):
                battery.check_params(p)
    with pytest.raises(ValueError):
        battery.check_params(uniform(3, WH, 5, 5)[:5])
    with pytest.raises(ValueError):
        battery.check_params(uniform(3, WH, 5, 5).astype(np.int32))


def _loop(pv, meter, cov, interval_s, origin, params, soc0):
    """The contract as a plain per-chain, per-second loop over Python integers, with the per-second
    invariants asserted: loss >= 0, |b| <= |a|, b has a's sign, every product below 2^60."""
    n_steps, n = pv.shape
    out = np.zeros((-(-(origin + n_steps) // interval_s), 10, n), dtype=np.int64)
    end = []
    for i in range(n):
        cap, pc, pd, ec, ed, sb = (int(v) for v in params[:, i])
        kc, kd = -(-(1 << 32) // ec), -(-(1 << 32) // ed)
        assert (1 << 16) <= kc <= (1 << 17) and (1 << 16) <= kd <= (1 << 17)
        x = min(max(int(soc0[i]), 0), cap)
        for t in range(n_steps):
            if np.isnan(pv[t, i]) or np.isnan(meter[t, i]) or cov[t, i] == 255:
                continue
            k, o = divmod(origin + t, interval_s)
            qp = round(float(pv[t, i]) * 2 ** K)       # Python's round: half to even
            qm = round(float(meter[t, i]) * 2 ** K)
            d = qp - qm
            a = min(max(d, -pd), pc)
            s = (a * ec) >> 16 if a >= 0 else -((-a * kd + 65535) >> 16)
            x1 = min(max(x + s, 0), cap)
            g = x1 - x
            if g == s:
                b = a
            elif g > 0:
                b = min(a, (g * kc + 65535) >> 16)
            elif g < 0:
                b = -min(-a, (-g * ed) >> 16)
            else:
                b = 0
            xn = max(x1 - sb, 0)
            loss = b - (xn - x)
            assert loss >= 0 and abs(b) <= abs(a) and b * a >= 0 and (b == 0 or (b > 0) == (a > 0))
            assert max(abs(a) * max(ec, kd), abs(g) * max(kc, ed)) + 65535 < 1 << 60
            x = xn
            out[k, 0, i] += qp
            out[k, 1, i] += qm
            out[k, 2, i] += 1
            out[k, 3, i] += int(cov[t, i] == 1)
            out[k, 4, i] += max(b - d, 0)
            out[k, 5, i] += max(d - b, 0)
            out[k, 6, i] += max(b, 0)
            out[k, 7, i] += max(-b, 0)
            out[k, 8, i] = max(int(out[k, 8, i]), ((o + 1) << 40) | xn)
            out[k, 9, i] += loss
        end.append(x)
    return out, np.array(end, dtype=np.int64)


def _slice_chains(cov, status):
    """A slice of A: chains dead at construction, the chains that fault inside the window, and live chains
    of every capacity (none included), lossless and lossy."""
    dead = np.flatnonzero(status == 1)[:2]
    faulted = np.flatnonzero((cov[-1] == 255) & (cov[0] != 255))
    live = np.flatnonzero(cov[-1] != 255)
    pick = [live[PARAMS[0, live] == c * QUARTER_WH][:2] for c in range(4)]
    lossless = live[(PARAMS[3, live] == 65536) & (PARAMS[4, live] == 65536) & (PARAMS[0, live] > 0)][:1]
    return np.unique(np.r_[dead, faulted, np.concatenate(pick), lossless])


@pytest.mark.parametrize("interval_s,origin", [(900, 0), (7, 0), (60, 17)])
def test_from_traces_against_the_scalar_loop(interval_s, origin):
    pv, meter, cov, status = _a()
    chains = _slice_chains(cov, status)
    assert len(chains) >= 12
    sub = [a[:, chains] for a in (pv, meter, cov)]          # night, the morning's charge, full, clipped, in-window faults
    par, x0 = PARAMS[:, chains], SOC0[chains]
    got, end = battery.from_traces(*sub, interval_s, origin=origin, params=par, soc0=x0)
    want, wend = _loop(*sub, interval_s, origin, par, x0)
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(end, wend)
    assert (got[:, 6].sum(axis=0) > 0).any() and (got[:, 7].sum(axis=0) > 0).any() and (got[:, 9].sum(axis=0) > 0).any()
    ev = events(*sub, par, x0)
    assert ev["partial_fill"] > 0 and ev["partial_empty"] > 0 and ev["refused"] > 0 and ev["standby_clip"] > 0, ev


def test_the_input_bites():
    """Conditions on the main GPU test's input, not measurements: the oracle's traces clear each by more
    than 2 x (55,986 partial fills, 322,008 partial empties, 131,867 refused charges, 742 chains with loss)."""
    pv, meter, cov, status = _a()
    a_has_teeth(pv, cov, status)
    ev = events(pv, meter, cov, PARAMS, SOC0)
    print(ev)
    assert ev["partial_fill"] >= 20000 and ev["partial_empty"] >= 100000 and ev["refused"] >= 50000
    assert ev["loss_chains"] >= 500 and ev["standby_clip"] > 0


def test_lossless_gives_the_storage_table():
    pv, meter, cov, _ = _a()
    bat = storage_battery(A_BATTERY)
    par = uniform(A_N, bat["capacity"], bat["p_charge"], bat["p_discharge"])
    raw, end = battery.from_traces(pv, meter, cov, 900, params=par, soc0=bat["soc0"])
    want, wend = storage.from_traces(pv, meter, cov, 900, **bat)
    np.testing.assert_array_equal(raw[:, :9], want)
    np.testing.assert_array_equal(end, wend)
    assert not raw[:, 9].any() and (want[:, 6] > 0).any() and (want[:, 7] > 0).any()


def test_identities(a_table):
    raw, end, _ = a_table
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7])
    assert (raw[:, 4:8] >= 0).all() and (raw[:, 9] >= 0).all()
    soc, off = battery.unpack_soc(raw[:, 8])
    has = off >= 0
    np.testing.assert_array_equal(has, raw[:, 2] > 0)
    prev = SOC0.copy()                                         # [6] - [7] - [9] is the interval's SoC change
    for k in range(raw.shape[0]):
        now = np.where(has[k], soc[k], prev)
        np.testing.assert_array_equal(raw[k, 6] - raw[k, 7] - raw[k, 9], now - prev)
        prev = now
    np.testing.assert_array_equal(prev, end)
    assert ((soc >= 0) & (soc <= PARAMS[0])).all() and ((end >= 0) & (end <= PARAMS[0])).all()
    pv, meter, cov, _ = _a()
    np.testing.assert_array_equal(raw[:, :4], intervals.from_traces(pv, meter, cov, 900))
    assert (raw[:, 6] > 0).any() and (raw[:, 7] > 0).any() and (raw[:, 5] > 0).any()
    # no battery: the SoC stays 0 and nothing is discharged; an ask of one unit that stores floor(ec / 2^16) = 0 is
    # "not clipped" (g == s == 0), so b = a = 1 is charged and lost at once: at most one unit per ok second
    none = PARAMS[0] == 0
    assert none.sum() > 100 and not soc[:, none].any() and not raw[:, 7, none].any()
    np.testing.assert_array_equal(raw[:, 6, none], raw[:, 9, none])
    assert (raw[:, 6, none] <= raw[:, 2, none]).all()
    assert int((raw[:, 9].sum(axis=0) > 0).sum()) >= 500


def test_blocks_of_128_chain_to_the_sequential_soc(a_table):
    """What the engine does: each 128-second block's per-second maps (per-chain parameters) folded into one
    triple, the blocks' triples applied in order from soc0 -- every block's start is the sequential SoC."""
    pv, meter, cov, _ = _a()
    a, lo, hi = battery.second_maps(pv, meter, cov, params=PARAMS)
    nblk = -(-A_STEPS // 128)
    x = SOC0.copy()
    seq = x.copy()
    for b in range(nblk):
        f = tuple(np.full(A_N, v, dtype=np.int64) for v in storage.IDENTITY)
        for s in range(128 * b, min(128 * b + 128, A_STEPS)):
            f = storage.compose(f, (a[s], lo[s], hi[s]))
            seq = storage.apply((a[s], lo[s], hi[s]), seq)
        assert (np.abs(f[0]) < 1 << 36).all()
        x = storage.apply(f, x)
        np.testing.assert_array_equal(x, seq, err_msg=f"after block {b}")
    np.testing.assert_array_equal(x, a_table[1])


def test_windows_carry_the_soc(a_table):
    raw, end, _ = a_table
    pv, meter, cov, _ = _a()
    x = SOC0
    acc = np.zeros_like(raw)
    done = 0
    for w in (5001, 5802):                                     # a window edge inside an interval
        part, x = battery.from_traces(pv[done:done + w], meter[done:done + w], cov[done:done + w], 900, soc0=x,
                                      origin=done, params=PARAMS)
        rows = part.shape[0]
        acc[:rows, :8] += part[:, :8]
        acc[:rows, 8] = np.maximum(acc[:rows, 8], part[:, 8])
        acc[:rows, 9] += part[:, 9]
        done += w
    assert done == A_STEPS
    np.testing.assert_array_equal(acc, raw)
    np.testing.assert_array_equal(x, end)


def test_soc_above_capacity_is_clamped():
    pv, meter, cov, _ = _a()
    sub = [a[4000:5000, :60] for a in (pv, meter, cov)]
    par = PARAMS[:, :60]
    raw, end = battery.from_traces(*sub, 900, params=par, soc0=par[0] + 12345)
    want, wend = battery.from_traces(*sub, 900, params=par, soc0=par[0])
    np.testing.assert_array_equal(raw, want)
    np.testing.assert_array_equal(end, wend)
    with pytest.raises(ValueError):
        battery.from_traces(*sub, 900, params=par[:, :59], soc0=0)
    with pytest.raises(ValueError):
        battery.from_traces(*sub, 1 << 23, params=par, soc0=0)


def test_to_watts(a_table):
    raw, _, _ = a_table
    w = battery.to_watts(raw, 900, n_steps=A_STEPS)
    base = storage.to_watts(raw[:, :9], 900)
    for key in base:
        np.testing.assert_array_equal(w[key], base[key])
    assert set(w) - set(base) == {"energy_wh_loss", "round_trip"}
    e = 3600.0 * 2 ** K
    np.testing.assert_array_equal(w["energy_wh_loss"], raw[:, 9] / e)
    dsoc = raw[:, 6] - raw[:, 7] - raw[:, 9]
    den = raw[:, 6] - dsoc
    np.testing.assert_array_equal(np.isnan(w["round_trip"]), den == 0)
    np.testing.assert_array_equal(w["round_trip"][den != 0], raw[:, 7][den != 0] / den[den != 0].astype(np.float64))
    rt = w["round_trip"][den != 0]
    assert ((rt >= 0) & (rt <= 1)).all() and (rt < 1).any() and (rt > 0.5).any()
    assert (den == 0).any() and (den != 0).any()
    assert battery.to_registers(raw).shape == (13, 6, A_N)
    with pytest.raises(ValueError):
        battery.to_watts(raw[:, :9], 900)
    with pytest.raises(ValueError):
        battery.to_watts(raw, 900, n_steps=A_STEPS + 900)


def test_abi_sizes_and_setter_refusals():
    """Host-side only: the struct and what tmh_set_battery refuses before it touches an engine."""
    L = _lib.load()
    assert "tmh_set_battery" in _lib.EXPORTS and L.tmh_abi_version() == 1
    assert C.sizeof(_lib.Battery) == C.sizeof(_lib.Intervals) + 4 * 8
    assert _lib.Battery.table.offset == 0 and _lib.Battery.soc.offset == C.sizeof(_lib.Intervals)
    assert _lib.Battery.params.offset == C.sizeof(_lib.Intervals) + 24
    assert C.sizeof(_lib.Storage) == C.sizeof(_lib.Intervals) + 6 * 8           # storage's ABI as it was
    assert L.tmh_storage_work_bytes(1000, 129) == 2 * 1000 * 24
    assert L.tmh_scratch_bytes(4096, 86400) == 155575808                        # unchanged by the kind
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    good = dict(table=_lib.Intervals(p, 0, 500, 60, 4), soc=p, work=p, work_bytes=512, params=p)

    def refused(word, **kw):
        bt = _lib.Battery(**{**good, **kw})
        assert L.tmh_set_battery(None, C.byref(bt)) == -1
        msg = L.tmh_last_error().decode()
        assert "battery" in msg and word in msg, msg

    refused("buffer", table=_lib.Intervals(None, 0, 500, 60, 4))
    refused("8-byte aligned", table=_lib.Intervals(p + 4, 0, 500, 60, 4))
    refused("interval_s", table=_lib.Intervals(p, 0, 500, 0, 4))
    refused("n_steps", table=_lib.Intervals(p, 0, 0, 60, 4))
    refused("ld", table=_lib.Intervals(p, 0, 500, 60, 0))
    refused("2^23", table=_lib.Intervals(p, 0, 500, 1 << 23, 4))
    refused("soc", soc=None)
    refused("soc", soc=p + 4)
    refused("work", work=None)
    refused("work", work=p + 2)
    refused("params", params=None)
    refused("params", params=p + 4)
    assert L.tmh_set_battery(None, C.byref(_lib.Battery(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_battery(None, None) == -1
