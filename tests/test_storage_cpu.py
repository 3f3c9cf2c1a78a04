"""Battery storage without a GPU: the contract in numpy (tmhpvsim_amd.storage) against a scalar pure-Python
loop on the oracle's traces of base input A with a 60-module system, the algebra of clamped additions the
engine's map pass and scan rest on (compose, apply), the table's identities, and the C-ABI's struct,
sizes and setter."""
import ctypes as C
import os

import numpy as np
import pytest

from series_util import A_N, A_STEPS, a_has_teeth
from storage_util import A_BATTERY, a60_oracle, battery, events
from tmhpvsim_amd import _lib, intervals, registers, series, storage

K = storage.FRAC_BITS
BAT = battery(A_BATTERY)


def _a():
    ref = a60_oracle()
    return ref["pv"], ref["meter"], ref["covered"], ref["status"]


def test_units_columns_and_params():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "tmhpvsim.h")).read()
    assert "#define TMH_OUT_STORAGE 7" in hdr and _lib.OUT_STORAGE == 7
    assert "#define TMH_STORAGE_COLS 9" in hdr and len(storage.COLUMNS) == 9
    assert (K, storage.MAX_W) == (series.FRAC_BITS, series.MAX_W)
    assert storage.COLUMNS[:4] == intervals.COLUMNS
    assert storage.COLUMNS[4:] == ("import", "export", "charge", "discharge", "soc_key")
    assert [storage.n_intervals(s, 900) for s in (0, 1, 900, 901, A_STEPS)] == [0, 1, 1, 2, 13]
    assert storage.quantize_params(0.5, 1000.0, 3000.0, 0.25) == (7372800, 1000 << K, 3000 << K, 3686400)
    assert storage.quantize_params(0.05, 300.0, 2000.0, 0.025)[0] == 737280
    assert storage.quantize_params(0.0, 0.0, 0.0) == (0, 0, 0, 0)
    for bad in ((-1.0, 1.0, 1.0), (2.0 ** 40 / 3600 / 2 ** K, 1.0, 1.0), (1.0, 2.0 ** 27 / 2 ** K + 1, 1.0), (1.0, 1.0, -1.0)):
        with pytest.raises(ValueError):
            storage.quantize_params(*bad)
    assert storage.IDENTITY == (0, -(1 << 62), (1 << 62) - 1)
    assert C.sizeof(_lib.Storage) == C.sizeof(_lib.Intervals) + 3 * 8 + 3 * 8
    assert _lib.Storage.table.offset == 0 and _lib.Storage.soc.offset == C.sizeof(_lib.Intervals)


def _loop(pv, meter, cov, interval_s, origin, chains, capacity, p_charge, p_discharge, soc0):
    """The contract as a plain per-chain, per-second loop (Python integers)."""
    n_steps = pv.shape[0]
    out = np.zeros((-(-(origin + n_steps) // interval_s), 9, len(chains)), dtype=np.int64)
    end = []
    for c, i in enumerate(chains):
        x = int(soc0)
        for s in range(n_steps):
            if np.isnan(pv[s, i]) or np.isnan(meter[s, i]) or cov[s, i] == 255:
                continue
            k, o = divmod(origin + s, interval_s)
            qp = round(float(pv[s, i]) * 2 ** K)       # Python's round: half to even
            qm = round(float(meter[s, i]) * 2 ** K)
            d = qp - qm
            a = min(max(d, -p_discharge), p_charge)
            xn = min(max(x + a, 0), capacity)
            g = xn - x
            x = xn
            out[k, 0, c] += qp
            out[k, 1, c] += qm
            out[k, 2, c] += 1
            out[k, 3, c] += int(cov[s, i] == 1)
            out[k, 4, c] += max(g - d, 0)
            out[k, 5, c] += max(d - g, 0)
            out[k, 6, c] += max(g, 0)
            out[k, 7, c] += max(-g, 0)
            out[k, 8, c] = max(int(out[k, 8, c]), ((o + 1) << 40) | xn)
        end.append(x)
    return out, np.array(end, dtype=np.int64)


def _slice_chains(cov, status):
    """A small slice of A: chains dead at construction, the chains that fault inside the window, live ones."""
    dead = np.flatnonzero(status == 1)[:2]
    faulted = np.flatnonzero((cov[-1] == 255) & (cov[0] != 255))
    live = np.flatnonzero(cov[-1] != 255)[:3]
    return [int(i) for i in np.r_[dead, faulted, live]]


@pytest.mark.parametrize("interval_s,origin", [(900, 0), (7, 0), (60, 17)])
def test_from_traces_against_the_scalar_loop(interval_s, origin):
    pv, meter, cov, status = _a()
    chains = _slice_chains(cov, status)
    lo, hi = 4000, 7000                                  # morning: empty, charging, full, clipped
    sub = [a[lo:hi][:, chains] for a in (pv, meter, cov)]
    got, end = storage.from_traces(*sub, interval_s, origin=origin, **BAT)
    want, wend = _loop(*sub, interval_s, origin, range(len(chains)), **BAT)
    assert got.dtype == np.int64 and got.shape == want.shape
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(end, wend)
    assert (got[:, 6].sum(axis=0) > 0).any() and (got[:, 7].sum(axis=0) > 0).any()


def test_the_input_bites():
    """The oracle's counts of the main GPU test's input (tests/test_gpu_storage.py asserts about half)."""
    pv, meter, cov, status = _a()
    a_has_teeth(pv, cov, status)
    ev = events(pv, meter, cov, **BAT)
    print(ev)
    assert ev == dict(full=40686, empty=9956067, inside=536920, charge_limit=174532, discharge_limit=6493506, both=967)
    assert int((status == 1).sum()) == 24 and int(((cov[-1] == 255) & (cov[0] != 255)).sum()) == 4


def _random_triples(rng, m, cap):
    """Triples with lo <= hi: per-second ones, the identity, saturated ones (lo == hi), wide ones."""
    a = rng.integers(-(1 << 34), 1 << 34, m)
    lo = rng.integers(0, cap + 1, m)
    hi = lo + rng.integers(0, cap + 1, m)
    kind = rng.integers(0, 4, m)
    lo = np.where(kind == 0, storage.LO, np.where(kind == 1, 0, lo))
    hi = np.where(kind == 0, storage.HI, np.where(kind == 1, cap, np.where(kind == 2, lo, hi)))
    a = np.where(kind == 0, 0, a)
    return a.astype(np.int64), lo.astype(np.int64), hi.astype(np.int64)


def test_compose_is_associative_and_applies_in_order():
    rng = np.random.default_rng(0x50C)
    m, cap = 20000, BAT["capacity"]
    f, g, h = (_random_triples(rng, m, cap) for _ in range(3))
    x = np.r_[rng.integers(-4 * cap, 5 * cap, m - 4), [0, cap, -1, cap + 1]].astype(np.int64)   # starts outside [0, C] too
    fg = storage.compose(f, g)
    for u, v in zip(storage.compose(fg, h), storage.compose(f, storage.compose(g, h))):
        np.testing.assert_array_equal(u, v)
    np.testing.assert_array_equal(storage.apply(fg, x), storage.apply(g, storage.apply(f, x)))
    np.testing.assert_array_equal(storage.apply(storage.compose(fg, h), x),
                                  storage.apply(h, storage.apply(g, storage.apply(f, x))))
    ident = tuple(np.full(m, v, dtype=np.int64) for v in storage.IDENTITY)
    for u, v, w in zip(storage.compose(f, ident), storage.compose(ident, f), f):
        np.testing.assert_array_equal(u, w)
        np.testing.assert_array_equal(v, w)
    np.testing.assert_array_equal(storage.apply(ident, x), x)
    assert [int(v) for v in storage.compose((5, 0, 10), (-7, 0, 10))] == [-2, 0, 3]
    assert int(storage.apply((5, 0, 10), 7)) == 10 and int(storage.apply((-7, 0, 10), 10)) == 3


def test_blocks_of_128_chain_to_the_sequential_soc():
    """What the engine does: each 128-second block's per-second maps folded into one triple, the blocks'
    triples applied in order from soc0 -- every block's start equals the sequential loop's SoC there."""
    pv, meter, cov, _ = _a()
    par = {k: v for k, v in BAT.items() if k != "soc0"}
    a, lo, hi = storage.second_maps(pv, meter, cov, **par)
    nblk = -(-A_STEPS // 128)
    x = np.full(A_N, BAT["soc0"], dtype=np.int64)
    seq = x.copy()
    for b in range(nblk):
        f = tuple(np.full(A_N, v, dtype=np.int64) for v in storage.IDENTITY)
        for s in range(128 * b, min(128 * b + 128, A_STEPS)):
            f = storage.compose(f, (a[s], lo[s], hi[s]))
            seq = storage.apply((a[s], lo[s], hi[s]), seq)
        assert (np.abs(f[0]) <= 128 << 27).all()
        x = storage.apply(f, x)
        np.testing.assert_array_equal(x, seq, err_msg=f"after block {b}")
    _, end = storage.from_traces(pv[:, :50], meter[:, :50], cov[:, :50], 900, **BAT)
    np.testing.assert_array_equal(x[:50], end)


@pytest.fixture(scope="module")
def a_table():
    pv, meter, cov, status = _a()
    return storage.from_traces(pv, meter, cov, 900, **BAT) + (status,)


def test_identities(a_table):
    raw, end, _ = a_table
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7])
    assert (raw[:, 4:8] >= 0).all()
    soc, off = storage.unpack_soc(raw[:, 8])
    has = off >= 0
    np.testing.assert_array_equal(has, raw[:, 2] > 0)
    prev = np.full(A_N, BAT["soc0"], dtype=np.int64)          # [6] - [7] is the interval's SoC change
    for k in range(raw.shape[0]):
        now = np.where(has[k], soc[k], prev)
        np.testing.assert_array_equal(raw[k, 6] - raw[k, 7], now - prev)
        prev = now
    np.testing.assert_array_equal(prev, end)
    pv, meter, cov, _ = _a()
    np.testing.assert_array_equal(raw[:, :4], intervals.from_traces(pv, meter, cov, 900))
    assert (raw[:, 6] > 0).any() and (raw[:, 7] > 0).any() and (raw[:, 5] > 0).any()


def test_no_battery_gives_the_registers():
    pv, meter, cov, _ = _a()
    sub = [a[:, :120] for a in (pv, meter, cov)]
    rg = registers.from_traces(*sub, 900)
    for par, soc0 in ((dict(capacity=0, p_charge=1000 << K, p_discharge=3000 << K), 0),
                      (dict(capacity=3600 << K, p_charge=0, p_discharge=0), 12345)):
        raw, end = storage.from_traces(*sub, 900, soc0=soc0, **par)
        np.testing.assert_array_equal(raw[:, :6], rg)
        assert not raw[:, 6:8].any() and (end == soc0).all()
        soc, off = storage.unpack_soc(raw[:, 8])
        np.testing.assert_array_equal(soc, np.where(off >= 0, soc0, 0))
    assert (rg[:, 5] > 0).any()


def test_windows_carry_the_soc(a_table):
    raw, end, _ = a_table
    pv, meter, cov, _ = _a()
    par = {k: v for k, v in BAT.items() if k != "soc0"}
    x = BAT["soc0"]
    acc = np.zeros_like(raw)
    done = 0
    for w in (5001, 37, 5765):                               # window edges inside intervals
        part, x = storage.from_traces(pv[done:done + w], meter[done:done + w], cov[done:done + w], 900, soc0=x,
                                      origin=done, **par)
        acc[:part.shape[0], :8] += part[:, :8]
        acc[:part.shape[0], 8] = np.maximum(acc[:part.shape[0], 8], part[:, 8])
        done += w
    np.testing.assert_array_equal(acc, raw)
    np.testing.assert_array_equal(x, end)


def test_the_soc_key(a_table):
    raw, end, status = a_table
    pv, meter, cov, _ = _a()
    soc, off = storage.unpack_soc(raw[:, 8])
    ok = cov != 255
    dead = status == 1
    assert dead.sum() >= 10 and not raw[:, :, dead].any() and (off[:, dead] == -1).all() and (end[dead] == BAT["soc0"]).all()
    faulted = np.flatnonzero((cov[-1] == 255) & ~dead)
    assert len(faulted) == 4
    for i in faulted:                                           # the key of the fault's interval: the last ok second
        last = int(np.flatnonzero(ok[:, i])[-1])
        k = last // 900
        assert off[k, i] == last - 900 * k and (off[k + 1:, i] == -1).all() and not raw[k + 1:, :, i].any()
        _, x = storage.from_traces(pv[:last + 1, i:i + 1], meter[:last + 1, i:i + 1], cov[:last + 1, i:i + 1], 900, **BAT)
        assert soc[k, i] == x[0] == end[i]
    live = ~dead & (cov[-1] != 255)
    assert (off[:12, live] == 899).all() and (off[12, live] == 2).all()      # full intervals, the last partial one
    np.testing.assert_array_equal(soc[12, live], end[live])
    assert ((soc >= 0) & (soc <= BAT["capacity"])).all()


def test_partial_first_and_last_intervals():
    pv, meter, cov, _ = _a()
    sub = [a[4000:4000 + 2405, :40] for a in (pv, meter, cov)]
    raw, _ = storage.from_traces(*sub, 900, origin=3, **BAT)
    assert raw.shape == (-(-(2405 + 3) // 900), 9, 40)
    live = raw[2, 2] > 0
    assert live.any() and (raw[0, 2, live] == 897).all() and (raw[2, 2, live] == 2408 - 1800).all()
    _, off = storage.unpack_soc(raw[:, 8])
    assert (off[0, live] == 899).all() and (off[2, live] == 2408 - 1800 - 1).all()
    with pytest.raises(ValueError):
        storage.from_traces(*sub, 1 << 23, **BAT)
    with pytest.raises(ValueError):
        storage.from_traces(*sub, 900, capacity=1 << 40, p_charge=0, p_discharge=0, soc0=0)


def test_to_watts(a_table):
    raw, _, _ = a_table
    w = storage.to_watts(raw, 900, n_steps=A_STEPS)
    base = intervals.to_watts(raw[:, :4], 900)
    for key in base:
        np.testing.assert_array_equal(w[key], base[key])
    e = 3600.0 * 2 ** K
    np.testing.assert_array_equal(w["energy_wh_import"], raw[:, 4] / e)
    np.testing.assert_array_equal(w["energy_wh_discharge"], raw[:, 7] / e)
    soc, off = storage.unpack_soc(raw[:, 8])
    np.testing.assert_array_equal(np.isnan(w["soc_wh"]), off < 0)
    assert np.nanmax(w["soc_wh"]) == 0.5 and np.nanmin(w["soc_wh"]) == 0.0
    ss = w["self_sufficiency"][np.isfinite(w["self_sufficiency"])]
    assert ((ss >= 0) & (ss <= 1)).all() and (ss > 0).any()
    assert storage.to_registers(raw).shape == (13, 6, A_N)
    with pytest.raises(ValueError):
        storage.to_watts(raw[:, :8], 900)
    with pytest.raises(ValueError):
        storage.to_watts(raw, 900, n_steps=A_STEPS + 900)


def test_abi_sizes_and_setter_refusals():
    """Host-side only: tmh_storage_work_bytes and what tmh_set_storage refuses before it touches an engine."""
    L = _lib.load()
    assert L.tmh_storage_work_bytes(1000, 128) == 1000 * 24 and L.tmh_storage_work_bytes(1000, 129) == 2 * 1000 * 24
    assert L.tmh_storage_work_bytes(16384, 2592000) == 20250 * 16384 * 24
    assert L.tmh_scratch_bytes(4096, 86400) == 155575808                    # unchanged by the kind
    buf = np.zeros(64, dtype=np.int64)
    p = buf.ctypes.data
    good = dict(table=_lib.Intervals(p, 0, 500, 60, 4), soc=p, work=p, work_bytes=512, capacity=100, p_charge=5, p_discharge=5)

    def refused(word, **kw):
        st = _lib.Storage(**{**good, **kw})
        assert L.tmh_set_storage(None, C.byref(st)) == -1
        msg = L.tmh_last_error().decode()
        assert "storage" in msg and word in msg, msg

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
    refused("capacity", capacity=-1)
    refused("capacity", capacity=1 << 40)
    refused("p_charge", p_charge=(1 << 27) + 1)
    refused("p_charge", p_discharge=-1)
    assert L.tmh_set_storage(None, C.byref(_lib.Storage(**good))) == -1 and b"NULL engine" in L.tmh_last_error()
    assert L.tmh_set_storage(None, None) == -1
