"""Battery storage on the GPU (tmh_set_storage, BatchedSim.enable_storage; fp64 throughout): integers, so
every comparison with the traces' table (storage.from_traces, a plain loop over the seconds) is bit for bit.
The expected table and the expected state of charge always come from traces of separate sims of the same
chains (pv / meter / residual through OUT_TRACE3, covered through OUT_ANY), never from the kernels under
test."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, C_BATTERY, battery, events, modules_params
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _kw, _run_windows
from test_gpu_series import _last, _np, _sim, _traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IV = 900
PREC = "fp64"


def _kw60(steps=A_STEPS):
    return _kw(PREC, steps, mp=modules_params())


def _identities(raw):
    """[4] - [5] == [1] - [0] + [6] - [7], columns 4-7 >= 0, a key iff the cell has an ok second."""
    from tmhpvsim_amd import storage
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7])
    assert (raw[:, 4:8] >= 0).all()
    np.testing.assert_array_equal(storage.unpack_soc(raw[:, 8])[1] >= 0, raw[:, 2] > 0)


def _soc_changes(raw, soc0, end):
    """[6] - [7] is each interval's change of the state of charge, from soc0 to the state after the run."""
    from tmhpvsim_amd import storage
    soc, off = storage.unpack_soc(raw[:, 8])
    prev = np.full(raw.shape[2], soc0, dtype=np.int64)
    for k in range(raw.shape[0]):
        now = np.where(off[k] >= 0, soc[k], prev)
        np.testing.assert_array_equal(raw[k, 6] - raw[k, 7], now - prev, err_msg=f"interval {k}")
        prev = now
    np.testing.assert_array_equal(prev, end)


@functools.lru_cache(maxsize=None)
def a60_gpu():
    """Input A with 60 modules: the fp64 traces of separate sims, the expected table and end state."""
    from tmhpvsim_amd import storage
    pv, meter, cov = _traces((_sim(A_N, A_START, **_kw60()), _sim(A_N, A_START, **_kw60())), A_WINDOWS)
    for a in (pv, meter, cov):
        a.setflags(write=False)
    want, end = storage.from_traces(pv, meter, cov, IV, **battery(A_BATTERY))
    return dict(pv=pv, meter=meter, cov=cov, want=want, end=end)


@functools.lru_cache(maxsize=None)
def a_st():
    """The storage sim of input A, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = sim.enable_storage(A_STEPS, IV, **A_BATTERY)
    assert tuple(raw.shape) == (13, 9, A_N) and tuple(sim.soc.shape) == (A_N,) and sim.soc.dtype == torch.int64
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def test_storage_equals_the_traces_table():
    """The main test: all nine columns and the state of charge bit for bit, over two windows (the second off
    the four-step grid), chains faulted at construction and inside the window, night and day, a battery
    that runs empty, fills, clips at both bounds and meets both power limits."""
    from tmhpvsim_amd import _lib
    g, t = a_st(), a60_gpu()
    bat = battery(A_BATTERY)
    assert (bat["capacity"], bat["soc0"]) == (7372800, 3686400)
    a_has_teeth(t["pv"], t["cov"], g["status"])
    ev = events(t["pv"], t["meter"], t["cov"], **bat)
    dead = g["status"] == 1
    print(ev, "dead at construction", int(dead.sum()), "in-window faults", int(((t["cov"][-1] == 255) & ~dead).sum()))
    assert ev["full"] >= 20000 and ev["empty"] >= 5000000 and ev["inside"] >= 250000
    assert ev["charge_limit"] >= 80000 and ev["discharge_limit"] >= 3000000 and ev["both"] >= 500
    assert g["variants"] == [_lib.OUT_STORAGE | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(9):
        np.testing.assert_array_equal(g["raw"][:, col], t["want"][:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(g["soc"], t["end"])
    assert not g["raw"][:, :, dead].any() and (g["soc"][dead] == bat["soc0"]).all()
    _identities(g["raw"])
    _soc_changes(g["raw"], bat["soc0"], g["soc"])
    assert g["raw"][12, 2].max() == 3 and g["raw"][:12, 2].max() == IV          # the last partial interval


def test_windows_pipelining_and_compaction_same_bits():
    """One tmh_run per window (a_st), one pipelined run over windows of 4,000 steps, and compacted
    windows of 3,601 steps (from the second window on only the live chains run, in dense slots: a slot's
    work column is the slot's, its soc and table column the chain's): the same table and end state."""
    g, t = a_st(), a60_gpu()
    pipe = _sim(A_N, A_START, **_kw60())
    rawp = pipe.enable_storage(A_STEPS, IV, **A_BATTERY)
    pipe.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(rawp), t["want"])
    np.testing.assert_array_equal(_np(pipe.soc), t["end"])
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_storage(A_STEPS, IV, **A_BATTERY)
    sim.run(A_STEPS, trace=(), window=3601, compact=True)
    torch.cuda.synchronize()
    assert len(sim.compact_slots) == 3 and sim.compact_slots[0] == A_N
    assert min(sim.compact_slots) < A_N, sim.compact_slots        # a window ran on fewer slots than chains
    assert sim.compact_slots[2] < sim.compact_slots[1]            # (A's in-window faults)
    np.testing.assert_array_equal(_np(raw), g["raw"])
    np.testing.assert_array_equal(_np(raw), t["want"])
    np.testing.assert_array_equal(_np(sim.soc), t["end"])
    np.testing.assert_array_equal(sim.status(), g["status"])


@functools.lru_cache(maxsize=None)
def c60_traces(n):
    """Input C with 60 modules: n chains, 2,405 steps from 06:58 across sunrise, as windows 1100 + 1305."""
    kw = _kw60(C_STEPS)
    pv, meter, cov = _traces((_sim(n, C_START, **kw), _sim(n, C_START, **kw)), C_WINDOWS)
    for a in (pv, meter, cov):
        a.setflags(write=False)
    return pv, meter, cov


@pytest.mark.parametrize("interval_s", [7, 60, 128, 900])
@pytest.mark.parametrize("n", [1300, 64])
def test_storage_boundaries(n, interval_s):
    """Boundaries inside four-second groups (7), several in a 128-s block (60), one per block (128),
    partial first and last intervals (900); the origin three steps before the run, so no interval edge
    coincides with a window edge; a partial wavefront and construction faults; a small battery that
    fills after sunrise."""
    from tmhpvsim_amd import _lib, storage
    pv, meter, cov = c60_traces(n)
    bat = battery(C_BATTERY)
    assert bat["capacity"] == 737280 and bat["soc0"] == 368640
    night_rows = int((np.nan_to_num(pv).max(axis=1) == 0).sum())
    ev = events(pv, meter, cov, **bat)
    print(f"n {n}: {ev}, construction faults {int((cov[0] == 255).sum())}, night rows {night_rows}")
    assert night_rows > 0 and (np.nan_to_num(pv) > 0).any()                                # night and daylight
    assert ev["full"] >= 800 and ev["inside"] >= 800 and ev["charge_limit"] >= 400
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = sim.enable_storage(C_STEPS + C_LEAD, interval_s, step0=-C_LEAD, **C_BATTERY)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_STORAGE | _lib.OUT_FP64
    torch.cuda.synchronize()
    want, end = storage.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, **bat)
    assert tuple(raw.shape) == want.shape == (-(-(C_STEPS + C_LEAD) // interval_s), 9, n)
    for w0 in np.cumsum((0,) + C_WINDOWS)[:-1]:                   # where a window begins (and the one before it ends)
        assert (int(w0) + C_LEAD) % interval_s != 0
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    _identities(_np(raw))
    _soc_changes(_np(raw), bat["soc0"], _np(sim.soc))
    live0 = want[0, 2] == interval_s - C_LEAD                     # the first cell begins at offset C_LEAD
    assert live0.any()
    np.testing.assert_array_equal(storage.unpack_soc(_np(raw)[0, 8, live0])[1], interval_s - 1)


def test_no_battery_gives_the_registers():
    """Capacity 0, then no power with a capacity of 1 Wh: columns 0-5 are a registers sim's table, nothing
    is charged or discharged, and the key holds 0 or the untouched soc0."""
    from tmhpvsim_amd import _lib, storage
    rgs = _sim(A_N, A_START, **_kw60())
    rg = rgs.enable_registers(A_STEPS, IV)
    _run_windows(rgs, A_WINDOWS)
    assert _last(rgs) == _lib.OUT_REGISTERS | _lib.OUT_FP64 and int((rg[:, 5] > 0).sum()) > 1000
    for spec, soc0 in ((dict(capacity_wh=0.0, charge_w=1000.0, discharge_w=3000.0, soc0_wh=0.0), 0),
                       (dict(capacity_wh=1.0, charge_w=0.0, discharge_w=0.0, soc0_wh=0.5), 7372800)):
        sim = _sim(A_N, A_START, **_kw60())
        raw = sim.enable_storage(A_STEPS, IV, **spec)
        _run_windows(sim, A_WINDOWS)
        got = _np(raw)
        np.testing.assert_array_equal(got[:, :6], _np(rg))
        assert not got[:, 6:8].any()
        soc, off = storage.unpack_soc(got[:, 8])
        np.testing.assert_array_equal(off >= 0, got[:, 2] > 0)
        np.testing.assert_array_equal(soc, np.where(off >= 0, soc0, 0))
        assert (_np(sim.soc) == soc0).all()


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_storage(spec):
    """Statistics beside the storage table are the statistics-only run's, bit for bit (the map pass adds
    nothing to them), and the table is the storage-only one."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    both, stats, alone = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = both.enable_storage(steps, 600, **A_BATTERY), alone.enable_storage(steps, 600, **A_BATTERY)
    for s in (both, stats, alone):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_STORAGE | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[:, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    assert int(ra[:, 6].sum()) > 0 and int(ra[:, 7].sum()) > 0
    _identities(_np(ra))


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_storage_per_chain_sites(spec):
    """The per-chain-sites kernels (map and replay), with statistics beside the table."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib, storage
    import dataclasses
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    mp = dataclasses.replace(modules_params(), cc_mode=ModelParams().cc_mode, seed=0x51E)
    sim = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    raw = sim.enable_storage(steps + 1, 450, step0=-1, **A_BATTERY)
    stats = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    for s in (sim, stats):
        s.enable_stats(**HISTS[spec])
    stats.run(steps, trace=(), window=1700)
    assert _last(stats) & 7 == _lib.OUT_STATS
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_STORAGE | _lib.OUT_SITES | _lib.OUT_FP64
    tr = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = storage.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1, **battery(A_BATTERY))
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0
    assert int(stats.hist.sum()) == int(raw[:, 2].sum()) > 0
    assert torch.equal(sim.hist, stats.hist)
    assert torch.equal(sim.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))


def test_two_batches_fill_one_table():
    """Chains [5000, 5512) and [5512, 6000) as two sims writing column slices of one table and one soc."""
    bat = battery(A_BATTERY)
    big = torch.zeros(13, 9, A_N, dtype=torch.int64, device="cuda:0")
    soc = torch.full((A_N,), bat["soc0"], dtype=torch.int64, device="cuda:0")
    for a, b in ((0, 512), (512, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_storage(A_STEPS, IV, buffer=view, soc=soc[a:b], **A_BATTERY)
        assert got is view and s._storage.ld == A_N and s.soc.data_ptr() == soc[a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), a60_gpu()["want"])
    np.testing.assert_array_equal(_np(soc), a60_gpu()["end"])
    with pytest.raises(ValueError, match="strides"):
        s.enable_storage(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2], **A_BATTERY)     # chains not contiguous
    with pytest.raises(ValueError, match="storage buffer"):
        s.enable_storage(A_STEPS, IV, buffer=torch.zeros(13, 8, s.n, dtype=torch.int64, device="cuda:0"), **A_BATTERY)
    with pytest.raises(ValueError, match="soc"):
        s.enable_storage(A_STEPS, IV, soc=soc[:2 * s.n:2], **A_BATTERY)
    s.enable_storage(None)
    assert s.soc is None and s.storage_raw is None


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message before anything is launched: the chains' state
    and the batteries' stay as they were and the table all zeros."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    bat = battery(A_BATTERY)

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool(sim.storage_raw.any())

    def desc(sim, **kw):
        """The sim's tmh_storage with fields replaced."""
        d = sim._storage_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, capacity=d.capacity,
                 p_charge=d.p_charge, p_discharge=d.p_discharge)
        return _lib.Storage(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    sim.enable_storage(500, 60, **A_BATTERY)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "storage tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # storage, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_storage(None)
    sim.enable_series(500)                                                 # a fleet series, then storage
    with pytest.raises(ValueError, match="fleet series"):
        sim.enable_storage(500, 60, **A_BATTERY)
    sim.enable_series(None)
    sim.enable_storage(500, 60, **A_BATTERY)
    refused(sim, "outside the storage", step0=0, k=501)                    # past the end
    refused(sim, "outside the storage", step0=450, k=100)
    sim.enable_storage(500, 60, step0=10, **A_BATTERY)
    refused(sim, "outside the storage", step0=0, k=100)                    # before the origin
    buf = sim.enable_storage(500, 60, **A_BATTERY)
    _lib.check(L.tmh_set_storage(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "storage tables ld")                                      # ld too small
    _lib.check(L.tmh_set_storage(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_storage_work_bytes(n, 100) - 8))))
    refused(sim, "work buffer too small")
    tb = sim._storage
    p = buf.data_ptr()
    for kw, word in ((dict(table=_lib.Intervals(p + 4, 0, 500, 60, n)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(None, 0, 500, 60, n)), b"buffer"),
                     (dict(table=_lib.Intervals(p, 0, 500, 0, n)), b"interval_s"),
                     (dict(table=_lib.Intervals(p, 0, 0, 60, n)), b"n_steps"),
                     (dict(table=_lib.Intervals(p, 0, 500, 60, 0)), b"ld"),
                     (dict(table=_lib.Intervals(p, 0, 500, 1 << 23, n)), b"2^23"),
                     (dict(soc=None), b"soc"), (dict(soc=sim.soc.data_ptr() + 4), b"soc"),
                     (dict(work=None), b"work"), (dict(work=p + 4), b"work"),
                     (dict(capacity=-1), b"capacity"), (dict(capacity=1 << 40), b"capacity"),
                     (dict(p_charge=(1 << 27) + 1), b"p_charge"), (dict(p_discharge=-1), b"p_discharge")):
        assert L.tmh_set_storage(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"storage" in L.tmh_last_error()                            # the setter refuses a bad struct
    # storage with another table kind on one engine, set in either order
    sim.enable_storage(500, 60, **A_BATTERY)
    for kind, cols, word in (("intervals", 4, "battery storage and interval metering"),
                             ("registers", 6, "battery storage and the import / export registers"),
                             ("demand", 8, "battery storage and the demand registers")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(_lib.Intervals(other.data_ptr(), 0, 500, 60, n))))
        refused(sim, word)
        _lib.check(L.tmh_set_storage(sim._eng, None))
        _lib.check(L.tmh_set_storage(sim._eng, C.byref(sim._storage_desc)))   # (now storage after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        with pytest.raises(ValueError, match="battery storage"):
            getattr(sim, "enable_" + kind)(500, 60)
        o = _sim(64, start, prec=PREC, horizon=1000)
        getattr(o, "enable_" + kind)(500, 60)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_storage(500, 60, **A_BATTERY)
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_storage(500, 60, **A_BATTERY)
    refused(seq, "storage tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_storage(500, 60, **A_BATTERY)
    refused(isim, "time-parallel", inj=isim._us)
    for key, val in (("Paco", float(L.tmh_series_max_w())), ("Pnt", float(L.tmh_series_max_w()))):
        mp = ModelParams()
        mp.inverter = dict(mp.inverter, **{key: val})                      # Paco, |Pnt| >= TMH_SERIES_MAX_W
        big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
        big.enable_storage(500, 60, **A_BATTERY)
        refused(big, "TMH_SERIES_MAX_W")
    # fp32 engines: refused at the setter and at enable_storage
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_storage(500, 60, **A_BATTERY)
    assert L.tmh_set_storage(f32._eng, C.byref(sim._storage_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"storage" in L.tmh_last_error()
    with pytest.raises(ValueError):
        sim.enable_storage(500, 60, capacity_wh=1e9, charge_w=1.0, discharge_w=1.0)
    with pytest.raises(ValueError, match="required"):
        sim.enable_storage(500, 60)

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_storage(500, 60, **A_BATTERY)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the storage"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.storage_raw.any())
    assert bool((sim.soc == bat["soc0"]).all())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.storage_raw)
    assert int(raw[0, 2].min()) >= 0 and int(raw[:2, 2].sum()) > 0
    assert not raw[2:].any()
    _identities(raw)
    _soc_changes(raw, bat["soc0"], _np(sim.soc))
    assert L.tmh_set_storage(sim._eng, None) == 0                          # NULL: off


def test_storage_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd import storage
    from tmhpvsim_amd.cli import TABLE_CSV, main
    f, z = tmp_path / "st.csv", tmp_path / "st.npz"
    r = CliRunner().invoke(main, ["storage", str(f), "--batch", "64", "--seconds", "1800", "--interval", "600",
                                  "--no-realtime", "--capacity-wh", "0.5", "--charge-w", "1000", "--discharge-w", "3000",
                                  "--soc0-wh", "0.25", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "import_wh", "export_wh", "pv_wh", "meter_wh", "charge_wh", "discharge_wh", "soc_wh",
                       "n_ok"] and len(rows) == 1 + 3
    assert rows[0][1:] == [name for name, _ in TABLE_CSV["storage"]]
    saved = np.load(z)
    assert saved["raw"].shape == (3, 9, 64) and int(saved["interval_s"]) == 600
    _identities(saved["raw"])
    want = storage.to_watts(saved["raw"][:, :, :1], 600, n_steps=1800)       # column 0: chain 0
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00"]
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][k, 0]) for _, key in TABLE_CSV["storage"]]
    assert float(rows[1][3]) > 0 and float(rows[1][8]) == 600 and float(rows[1][6]) > 0   # noon: produces, discharges
    full = storage.to_watts(saved["raw"], 600, n_steps=1800)
    for key in full:
        np.testing.assert_array_equal(saved[key], full[key], err_msg=key)
    r = CliRunner().invoke(main, ["storage", str(f), "--batch", "4", "--no-realtime"])
    assert r.exit_code != 0 and "capacity-wh" in r.output
