"""The battery sweep on the GPU (tmh_set_battery_sweep, BatchedSim.enable_battery_sweep; fp64 throughout): K
batteries per chain in one run, every variant's table and state of charge bit for bit battery.from_traces of the
traces of separate sims of the same chains (test_gpu_storage.a60_gpu / c60_traces: computed once, shared with the
storage and battery tests), never from the kernels under test.  The variants are sweep_util's: K = 5, above the
kernels' four variants per launch and no multiple of it, so a full group of launches, a short last group and
the one-launch rule of the statistics all run."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from sweep_util import K, pair_shares, variants
from test_gpu_battery import _identities, _soc_changes, a_bt
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = variants()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, n_steps, interval_s, params=PARAMS, soc0=SOC0, **kw):
    """enable_battery_sweep with ready parameters and a caller-owned soc (sweep_util's by default)."""
    return sim.enable_battery_sweep(n_steps, interval_s, params=_dev(params), soc=_dev(soc0), **kw)


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected tables and end states of input A, variant by variant from the storage tests' traces."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    got = [battery.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS[v], soc0=SOC0[v]) for v in range(K)]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


@functools.lru_cache(maxsize=None)
def a_sw():
    """The sweep sim of input A, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV)
    assert tuple(raw.shape) == (K, 13, 10, A_N) and tuple(sim.soc.shape) == (K, A_N) and sim.soc.dtype == torch.int64
    assert tuple(sim.battery_params.shape) == (K, 6, A_N) and sim.battery_sweep_raw is raw
    variants_, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants_, guards=guards, status=sim.status(),
                watts=sim.battery_sweep())


def test_sweep_equals_the_traces_tables():
    """The main test: every variant's ten columns and state of charge bit for bit, over two windows (the second
    off the four-step grid), chains faulted at construction and inside the window, night and day; a full group of
    four variants and a last group of one."""
    from tmhpvsim_amd import _lib, battery
    g, t = a_sw(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    live = g["status"] == 0
    shares = pair_shares(want[:, :, 4], live)
    print("column-4 shares", {k: round(s, 4) for k, s in shares.items()})
    assert min(shares.values()) >= 0.9                                   # (test_battery_sweep_cpu.MIN_PAIR_SHARE)
    assert g["variants"] == [_lib.OUT_BATTERY_SWEEP | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    dead = g["status"] == 1
    assert dead.any()
    for v in range(K):
        for col in range(10):
            np.testing.assert_array_equal(g["raw"][v, :, col], want[v, :, col], err_msg=f"variant {v} column {col}")
        np.testing.assert_array_equal(g["soc"][v], end[v], err_msg=f"variant {v} soc")
        assert not g["raw"][v][:, :, dead].any() and (g["soc"][v][dead] == SOC0[v][dead]).all()
        _identities(g["raw"][v])
        _soc_changes(g["raw"][v], SOC0[v], g["soc"][v])
        np.testing.assert_array_equal(g["raw"][v, :, :4], g["raw"][0, :, :4])
        w = battery.to_watts(want[v], IV, n_steps=A_STEPS)
        assert set(g["watts"][v]) == set(w)
        for key in w:
            np.testing.assert_array_equal(g["watts"][v][key], w[key], err_msg=key)
    b = a_bt()                                                             # variant 0: the recipe, the battery kind's own run
    np.testing.assert_array_equal(g["raw"][0], b["raw"])
    np.testing.assert_array_equal(g["soc"][0], b["soc"])


def test_windows_pipelining_and_compaction_same_bits():
    """One pipelined run over windows of 4,000 steps and compacted windows of 3,601 steps (from the second window on
    only the live chains run, in dense slots; every variant's soc, table column and parameters are the chain's)."""
    want, end = a_want()
    pipe = _sim(A_N, A_START, **_kw60())
    rawp = _enable(pipe, A_STEPS, IV)
    pipe.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(rawp), want)
    np.testing.assert_array_equal(_np(pipe.soc), end)
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV)
    sim.run(A_STEPS, trace=(), window=3601, compact=True)
    torch.cuda.synchronize()
    assert len(sim.compact_slots) == 3 and sim.compact_slots[0] == A_N
    assert min(sim.compact_slots) < A_N, sim.compact_slots        # a window ran on fewer slots than chains
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)


@pytest.mark.parametrize("interval_s", [7, 128])
@pytest.mark.parametrize("n", [1300, 64])
def test_sweep_boundaries(n, interval_s):
    """Boundaries inside four-second groups (7) and one per 128-s block (128); the origin three steps before the
    run; a partial wavefront, more than one workgroup and construction faults; the variants tiled past A_N."""
    from tmhpvsim_amd import _lib, battery
    pv, meter, cov = c60_traces(n)
    par, soc0 = variants(K, n)
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_BATTERY_SWEEP | _lib.OUT_FP64
    torch.cuda.synchronize()
    got, soc = _np(raw), _np(sim.soc)
    assert got.shape == (K, -(-(C_STEPS + C_LEAD) // interval_s), 10, n)
    for v in range(K):
        want, end = battery.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par[v], soc0=soc0[v])
        np.testing.assert_array_equal(got[v], want, err_msg=f"variant {v}")
        np.testing.assert_array_equal(soc[v], end, err_msg=f"variant {v}")
        _identities(got[v])
        _soc_changes(got[v], soc0[v], soc[v])
        assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0
    assert (got[0, :, 4:] != got[K - 1, :, 4:]).any()


def test_variant_counts():
    """K = 1 is enable_battery bit for bit (a_bt: the recipe); a sweep over the first two variants is the first two
    slices of the K-variant sweep (a short only group against a full one)."""
    from tmhpvsim_amd import _lib
    g, b = a_sw(), a_bt()
    one = _sim(A_N, A_START, **_kw60())
    r1 = _enable(one, A_STEPS, IV, PARAMS[:1], SOC0[:1])
    _run_windows(one, A_WINDOWS)
    assert _last(one) == _lib.OUT_BATTERY_SWEEP | _lib.OUT_FP64 and tuple(r1.shape) == (1, 13, 10, A_N)
    np.testing.assert_array_equal(_np(r1)[0], b["raw"])
    np.testing.assert_array_equal(_np(one.soc)[0], b["soc"])
    two = _sim(A_N, A_START, **_kw60())
    r2 = _enable(two, A_STEPS, IV, PARAMS[:2], SOC0[:2])
    _run_windows(two, A_WINDOWS)
    np.testing.assert_array_equal(_np(r2), g["raw"][:2])
    np.testing.assert_array_equal(_np(two.soc), g["soc"][:2])
    assert (g["raw"][1, :, 4:] != g["raw"][0, :, 4:]).any()


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_sweep(spec):
    """Statistics beside the sweep are the statistics-only run's, bit for bit: of the two groups' replay launches
    exactly one accumulates them (two would double the histogram and the energies), the map passes none."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, soc0 = PARAMS[:, :, :n], SOC0[:, :n]
    both, stats, alone = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = _enable(both, steps, 600, par, soc0), _enable(alone, steps, 600, par, soc0)
    for s in (both, stats, alone):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_BATTERY_SWEEP | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[0, :, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[0, :, 2].sum()) == int(ra[K - 1, :, 2].sum())
    for v in range(K):
        assert int(ra[v, :, 6].sum()) > 0 and int(ra[v, :, 7].sum()) > 0 and int(ra[v, :, 9].sum()) > 0
        _identities(_np(ra[v]))


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one [K, 13, 10, 1000] table, reading
    slices of one [K, 6, 1000] params tensor and carrying slices of one [K, 1000] soc."""
    want, end = a_want()
    big = torch.zeros(K, 13, 10, A_N, dtype=torch.int64, device="cuda:0")
    params, soc = _dev(PARAMS), _dev(SOC0)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, :, a:b]
        got = s.enable_battery_sweep(A_STEPS, IV, buffer=view, soc=soc[:, a:b], params=params[:, :, a:b])
        assert got is view and s._battery_sweep.ld == A_N and s.soc.data_ptr() == soc[:, a:b].data_ptr()
        assert s.battery_params.data_ptr() == params[:, :, a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    with pytest.raises(ValueError, match="strides"):
        s.enable_battery_sweep(A_STEPS, IV, buffer=big[:, :, :, :2 * s.n:2], params=params[:, :, 500:], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="battery sweep buffer"):
        s.enable_battery_sweep(A_STEPS, IV, buffer=torch.zeros(K, 13, 9, s.n, dtype=torch.int64, device="cuda:0"),
                               params=params[:, :, 500:], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="same width"):                                    # params of another width than the table
        s.enable_battery_sweep(A_STEPS, IV, params=params[:, :, 500:])
    with pytest.raises(ValueError, match="params"):
        s.enable_battery_sweep(A_STEPS, IV, buffer=big[:, :, :, 500:], params=params[:, :, :2 * s.n:2], soc=soc[:, 500:])
    with pytest.raises(ValueError, match="soc"):
        s.enable_battery_sweep(A_STEPS, IV, buffer=big[:, :, :, 500:], params=params[:, :, 500:], soc=soc[:, :2 * s.n:2])
    s.enable_battery_sweep(None)
    assert s.soc is None and s.battery_sweep_raw is None and s.battery_params is None


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "battery sweep" before anything is launched: the
    chains' state and the batteries' stay as they were and the tables all zeros; what was enabled before still works."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams, site_grid
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :, :n], SOC0[:, :n]
    SW = dict(capacity_wh=[0.5, 0.25, 0.75], charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9,
              standby_w=1.0, soc0_wh=0.25)

    def refused(sim, match, step0=0, k=100, trace=None, inj=None, raw=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "battery sweep" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool((sim.battery_sweep_raw if raw is None else raw).any())

    def desc(sim, **kw):
        """The sim's tmh_battery_sweep with fields replaced."""
        d = sim._sweep_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params, n_variants=d.n_variants)
        return _lib.BatterySweep(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "battery sweep tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # the sweep, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_battery_sweep(None)
    sim.enable_series(500)                                                 # a fleet series, then the sweep
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, soc0)
    sim.run(10, trace=())                                                  # the series still works
    torch.cuda.synchronize()
    assert int(sim.series_raw[0, :10, 2].sum()) > 0
    sim.enable_series(None)
    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    refused(sim, "outside the battery sweep", step0=0, k=501)              # past the end
    refused(sim, "outside the battery sweep", step0=450, k=100)
    _enable(sim, 500, 60, par, soc0, step0=10)
    refused(sim, "outside the battery sweep", step0=0, k=100)              # before the origin
    buf = _enable(sim, 500, 60, par, soc0)
    _lib.check(L.tmh_set_battery_sweep(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "battery sweep tables ld")                                # ld too small
    _lib.check(L.tmh_set_battery_sweep(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_battery_sweep_work_bytes(n, 100, K) - 8))))
    refused(sim, "work buffer too small")                                  # enough for four variants of the window, not five
    p = buf.data_ptr()
    for kw, word in ((dict(table=_lib.Intervals(p + 4, 0, 500, 60, n)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(None, 0, 500, 60, n)), b"buffer"),
                     (dict(table=_lib.Intervals(p, 0, 500, 0, n)), b"interval_s"),
                     (dict(table=_lib.Intervals(p, 0, 0, 60, n)), b"n_steps"),
                     (dict(table=_lib.Intervals(p, 0, 500, 60, 0)), b"ld"),
                     (dict(table=_lib.Intervals(p, 0, 500, 1 << 23, n)), b"2^23"),
                     (dict(n_variants=0), b"n_variants"), (dict(n_variants=17), b"n_variants"),
                     (dict(soc=None), b"soc"), (dict(soc=sim.soc.data_ptr() + 4), b"soc"),
                     (dict(work=None), b"work"), (dict(work=p + 4), b"work"), (dict(work_bytes=K * 24 - 8), b"too small"),
                     (dict(params=None), b"params"), (dict(params=sim.battery_params.data_ptr() + 4), b"params")):
        assert L.tmh_set_battery_sweep(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"battery sweep" in L.tmh_last_error()                      # the setter refuses a bad struct
    # the sweep with another table kind on one engine, storage and the battery kind included, set in either order
    _enable(sim, 500, 60, par, soc0)
    for kind, cols, word in (("intervals", 4, "the battery sweep and interval metering"),
                             ("registers", 6, "the battery sweep and the import / export registers"),
                             ("demand", 8, "the battery sweep and the demand registers"),
                             ("storage", 9, "the battery sweep and battery storage"),
                             ("battery", 10, "the battery sweep and the battery kind")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._sweep_desc
        arg = (_lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage"
               else _lib.Battery(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "battery" else tbl)
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_battery_sweep(sim._eng, None))
        _lib.check(L.tmh_set_battery_sweep(sim._eng, C.byref(sim._sweep_desc)))   # (now the sweep after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        extra = A_BATTERY if kind in ("storage", "battery") else {}
        with pytest.raises(ValueError, match="the battery sweep"):
            getattr(sim, "enable_" + kind)(500, 60, **extra)
        o = _sim(64, start, prec=PREC, horizon=1000)
        oraw = getattr(o, "enable_" + kind)(500, 60, **extra)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_battery_sweep(500, 60, **SW)
        o.run(60, trace=())                                                # the table enabled before still works
        torch.cuda.synchronize()
        assert int(oraw[0, 2].sum()) > 0 and o.battery_sweep_raw is None
    # the battery fleet series: the battery kind's own output, in either order
    fl = torch.zeros(1, 500, 8, dtype=torch.int64, device="cuda:0")
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(fl.data_ptr(), 0, 500, 0, 1, 0))))
    refused(sim, "battery fleet series")
    _lib.check(L.tmh_set_battery_sweep(sim._eng, None))
    _lib.check(L.tmh_set_battery_sweep(sim._eng, C.byref(sim._sweep_desc)))
    refused(sim, "battery fleet series")
    assert not bool(fl.any())
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    with pytest.raises(ValueError, match="enable_battery first"):
        sim.enable_battery_fleet(500)
    o = _sim(64, start, prec=PREC, horizon=1000)
    o.enable_battery(500, 60, **A_BATTERY)
    o.enable_battery_fleet(500)
    with pytest.raises(ValueError, match="battery fleet series"):
        o.enable_battery_sweep(500, 60, **SW)
    o.run(60, trace=())
    torch.cuda.synchronize()
    assert int(o.battery_fleet_raw[0, :60, 2].sum()) > 0 and int(o.battery_raw[0, 2].sum()) > 0
    # per-chain sites
    ss = _sim(64, start, prec=PREC, horizon=1000, sites=site_grid(8, 8))
    with pytest.raises(ValueError, match="per-chain sites"):
        ss.enable_battery_sweep(500, 60, **SW)
    sraw = torch.zeros(K, 9, 10, 64, dtype=torch.int64, device="cuda:0")
    ssoc, spar = _dev(SOC0[:, :64]), _dev(PARAMS[:, :, :64])
    swork = torch.empty(L.tmh_battery_sweep_work_bytes(64, 500, K), dtype=torch.uint8, device="cuda:0")
    sdesc = _lib.BatterySweep(_lib.Intervals(sraw.data_ptr(), 0, 500, 60, 64), ssoc.data_ptr(), swork.data_ptr(), swork.numel(),
                              spar.data_ptr(), K)
    _lib.check(L.tmh_set_battery_sweep(ss._eng, C.byref(sdesc)))
    ss.soc = ssoc
    refused(ss, "per-chain sites", raw=sraw)
    _lib.check(L.tmh_set_battery_sweep(ss._eng, None))
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_battery_sweep(500, 60, **SW)
    refused(seq, "battery sweep tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_battery_sweep(500, 60, **SW)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))      # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
    big.enable_battery_sweep(500, 60, **SW)
    refused(big, "TMH_SERIES_MAX_W")
    # fp32 engines: refused at the setter and at enable_battery_sweep
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_battery_sweep(500, 60, **SW)
    assert L.tmh_set_battery_sweep(f32._eng, C.byref(sim._sweep_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"battery sweep" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges before upload, a soc0 outside [0, C], lists of two lengths
    for bad in (dict(capacity_wh=1e9), dict(charge_w=-1.0), dict(charge_eff=0.4), dict(discharge_eff=[1.1, 1.0, 1.0]),
                dict(standby_w=-1.0), dict(soc0_wh=0.6), dict(soc0_wh=-0.1), dict(charge_w=[1.0, 2.0]),
                dict(capacity_wh=[0.5] * 17), dict(n_variants=4)):
        with pytest.raises(ValueError):
            sim.enable_battery_sweep(500, 60, **{**SW, **bad})
    worse = par.copy()
    worse[2, 3, 5] = 70000
    with pytest.raises(ValueError, match="eff_charge"):
        sim.enable_battery_sweep(500, 60, params=_dev(worse))
    with pytest.raises(ValueError, match="required"):
        sim.enable_battery_sweep(500, 60)

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_battery_sweep(500, 60, **SW)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the battery sweep"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.battery_sweep_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.battery_sweep_raw)
    assert raw.shape == (3, 9, 10, n)
    for v in range(3):
        assert int(raw[v, :2, 2].sum()) > 0 and not raw[v, 2:].any()
        _identities(raw[v])
    assert L.tmh_set_battery_sweep(sim._eng, None) == 0                    # NULL: off


def test_battery_sweep_cli(tmp_path):
    """A CSV row per variant (its parameters, the fleet's totals and ratios) and the .npz's tables, against
    sweep_summary of the tables that sweep_from_traces gives for the traces of a separate sim."""
    from click.testing import CliRunner
    from tmhpvsim_amd import battery
    from tmhpvsim_amd.cli import SWEEP_OPTIONS, SWEEP_RATIOS, SWEEP_TOTALS, main
    from tmhpvsim_amd.params import ModelParams
    f, z = tmp_path / "sw.csv", tmp_path / "sw.npz"
    n, steps, iv = 64, 1800, 600
    caps = [0.05, 0.0, 0.02, 0.05, 0.1]
    r = CliRunner().invoke(main, ["battery-sweep", str(f), "--batch", str(n), "--seconds", str(steps), "--interval", str(iv),
                                  "--no-realtime", "--capacity-wh", ",".join(map(str, caps)), "--charge-w", "1000",
                                  "--discharge-w", "3000,1500,3000,3000,50", "--charge-eff", "0.95", "--discharge-eff",
                                  "0.9,1.0,1.0,0.9,0.9", "--standby-w", "2", "--soc0-wh", "0.02,0,0.01,0,0.1",
                                  "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    opts = dict(capacity_wh=caps, charge_w=[1000.0] * 5, discharge_w=[3000.0, 1500.0, 3000.0, 3000.0, 50.0],
                charge_eff=[0.95] * 5, discharge_eff=[0.9, 1.0, 1.0, 0.9, 0.9], standby_w=[2.0] * 5,
                soc0_wh=[0.02, 0.0, 0.01, 0.0, 0.1])
    par = battery.quantize_sweep_params(*(opts[o] for o in SWEEP_OPTIONS[:6]), n=n)
    soc0 = battery.quantize_sweep_soc(opts["soc0_wh"], par)
    tr = _sim(n, "2019-09-06T12:00:00", prec=PREC, mp=ModelParams(seed=0x5EED), horizon=steps)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = battery.sweep_from_traces(out["pv"], out["meter"], out["covered"], iv, params=par, soc0=soc0)
    saved = np.load(z)
    assert saved["raw"].shape == (5, 3, 10, n) and int(saved["interval_s"]) == iv
    np.testing.assert_array_equal(saved["raw"], want)
    np.testing.assert_array_equal(saved["soc"], end)
    np.testing.assert_array_equal(saved["params"], par)
    fleet = battery.sweep_summary(want, iv, par, fleet=True)
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["variant"] + list(SWEEP_OPTIONS) + [h for h, _ in SWEEP_TOTALS] + list(SWEEP_RATIOS) and len(rows) == 1 + 5
    for v, row in enumerate(rows[1:]):
        assert int(row[0]) == v and [float(x) for x in row[1:8]] == [opts[o][v] for o in SWEEP_OPTIONS]
        got = [float(x) for x in row[8:]]
        exp = [float(fleet[key][v]) for _, key in SWEEP_TOTALS] + [float(fleet[key][v]) for key in SWEEP_RATIOS]
        assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(got, exp)), (v, got, exp)
    assert np.isnan(float(rows[2][-1])) and float(rows[1][-1]) > 0           # no battery: no cycles
    assert float(rows[1][8]) != float(rows[5][8])                            # another battery, another import
