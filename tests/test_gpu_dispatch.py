"""Battery dispatch on the GPU (tmh_set_dispatch, BatchedSim.enable_dispatch; fp64 throughout): integers, so
every comparison with the traces' table (dispatch.from_traces, a plain loop over the seconds) is bit for bit.
The expected table and state of charge always come from traces of separate sims of the same chains
(test_gpu_storage.a60_gpu / c60_traces: computed once, shared with the storage and battery tests), never from
the kernels under test.  The households are dispatch_util.recipe's: battery_util's per-chain batteries plus a
charge threshold, a discharge threshold and a feed-in limit per chain."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from battery_util import QUARTER_WH
from dispatch_util import A_FLOORS, NO_LIMIT, identities, recipe, run, soc_changes, tiled
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = recipe()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, n_steps, interval_s, params=PARAMS, soc0=SOC0, **kw):
    """enable_dispatch with ready parameters and a caller-owned soc (the recipe's by default)."""
    return sim.enable_dispatch(n_steps, interval_s, params=_dev(params), soc=_dev(soc0), **kw)


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected table and end state of input A with the recipe's households, from the storage tests' traces."""
    from tmhpvsim_amd import dispatch
    t = a60_gpu()
    return dispatch.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, soc0=SOC0)


@functools.lru_cache(maxsize=None)
def a_dp():
    """The dispatch sim of input A, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV)
    assert tuple(raw.shape) == (13, 13, A_N) and tuple(sim.soc.shape) == (A_N,) and sim.soc.dtype == torch.int64
    assert tuple(sim.dispatch_params.shape) == (9, A_N) and sim.dispatch_raw is raw
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def test_dispatch_equals_the_traces_table():
    """The main test: all thirteen columns and the state of charge bit for bit, over two windows (the second off
    the four-step grid), chains faulted at construction and inside the window, night and day, thresholds that
    block and let through charges and discharges, limits that curtail while the battery is full and while it
    charges."""
    from tmhpvsim_amd import _lib
    g, t = a_dp(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    _, _, ev = run(t["pv"], t["meter"], t["cov"], IV, PARAMS, SOC0)
    dead = g["status"] == 1
    print(ev, "dead at construction", int(dead.sum()), "in-window faults", int(((t["cov"][-1] == 255) & ~dead).sum()))
    for name, floor in A_FLOORS.items():
        assert ev[name] >= floor, (name, ev[name], floor)
    assert g["variants"] == [_lib.OUT_DISPATCH | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(13):
        np.testing.assert_array_equal(g["raw"][:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(g["soc"], end)
    assert dead.any() and not g["raw"][:, :, dead].any() and (g["soc"][dead] == SOC0[dead]).all()
    identities(g["raw"], PARAMS)
    soc_changes(g["raw"], SOC0, g["soc"])
    assert int((g["raw"][:, 10].sum(axis=0) > 0).sum()) >= A_FLOORS["curtail_chains"]
    assert g["raw"][12, 2].max() == 3 and g["raw"][:12, 2].max() == IV          # the last partial interval


def test_windows_pipelining_and_compaction_same_bits():
    """One tmh_run per window (a_dp), one pipelined run over windows of 4,000 steps, and compacted windows
    of 3,601 steps (from the second window on only the live chains run, in dense slots: a slot's work column
    is the slot's; its soc, its table column and its nine parameters are the chain's, ids[slot]): the same bits."""
    g = a_dp()
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
    ids = np.flatnonzero(g["status"] != 1)                        # the second window's chains, in slot order (at least)
    for row in range(9):                                          # parameters indexed by slot would be other chains'
        assert (PARAMS[row, ids] != PARAMS[row, :len(ids)]).any(), row
    np.testing.assert_array_equal(_np(raw), g["raw"])
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    np.testing.assert_array_equal(sim.status(), g["status"])


@pytest.mark.parametrize("interval_s", [7, 128])
@pytest.mark.parametrize("n", [1300, 64])
def test_dispatch_boundaries(n, interval_s):
    """Boundaries inside four-second groups (7) and one per 128-s block (128); the origin three steps before
    the run, so no interval edge coincides with a window edge; a partial wavefront and construction faults;
    the C recipe (thresholds and limits that bind just after sunrise) tiled past A_N."""
    from tmhpvsim_amd import _lib, demand, dispatch
    pv, meter, cov = c60_traces(n)
    par, soc0 = tiled(n, "C")
    want, end, ev = run(pv, meter, cov, interval_s, par, soc0, origin=C_LEAD)
    print(f"n {n}: {ev}, construction faults {int((cov[0] == 255).sum())}")
    for name, count in ev.items():
        assert count > 0 or name == "partial_fill", name
    if n > 1000:
        assert ev["partial_fill"] > 0 and (cov[0] == 255).any()                           # construction faults
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_DISPATCH | _lib.OUT_FP64
    torch.cuda.synchronize()
    ref, rend = dispatch.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par, soc0=soc0)
    np.testing.assert_array_equal(ref, want)                      # (the two derivations agree on this input too)
    assert tuple(raw.shape) == want.shape == (-(-(C_STEPS + C_LEAD) // interval_s), 13, n)
    for w0 in np.cumsum((0,) + C_WINDOWS)[:-1]:                   # where a window begins (and the one before it ends)
        assert (int(w0) + C_LEAD) % interval_s != 0
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    np.testing.assert_array_equal(rend, end)
    identities(_np(raw), par)
    soc_changes(_np(raw), soc0, _np(sim.soc))
    live0 = want[0, 2] == interval_s - C_LEAD                     # the first cell begins at offset C_LEAD
    assert live0.any()
    for col in (11, 12):
        assert (demand.unpack(_np(raw)[0, col, live0])[1] >= C_LEAD).all()


def test_reductions_to_the_battery_kind_and_the_demand_registers():
    """Tc = Td = 0 and no limit: columns 0-9 and soc are an enable_battery sim's bit for bit (the existing kernels
    as a second reference) and column 10 is 0.  No battery and no limit: columns 11 and 12 are an fp64
    enable_demand sim's columns 6 and 7."""
    from tmhpvsim_amd import _lib
    greedy = PARAMS.copy()
    greedy[6:8], greedy[8] = 0, NO_LIMIT
    bt = _sim(A_N, A_START, **_kw60())
    rb = bt.enable_battery(A_STEPS, IV, params=_dev(greedy[:6]), soc=_dev(SOC0))
    _run_windows(bt, A_WINDOWS)
    assert _last(bt) == _lib.OUT_BATTERY | _lib.OUT_FP64
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, greedy)
    _run_windows(sim, A_WINDOWS)
    assert _last(sim) == _lib.OUT_DISPATCH | _lib.OUT_FP64
    got = _np(raw)
    np.testing.assert_array_equal(got[:, :10], _np(rb))
    np.testing.assert_array_equal(_np(sim.soc), _np(bt.soc))
    assert not got[:, 10].any() and int(got[:, 6].sum()) > 0 and int(got[:, 7].sum()) > 0 and int(got[:, 9].sum()) > 0
    dm = _sim(A_N, A_START, **_kw60())
    rd = dm.enable_demand(A_STEPS, IV)
    _run_windows(dm, A_WINDOWS)
    assert _last(dm) == _lib.OUT_DEMAND | _lib.OUT_FP64
    none = _sim(A_N, A_START, **_kw60())
    rn = none.enable_dispatch(A_STEPS, IV, capacity_wh=0.0, charge_w=1000.0, discharge_w=3000.0,
                              charge_above_w=250.0, discharge_above_w=2000.0)
    assert (_np(none.dispatch_params)[8] == NO_LIMIT).all()
    _run_windows(none, A_WINDOWS)
    gn, gd = _np(rn), _np(rd)
    np.testing.assert_array_equal(gn[:, 11:13], gd[:, 6:8])
    np.testing.assert_array_equal(gn[:, :6], gd[:, :6])
    assert not gn[:, 6:8].any() and not gn[:, 9:11].any() and int((gd[:, 7] >> 32).max()) > 0


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one table, reading slices of
    one [9, 1000] params tensor and carrying slices of one soc."""
    want, end = a_want()
    big = torch.zeros(13, 13, A_N, dtype=torch.int64, device="cuda:0")
    params, soc = _dev(PARAMS), _dev(SOC0)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_dispatch(A_STEPS, IV, buffer=view, soc=soc[a:b], params=params[:, a:b])
        assert got is view and s._dispatch.ld == A_N and s.soc.data_ptr() == soc[a:b].data_ptr()
        assert s.dispatch_params.data_ptr() == params[:, a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    with pytest.raises(ValueError, match="strides"):
        s.enable_dispatch(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2], params=params[:, 500:])  # chains not contiguous
    with pytest.raises(ValueError, match="dispatch buffer"):
        s.enable_dispatch(A_STEPS, IV, buffer=torch.zeros(13, 10, s.n, dtype=torch.int64, device="cuda:0"),
                          params=params[:, 500:])
    with pytest.raises(ValueError, match="row stride"):                                    # params of another width than the table
        s.enable_dispatch(A_STEPS, IV, params=params[:, 500:])
    with pytest.raises(ValueError, match="params"):
        s.enable_dispatch(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, :2 * s.n:2])
    with pytest.raises(ValueError, match="params"):                                        # the battery kind's six rows only
        s.enable_dispatch(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:6, 500:])
    with pytest.raises(ValueError, match="soc"):
        s.enable_dispatch(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, 500:], soc=soc[:2 * s.n:2])
    s.enable_dispatch(None)
    assert s.soc is None and s.dispatch_raw is None and s.dispatch_params is None


def test_dispatch_per_chain_sites(spec="default"):
    """The per-chain-sites kernels (map and replay), with statistics beside the table."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib, dispatch
    import dataclasses
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    par, soc0 = (a[..., :n] for a in recipe(A_N, "C"))
    mp = dataclasses.replace(modules_params(), cc_mode=ModelParams().cc_mode, seed=0x51E)
    sim = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    raw = _enable(sim, steps + 1, 450, par, soc0, step0=-1)
    stats = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    for s in (sim, stats):
        s.enable_stats(**HISTS[spec])
    stats.run(steps, trace=(), window=1700)
    assert _last(stats) & 7 == _lib.OUT_STATS
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_DISPATCH | _lib.OUT_SITES | _lib.OUT_FP64
    tr = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = dispatch.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1, params=par, soc0=soc0)
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0 and int(want[:, 9].sum()) > 0
    print("curtailed", int(want[:, 10].sum()), "peak feed-in", int((want[:, 12] >> 32).max()))
    identities(want, par)
    assert int(stats.hist.sum()) == int(raw[:, 2].sum()) > 0
    assert torch.equal(sim.hist, stats.hist)
    assert torch.equal(sim.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_dispatch(spec):
    """Statistics beside the dispatch table are the statistics-only run's, bit for bit (the map pass adds
    nothing to them), and the table is the dispatch-only one."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw60(steps)
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    both, stats, alone = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = _enable(both, steps, 600, par, soc0), _enable(alone, steps, 600, par, soc0)
    for s in (both, stats, alone):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) == _lib.OUT_DISPATCH | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[:, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    assert int(ra[:, 6].sum()) > 0 and int(ra[:, 7].sum()) > 0 and int(ra[:, 9].sum()) > 0
    identities(_np(ra), par)


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "dispatch" before anything is launched: the
    chains' state and the batteries' stay as they were and the table all zeros."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    BAT = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9, standby_w=1.0,
               soc0_wh=0.25)
    DSP = dict(BAT, charge_above_w=250.0, discharge_above_w=2000.0, feed_in_limit_w=500.0)

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "dispatch" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool(sim.dispatch_raw.any())

    def desc(sim, **kw):
        """The sim's tmh_dispatch with fields replaced."""
        d = sim._dispatch_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params)
        return _lib.Dispatch(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "dispatch tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # dispatch, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_dispatch(None)
    sim.enable_series(500)                                                 # a fleet series, then dispatch
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, soc0)
    sim.enable_series(None)
    _enable(sim, 500, 60, par, soc0)
    fl = torch.zeros(1, 500, 8, dtype=torch.int64, device="cuda:0")        # the battery fleet series beside dispatch
    _lib.check(L.tmh_set_battery_fleet(sim._eng, C.byref(_lib.Series(fl.data_ptr(), 0, 500, 0, 1, 0))))
    refused(sim, "battery fleet series")
    assert not bool(fl.any())
    _lib.check(L.tmh_set_battery_fleet(sim._eng, None))
    with pytest.raises(ValueError, match="enable_battery first"):
        sim.enable_battery_fleet(500)
    refused(sim, "outside the battery dispatch", step0=0, k=501)           # past the end
    refused(sim, "outside the battery dispatch", step0=450, k=100)
    _enable(sim, 500, 60, par, soc0, step0=10)
    refused(sim, "outside the battery dispatch", step0=0, k=100)           # before the origin
    buf = _enable(sim, 500, 60, par, soc0)
    _lib.check(L.tmh_set_dispatch(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "dispatch tables ld")                                     # ld too small
    _lib.check(L.tmh_set_dispatch(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_storage_work_bytes(n, 100) - 8))))
    refused(sim, "work buffer too small")
    p = buf.data_ptr()
    for kw, word in ((dict(table=_lib.Intervals(p + 4, 0, 500, 60, n)), b"8-byte aligned"),
                     (dict(table=_lib.Intervals(None, 0, 500, 60, n)), b"buffer"),
                     (dict(table=_lib.Intervals(p, 0, 500, 0, n)), b"interval_s"),
                     (dict(table=_lib.Intervals(p, 0, 0, 60, n)), b"n_steps"),
                     (dict(table=_lib.Intervals(p, 0, 500, 60, 0)), b"ld"),
                     (dict(table=_lib.Intervals(p, 0, 500, 1 << 23, n)), b"2^23"),
                     (dict(soc=None), b"soc"), (dict(soc=sim.soc.data_ptr() + 4), b"soc"),
                     (dict(work=None), b"work"), (dict(work=p + 4), b"work"),
                     (dict(params=None), b"params"), (dict(params=sim.dispatch_params.data_ptr() + 4), b"params")):
        assert L.tmh_set_dispatch(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"dispatch" in L.tmh_last_error()                           # the setter refuses a bad struct
    # dispatch with another table kind on one engine -- storage, the battery kind and the sweep included -- in either order
    _enable(sim, 500, 60, par, soc0)
    for kind, cols, word in (("intervals", 4, "battery dispatch and interval metering"),
                             ("registers", 6, "battery dispatch and the import / export registers"),
                             ("demand", 8, "battery dispatch and the demand registers"),
                             ("storage", 9, "battery dispatch and battery storage"),
                             ("battery", 10, "battery dispatch and the battery kind"),
                             ("battery_sweep", 10, "battery dispatch and the battery sweep")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._dispatch_desc
        arg = (_lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage"
               else _lib.Battery(tbl, d.soc, d.work, d.work_bytes, d.params) if kind == "battery"
               else _lib.BatterySweep(tbl, d.soc, d.work, d.work_bytes, d.params, 1) if kind == "battery_sweep" else tbl)
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_dispatch(sim._eng, None))
        _lib.check(L.tmh_set_dispatch(sim._eng, C.byref(sim._dispatch_desc)))   # (now dispatch after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        kw = A_BATTERY if kind == "storage" else BAT if kind in ("battery", "battery_sweep") else {}
        with pytest.raises(ValueError, match="battery dispatch"):
            getattr(sim, "enable_" + kind)(500, 60, **kw)
        o = _sim(64, start, prec=PREC, horizon=1000)
        getattr(o, "enable_" + kind)(500, 60, **kw)
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_dispatch(500, 60, **DSP)
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_dispatch(500, 60, **DSP)
    refused(seq, "dispatch tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_dispatch(500, 60, **DSP)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))      # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
    big.enable_dispatch(500, 60, **DSP)
    refused(big, "TMH_SERIES_MAX_W")
    # fp32 engines: refused at the setter and at enable_dispatch
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_dispatch(500, 60, **DSP)
    assert L.tmh_set_dispatch(f32._eng, C.byref(sim._dispatch_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"dispatch" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges before upload, and a soc0 outside [0, C]
    for bad in (dict(capacity_wh=1e9), dict(charge_w=-1.0), dict(charge_eff=0.4), dict(discharge_eff=1.1),
                dict(standby_w=-1.0), dict(soc0_wh=0.6), dict(soc0_wh=-0.1), dict(capacity_wh=[0.5] * 7),
                dict(charge_above_w=-1.0), dict(discharge_above_w=40000.0), dict(feed_in_limit_w=-1.0),
                dict(feed_in_limit_w=float("nan")), dict(charge_above_w=[1.0] * 7)):
        with pytest.raises(ValueError):
            sim.enable_dispatch(500, 60, **{**DSP, **bad})
    worse = par.copy()
    worse[8, 5] = (1 << 27) + 1
    with pytest.raises(ValueError, match="feed_in_limit"):
        sim.enable_dispatch(500, 60, params=_dev(worse))
    with pytest.raises(ValueError, match="required"):
        sim.enable_dispatch(500, 60)

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_dispatch(500, 60, **DSP)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the dispatch"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.dispatch_raw.any())
    assert bool((sim.soc == QUARTER_WH).all())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.dispatch_raw)
    assert int(raw[0, 2].min()) >= 0 and int(raw[:2, 2].sum()) > 0
    assert not raw[2:].any()
    identities(raw, _np(sim.dispatch_params))
    soc_changes(raw, np.full(n, QUARTER_WH), _np(sim.soc))
    assert L.tmh_set_dispatch(sim._eng, None) == 0                         # NULL: off


def test_dispatch_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd import dispatch
    from tmhpvsim_amd.cli import TABLE_CSV, main
    f, z = tmp_path / "dp.csv", tmp_path / "dp.npz"
    r = CliRunner().invoke(main, ["dispatch", str(f), "--batch", "64", "--seconds", "1800", "--interval", "600",
                                  "--no-realtime", "--capacity-wh", "0.5,0,0.25", "--charge-w", "1000", "--discharge-w",
                                  "3000,1500", "--charge-eff", "0.95", "--discharge-eff", "0.9,1.0", "--standby-w", "2",
                                  "--soc0-wh", "0.25,0,0.25", "--charge-above-w", "20,0", "--discharge-above-w", "100",
                                  "--feed-in-limit-w", "10,none,60", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "import_wh", "export_wh", "pv_wh", "meter_wh", "charge_wh", "discharge_wh", "soc_wh",
                       "loss_wh", "n_ok", "curtailed_wh", "peak_import_w", "peak_export_w"] and len(rows) == 1 + 3
    assert rows[0][1:] == [name for name, _ in TABLE_CSV["dispatch"]]
    assert TABLE_CSV["dispatch"][:len(TABLE_CSV["battery"])] == TABLE_CSV["battery"]
    saved = np.load(z)
    raw = saved["raw"]
    assert raw.shape == (3, 13, 64) and int(saved["interval_s"]) == 600
    lim = np.array([10 << 12, NO_LIMIT, 60 << 12], dtype=np.int64)[np.arange(64) % 3]     # dealt round-robin
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7] + raw[:, 10])
    assert ((raw[:, 12] >> 32) <= lim).all()
    want = dispatch.to_watts(raw[:, :, :1], 600, n_steps=1800)             # column 0: chain 0
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00"]
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][k, 0]) for _, key in TABLE_CSV["dispatch"]]
    assert float(rows[1][3]) > 0 and float(rows[1][9]) == 600              # noon: produces
    # ... and curtails: chain 0 charges from the surplus above 20 W only and may feed in 10 W, so a second with more
    # than 20 W of surplus leaves 20 W at the meter while the battery has room, 10 W of them thrown away
    assert float(rows[1][10]) > 0 and float(rows[1][12]) == 10.0
    full = dispatch.to_watts(raw, 600, n_steps=1800)
    for key in full:
        np.testing.assert_array_equal(saved[key], full[key], err_msg=key)
    assert {"energy_wh_curtailed", "curtailed_share", "peak_w_import", "peak_w_export", "t_peak_import",
            "t_peak_export", "energy_wh_loss", "soc_wh"} <= set(saved.files)
    nolim = np.arange(64) % 3 == 1                                          # `none`: nothing curtailed
    assert not raw[:, 10, nolim].any() and int(raw[:, 10, ~nolim].sum()) > 0
    r = CliRunner().invoke(main, ["dispatch", str(f), "--batch", "4", "--no-realtime"])
    assert r.exit_code != 0 and "capacity-wh" in r.output
    r = CliRunner().invoke(main, ["dispatch", str(f), "--batch", "4", "--no-realtime", "--capacity-wh", "1", "--charge-w", "1",
                                  "--discharge-w", "1", "--feed-in-limit-w", "-5"])
    assert r.exit_code != 0 and "feed_in_limit" in r.output
