"""The battery kind on the GPU (tmh_set_battery, BatchedSim.enable_battery; fp64 throughout): integers, so
every comparison with the traces' table (battery.from_traces, a plain loop over the seconds) is bit for bit.
The expected table and state of charge always come from traces of separate sims of the same chains
(test_gpu_storage.a60_gpu / c60_traces: computed once, shared with the storage tests), never from the
kernels under test.  The batteries are battery_util.recipe's: per-chain capacities (none included), power
limits, efficiencies and standby drains."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from battery_util import QUARTER_WH, events, recipe, uniform
from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth
from storage_util import A_BATTERY, modules_params
from storage_util import battery as storage_battery
from test_gpu_registers import C_LEAD, C_START, C_STEPS, C_WINDOWS, _run_windows
from test_gpu_series import _last, _np, _sim
from test_gpu_storage import IV, PREC, _kw60, a60_gpu, c60_traces

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

PARAMS, SOC0 = recipe()


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _enable(sim, n_steps, interval_s, params=PARAMS, soc0=SOC0, **kw):
    """enable_battery with ready parameters and a caller-owned soc (the recipe's by default)."""
    return sim.enable_battery(n_steps, interval_s, params=_dev(params), soc=_dev(soc0), **kw)


def _identities(raw):
    """[4] - [5] == [1] - [0] + [6] - [7], columns 4-7 and 9 >= 0, a key iff the cell has an ok second."""
    from tmhpvsim_amd import battery
    np.testing.assert_array_equal(raw[:, 4] - raw[:, 5], raw[:, 1] - raw[:, 0] + raw[:, 6] - raw[:, 7])
    assert (raw[:, 4:8] >= 0).all() and (raw[:, 9] >= 0).all()
    np.testing.assert_array_equal(battery.unpack_soc(raw[:, 8])[1] >= 0, raw[:, 2] > 0)


def _soc_changes(raw, soc0, end):
    """[6] - [7] - [9] is each interval's change of the state of charge, from soc0 to the state after the run."""
    from tmhpvsim_amd import battery
    soc, off = battery.unpack_soc(raw[:, 8])
    prev = np.asarray(soc0, dtype=np.int64).copy()
    for k in range(raw.shape[0]):
        now = np.where(off[k] >= 0, soc[k], prev)
        np.testing.assert_array_equal(raw[k, 6] - raw[k, 7] - raw[k, 9], now - prev, err_msg=f"interval {k}")
        prev = now
    np.testing.assert_array_equal(prev, end)


@functools.lru_cache(maxsize=None)
def a_want():
    """The expected table and end state of input A with the recipe's batteries, from the storage tests' traces."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    want, end = battery.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, soc0=SOC0)
    return want, end


@functools.lru_cache(maxsize=None)
def a_bt():
    """The battery sim of input A, one tmh_run per window of A_WINDOWS."""
    sim = _sim(A_N, A_START, **_kw60())
    assert sim.path == "time_parallel"
    raw = _enable(sim, A_STEPS, IV)
    assert tuple(raw.shape) == (13, 10, A_N) and tuple(sim.soc.shape) == (A_N,) and sim.soc.dtype == torch.int64
    assert tuple(sim.battery_params.shape) == (6, A_N)
    variants, guards = _run_windows(sim, A_WINDOWS)
    return dict(raw=_np(raw), soc=_np(sim.soc), variants=variants, guards=guards, status=sim.status())


def test_battery_equals_the_traces_table():
    """The main test: all ten columns and the state of charge bit for bit, over two windows (the second off the
    four-step grid), chains faulted at construction and inside the window, night and day, per-chain batteries
    that fill and empty partway, refuse charges when full and lose their standby drain down to empty."""
    from tmhpvsim_amd import _lib
    g, t = a_bt(), a60_gpu()
    want, end = a_want()
    a_has_teeth(t["pv"], t["cov"], g["status"])
    ev = events(t["pv"], t["meter"], t["cov"], PARAMS, SOC0)
    dead = g["status"] == 1
    print(ev, "dead at construction", int(dead.sum()), "in-window faults", int(((t["cov"][-1] == 255) & ~dead).sum()))
    assert ev["partial_fill"] >= 20000 and ev["partial_empty"] >= 100000 and ev["refused"] >= 50000
    assert ev["loss_chains"] >= 500 and ev["standby_clip"] > 0
    assert g["variants"] == [_lib.OUT_BATTERY | _lib.OUT_FP64] * len(A_WINDOWS)
    assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(10):
        np.testing.assert_array_equal(g["raw"][:, col], want[:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(g["soc"], end)
    assert dead.any() and not g["raw"][:, :, dead].any() and (g["soc"][dead] == SOC0[dead]).all()
    _identities(g["raw"])
    _soc_changes(g["raw"], SOC0, g["soc"])
    assert int((g["raw"][:, 9].sum(axis=0) > 0).sum()) >= 500
    assert g["raw"][12, 2].max() == 3 and g["raw"][:12, 2].max() == IV          # the last partial interval


def test_windows_pipelining_and_compaction_same_bits():
    """One tmh_run per window (a_bt), one pipelined run over windows of 4,000 steps, and compacted windows
    of 3,601 steps (from the second window on only the live chains run, in dense slots: a slot's work column
    is the slot's; its soc, its table column and its parameters are the chain's, ids[slot]): the same bits."""
    g = a_bt()
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
    for row in range(6):                                          # parameters indexed by slot would be other chains'
        assert (PARAMS[row, ids] != PARAMS[row, :len(ids)]).any()
    np.testing.assert_array_equal(_np(raw), g["raw"])
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    np.testing.assert_array_equal(sim.status(), g["status"])


@pytest.mark.parametrize("interval_s", [7, 128])
@pytest.mark.parametrize("n", [1300, 64])
def test_battery_boundaries(n, interval_s):
    """Boundaries inside four-second groups (7) and one per 128-s block (128); the origin three steps before
    the run, so no interval edge coincides with a window edge; a partial wavefront and construction faults;
    the recipe's first n batteries (tiled past A_N), which fill after sunrise."""
    from tmhpvsim_amd import _lib, battery
    pv, meter, cov = c60_traces(n)
    reps = -(-n // A_N)
    par, soc0 = np.tile(PARAMS, (1, reps))[:, :n], np.tile(SOC0, reps)[:n]
    ev = events(pv, meter, cov, par, soc0)
    print(f"n {n}: {ev}, construction faults {int((cov[0] == 255).sum())}")
    assert ev["partial_fill"] > 0 and ev["partial_empty"] > 0 and ev["refused"] > 0 and ev["standby_clip"] > 0
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    sim = _sim(n, C_START, **_kw60(C_STEPS))
    raw = _enable(sim, C_STEPS + C_LEAD, interval_s, par, soc0, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) == _lib.OUT_BATTERY | _lib.OUT_FP64
    torch.cuda.synchronize()
    want, end = battery.from_traces(pv, meter, cov, interval_s, origin=C_LEAD, params=par, soc0=soc0)
    assert tuple(raw.shape) == want.shape == (-(-(C_STEPS + C_LEAD) // interval_s), 10, n)
    for w0 in np.cumsum((0,) + C_WINDOWS)[:-1]:                   # where a window begins (and the one before it ends)
        assert (int(w0) + C_LEAD) % interval_s != 0
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    _identities(_np(raw))
    _soc_changes(_np(raw), soc0, _np(sim.soc))
    live0 = want[0, 2] == interval_s - C_LEAD                     # the first cell begins at offset C_LEAD
    assert live0.any()
    np.testing.assert_array_equal(battery.unpack_soc(_np(raw)[0, 8, live0])[1], interval_s - 1)


def test_lossless_equals_storage():
    """Uniform batteries with ec = ed = 1 and no standby drain, given in Wh and W: columns 0-8 and soc are an
    enable_storage sim's bit for bit (the existing kernels as a second reference), column 9 is 0."""
    from tmhpvsim_amd import _lib
    st = _sim(A_N, A_START, **_kw60())
    rs = st.enable_storage(A_STEPS, IV, **A_BATTERY)
    _run_windows(st, A_WINDOWS)
    assert _last(st) == _lib.OUT_STORAGE | _lib.OUT_FP64
    sim = _sim(A_N, A_START, **_kw60())
    raw = sim.enable_battery(A_STEPS, IV, charge_eff=1.0, discharge_eff=1.0, standby_w=0.0, **A_BATTERY)
    bat = storage_battery(A_BATTERY)
    np.testing.assert_array_equal(_np(sim.battery_params), uniform(A_N, bat["capacity"], bat["p_charge"], bat["p_discharge"]))
    assert (_np(sim.soc) == bat["soc0"]).all()
    _run_windows(sim, A_WINDOWS)
    assert _last(sim) == _lib.OUT_BATTERY | _lib.OUT_FP64
    got = _np(raw)
    np.testing.assert_array_equal(got[:, :9], _np(rs))
    np.testing.assert_array_equal(got[:, :9], a60_gpu()["want"])
    np.testing.assert_array_equal(_np(sim.soc), _np(st.soc))
    assert not got[:, 9].any() and int(got[:, 6].sum()) > 0 and int(got[:, 7].sum()) > 0


def test_two_batches_fill_one_table():
    """Chains [5000, 5500) and [5500, 6000) as two sims writing column slices of one table, reading slices of
    one [6, 1000] params tensor and carrying slices of one soc."""
    want, end = a_want()
    big = torch.zeros(13, 10, A_N, dtype=torch.int64, device="cuda:0")
    params, soc = _dev(PARAMS), _dev(SOC0)
    for a, b in ((0, 500), (500, A_N)):
        s = _sim(b - a, A_START, prec=PREC, chain0=A_CHAIN0 + a, mp=modules_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_battery(A_STEPS, IV, buffer=view, soc=soc[a:b], params=params[:, a:b])
        assert got is view and s._battery.ld == A_N and s.soc.data_ptr() == soc[a:b].data_ptr()
        assert s.battery_params.data_ptr() == params[:, a:b].data_ptr()
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), want)
    np.testing.assert_array_equal(_np(soc), end)
    np.testing.assert_array_equal(_np(params), PARAMS)                                     # read only
    with pytest.raises(ValueError, match="strides"):
        s.enable_battery(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2], params=params[:, 500:])  # chains not contiguous
    with pytest.raises(ValueError, match="battery buffer"):
        s.enable_battery(A_STEPS, IV, buffer=torch.zeros(13, 9, s.n, dtype=torch.int64, device="cuda:0"),
                         params=params[:, 500:])
    with pytest.raises(ValueError, match="row stride"):                                    # params of another width than the table
        s.enable_battery(A_STEPS, IV, params=params[:, 500:])
    with pytest.raises(ValueError, match="params"):
        s.enable_battery(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, :2 * s.n:2])
    with pytest.raises(ValueError, match="soc"):
        s.enable_battery(A_STEPS, IV, buffer=big[:, :, 500:], params=params[:, 500:], soc=soc[:2 * s.n:2])
    s.enable_battery(None)
    assert s.soc is None and s.battery_raw is None and s.battery_params is None


def test_battery_per_chain_sites(spec="default"):
    """The per-chain-sites kernels (map and replay), with statistics beside the table."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib, battery
    import dataclasses
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    mp = dataclasses.replace(modules_params(), cc_mode=ModelParams().cc_mode, seed=0x51E)
    sim = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    raw = _enable(sim, steps + 1, 450, par, soc0, step0=-1)
    stats = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    for s in (sim, stats):
        s.enable_stats(**HISTS[spec])
    stats.run(steps, trace=(), window=1700)
    assert _last(stats) & 7 == _lib.OUT_STATS
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_BATTERY | _lib.OUT_SITES | _lib.OUT_FP64
    tr = _sim(n, start, prec=PREC, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    want, end = battery.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1, params=par, soc0=soc0)
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    assert int(want[:, 6].sum()) > 0 and int(want[:, 7].sum()) > 0 and int(want[:, 9].sum()) > 0
    assert int(stats.hist.sum()) == int(raw[:, 2].sum()) > 0
    assert torch.equal(sim.hist, stats.hist)
    assert torch.equal(sim.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))


@pytest.mark.parametrize("spec", ["default", "huge"])
def test_statistics_unperturbed_by_the_battery(spec):
    """Statistics beside the battery table are the statistics-only run's, bit for bit (the map pass adds
    nothing to them), and the table is the battery-only one."""
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
    assert _last(both) == _lib.OUT_BATTERY | _lib.OUT_FP64 and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and torch.equal(both.soc, alone.soc) and int(ra[:, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    assert int(ra[:, 6].sum()) > 0 and int(ra[:, 7].sum()) > 0 and int(ra[:, 9].sum()) > 0
    _identities(_np(ra))


def test_soc_above_capacity_is_clamped():
    """A caller-owned soc above C (and below 0) is clamped at the first read: the result is from_traces' of the
    same start, which is the run from a full (an empty) battery."""
    from tmhpvsim_amd import battery
    t = a60_gpu()
    soc0 = PARAMS[0] + 12345
    soc0[::3] = -5
    want, end = battery.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, soc0=soc0)
    full, fend = battery.from_traces(t["pv"], t["meter"], t["cov"], IV, params=PARAMS, soc0=np.clip(soc0, 0, PARAMS[0]))
    np.testing.assert_array_equal(want, full)
    sim = _sim(A_N, A_START, **_kw60())
    raw = _enable(sim, A_STEPS, IV, soc0=soc0)
    sim.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(raw), want)
    np.testing.assert_array_equal(_np(sim.soc), end)
    dead = sim.status() == 1                                   # never ran an ok second, yet read and clamped
    assert dead.any() and (_np(sim.soc)[dead] == np.clip(soc0, 0, PARAMS[0])[dead]).all()
    assert ((_np(sim.soc) >= 0) & (_np(sim.soc) <= PARAMS[0])).all()


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message naming "battery" before anything is launched: the
    chains' state and the batteries' stay as they were and the table all zeros."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"
    par, soc0 = PARAMS[:, :n], SOC0[:n]
    BAT = dict(capacity_wh=0.5, charge_w=1000.0, discharge_w=3000.0, charge_eff=0.95, discharge_eff=0.9, standby_w=1.0,
               soc0_wh=0.25)

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before, soc = sim.state.clone(), sim.soc.clone()
        ws = sim.workspace(k)
        tr = trace or _lib.Trace(None, None, None, None, None, sim.n)
        ij = C.byref(inj) if inj is not None else None
        torch.cuda.synchronize()
        rc = L.tmh_run(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr), None,
                       C.c_void_p(ws.data_ptr()), ws.numel(), None)
        msg = L.tmh_last_error().decode()
        assert rc == -1 and match in msg and "battery" in msg, (rc, msg)
        pb = L.tmh_plan_bytes(k)                      # the halves refuse alike; a walk of the window too (it has no traces)
        plan, scr = C.c_void_p(ws.data_ptr()), C.c_void_p(ws.data_ptr() + pb)
        assert L.tmh_expand(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, ij, C.byref(tr),
                            None, plan, scr, ws.numel() - pb, None) == -1
        if sim.path == "time_parallel" and trace is None:
            assert L.tmh_walk(sim._eng, C.c_void_p(sim.state.data_ptr()), sim.chain0, sim.n, step0, k, plan, scr,
                              ws.numel() - pb, None) == -1
        torch.cuda.synchronize()
        assert torch.equal(before, sim.state) and torch.equal(soc, sim.soc)
        assert not bool(sim.battery_raw.any())

    def desc(sim, **kw):
        """The sim's tmh_battery with fields replaced."""
        d = sim._battery_desc
        f = dict(table=d.table, soc=d.soc, work=d.work, work_bytes=d.work_bytes, params=d.params)
        return _lib.Battery(**{**f, **kw})

    sim = _sim(n, start, prec=PREC, horizon=1000)
    _enable(sim, 500, 60, par, soc0)
    out = torch.zeros(100, n, dtype=torch.float64, device="cuda:0")
    refused(sim, "battery tables are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    ser = sim.enable_series(500)                                           # battery, then a fleet series
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    sim.enable_battery(None)
    sim.enable_series(500)                                                 # a fleet series, then battery
    with pytest.raises(ValueError, match="fleet series"):
        _enable(sim, 500, 60, par, soc0)
    sim.enable_series(None)
    _enable(sim, 500, 60, par, soc0)
    refused(sim, "outside the battery", step0=0, k=501)                    # past the end
    refused(sim, "outside the battery", step0=450, k=100)
    _enable(sim, 500, 60, par, soc0, step0=10)
    refused(sim, "outside the battery", step0=0, k=100)                    # before the origin
    buf = _enable(sim, 500, 60, par, soc0)
    _lib.check(L.tmh_set_battery(sim._eng, C.byref(desc(sim, table=_lib.Intervals(buf.data_ptr(), 0, 500, 60, n - 1)))))
    refused(sim, "battery tables ld")                                      # ld too small
    _lib.check(L.tmh_set_battery(sim._eng, C.byref(desc(sim, work_bytes=L.tmh_storage_work_bytes(n, 100) - 8))))
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
                     (dict(params=None), b"params"), (dict(params=sim.battery_params.data_ptr() + 4), b"params")):
        assert L.tmh_set_battery(sim._eng, C.byref(desc(sim, **kw))) == -1 and word in L.tmh_last_error()
        assert b"battery" in L.tmh_last_error()                            # the setter refuses a bad struct
    # the battery kind with another table kind on one engine, storage included, set in either order
    _enable(sim, 500, 60, par, soc0)
    for kind, cols, word in (("intervals", 4, "the battery kind and interval metering"),
                             ("registers", 6, "the battery kind and the import / export registers"),
                             ("demand", 8, "the battery kind and the demand registers"),
                             ("storage", 9, "the battery kind and battery storage")):
        other = torch.zeros(9, cols, n, dtype=torch.int64, device="cuda:0")
        tbl = _lib.Intervals(other.data_ptr(), 0, 500, 60, n)
        d = sim._battery_desc
        arg = _lib.Storage(tbl, d.soc, d.work, d.work_bytes, 100, 5, 5) if kind == "storage" else tbl
        setter = getattr(L, "tmh_set_" + kind)
        _lib.check(setter(sim._eng, C.byref(arg)))
        refused(sim, word)
        _lib.check(L.tmh_set_battery(sim._eng, None))
        _lib.check(L.tmh_set_battery(sim._eng, C.byref(sim._battery_desc)))   # (now battery after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
        with pytest.raises(ValueError, match="the battery kind"):
            getattr(sim, "enable_" + kind)(500, 60, **(A_BATTERY if kind == "storage" else {}))
        o = _sim(64, start, prec=PREC, horizon=1000)
        getattr(o, "enable_" + kind)(500, 60, **(A_BATTERY if kind == "storage" else {}))
        with pytest.raises(ValueError, match="one table output per sim"):
            o.enable_battery(500, 60, **BAT)
    seq = _sim(64, start, prec=PREC, horizon=1000, kernel_path="sequential")   # the sequential path
    seq.enable_battery(500, 60, **BAT)
    refused(seq, "battery tables need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), precision=PREC, device="cuda:0",
                      injected=inj, horizon=1000)
    isim.enable_battery(500, 60, **BAT)
    refused(isim, "time-parallel", inj=isim._us)
    mp = ModelParams()
    mp.inverter = dict(mp.inverter, Paco=float(L.tmh_series_max_w()))      # Paco >= TMH_SERIES_MAX_W
    big = _sim(64, start, prec=PREC, mp=mp, horizon=1000)
    big.enable_battery(500, 60, **BAT)
    refused(big, "TMH_SERIES_MAX_W")
    # fp32 engines: refused at the setter and at enable_battery
    f32 = _sim(64, start, prec="fp32", horizon=1000)
    with pytest.raises(ValueError, match="fp64"):
        f32.enable_battery(500, 60, **BAT)
    assert L.tmh_set_battery(f32._eng, C.byref(sim._battery_desc)) == -1
    assert b"fp64" in L.tmh_last_error() and b"battery" in L.tmh_last_error()
    # the Python layer refuses values outside their ranges before upload, and a soc0 outside [0, C]
    for bad in (dict(capacity_wh=1e9), dict(charge_w=-1.0), dict(charge_eff=0.4), dict(discharge_eff=1.1),
                dict(standby_w=-1.0), dict(soc0_wh=0.6), dict(soc0_wh=-0.1), dict(capacity_wh=[0.5] * 7)):
        with pytest.raises(ValueError):
            sim.enable_battery(500, 60, **{**BAT, **bad})
    worse = par.copy()
    worse[3, 5] = 70000
    with pytest.raises(ValueError, match="eff_charge"):
        sim.enable_battery(500, 60, params=_dev(worse))
    with pytest.raises(ValueError, match="required"):
        sim.enable_battery(500, 60)

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_battery(500, 60, **BAT)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the battery"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.battery_raw.any())
    assert bool((sim.soc == QUARTER_WH).all())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.battery_raw)
    assert int(raw[0, 2].min()) >= 0 and int(raw[:2, 2].sum()) > 0
    assert not raw[2:].any()
    _identities(raw)
    _soc_changes(raw, np.full(n, QUARTER_WH), _np(sim.soc))
    assert L.tmh_set_battery(sim._eng, None) == 0                          # NULL: off


def test_battery_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd import battery
    from tmhpvsim_amd.cli import TABLE_CSV, main
    f, z = tmp_path / "bt.csv", tmp_path / "bt.npz"
    r = CliRunner().invoke(main, ["battery", str(f), "--batch", "64", "--seconds", "1800", "--interval", "600",
                                  "--no-realtime", "--capacity-wh", "0.5,0,0.25", "--charge-w", "1000", "--discharge-w",
                                  "3000,1500", "--charge-eff", "0.95", "--discharge-eff", "0.9,1.0", "--standby-w", "2",
                                  "--soc0-wh", "0.25,0,0.25", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "import_wh", "export_wh", "pv_wh", "meter_wh", "charge_wh", "discharge_wh", "soc_wh",
                       "loss_wh", "n_ok"] and len(rows) == 1 + 3
    assert rows[0][1:] == [name for name, _ in TABLE_CSV["battery"]]
    saved = np.load(z)
    assert saved["raw"].shape == (3, 10, 64) and int(saved["interval_s"]) == 600
    _identities(saved["raw"])
    want = battery.to_watts(saved["raw"][:, :, :1], 600, n_steps=1800)       # column 0: chain 0
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00"]
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][k, 0]) for _, key in TABLE_CSV["battery"]]
    assert float(rows[1][3]) > 0 and float(rows[1][9]) == 600 and float(rows[1][6]) > 0   # noon: produces, discharges
    assert float(rows[1][8]) > 0                                                          # ... and loses
    full = battery.to_watts(saved["raw"], 600, n_steps=1800)
    for key in full:
        np.testing.assert_array_equal(saved[key], full[key], err_msg=key)
    none = np.arange(64) % 3 == 1                                            # the list dealt round-robin: no battery
    assert not saved["raw"][:, 7, none].any() and np.nanmax(full["soc_wh"][:, none]) == 0
    assert np.nanmax(full["soc_wh"][:, ~none]) > 0
    r = CliRunner().invoke(main, ["battery", str(f), "--batch", "4", "--no-realtime"])
    assert r.exit_code != 0 and "capacity-wh" in r.output
    r = CliRunner().invoke(main, ["battery", str(f), "--batch", "4", "--no-realtime", "--capacity-wh", "1", "--charge-w", "1",
                                  "--discharge-w", "1", "--charge-eff", "0.3"])
    assert r.exit_code != 0 and "eff_charge" in r.output
