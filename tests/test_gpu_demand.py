"""The demand registers on the GPU (tmh_set_demand, BatchedSim.enable_demand): integer sums
and integer maxima, so every comparison with the traces' table (demand.from_traces) is bit
for bit.  The expected table always comes from traces of separate sims of the same chains
(pv / meter / residual through OUT_TRACE3, covered through OUT_ANY), never from the code
under test."""
import ctypes as C
import csv
import functools

import numpy as np
import pytest

from series_util import A_CHAIN0, A_N, A_START, A_STEPS, A_TZ, A_WINDOWS, a_has_teeth, a_params
from test_gpu_registers import (C_LEAD, C_START, C_STEPS, C_WINDOWS, _export_seconds, _identity, _kw, _run_windows,
                                big_params, c_traces)
from test_gpu_series import _last, _np, _sim, _traces, a_gpu

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

IV = 900


def _keys_sane(raw, interval_s):
    """A key in both peak columns iff the cell has an ok second; offsets inside the interval; peak x n_ok >= the sum."""
    from tmhpvsim_amd import demand
    for col, reg in ((6, 4), (7, 5)):
        v, o = demand.unpack(raw[:, col])
        np.testing.assert_array_equal(raw[:, col] != 0, raw[:, 2] > 0)
        assert (o < interval_s).all() and (v * raw[:, 2] >= raw[:, reg]).all()


@functools.lru_cache(maxsize=None)
def a_dm(prec):
    """Input A with the demand registers, once per precision: the table over the windows A_WINDOWS
    (900-s intervals), the expected table from the traces of the same chains (test_gpu_series.a_gpu:
    separate sims), the registers table of another sim."""
    from tmhpvsim_amd import demand
    sim = _sim(A_N, A_START, **_kw(prec))
    assert sim.path == "time_parallel"
    raw = sim.enable_demand(A_STEPS, IV)
    assert tuple(raw.shape) == (13, 8, A_N)
    variants, guards = _run_windows(sim, A_WINDOWS)
    rgs = _sim(A_N, A_START, **_kw(prec))
    rg = rgs.enable_registers(A_STEPS, IV)
    _run_windows(rgs, A_WINDOWS)
    g = a_gpu(prec)
    want = demand.from_traces(g["pv"], g["meter"], g["cov"], IV)
    return dict(raw=_np(raw), want=want, rg=_np(rg), guards=guards, variants=variants, status=sim.status())


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_demand_equals_the_traces_table(prec):
    """The main test: all eight columns bit for bit, over two windows (the second off the four-step
    grid), chains faulted at construction and inside the window, night and day."""
    from tmhpvsim_amd import _lib, demand
    g, t = a_dm(prec), a_gpu(prec)
    a_has_teeth(t["pv"], t["cov"], t["status"])
    assert g["variants"] == [_lib.OUT_DEMAND | t["fp64"]] * len(A_WINDOWS)
    if prec == "fp32":   # the windows hold seconds the fixup replaced
        assert max(g["guards"]) > 0, g["guards"]
    else:
        assert g["guards"] == [0] * len(A_WINDOWS)
    for col in range(8):
        np.testing.assert_array_equal(g["raw"][:, col], g["want"][:, col], err_msg=f"column {col}")
    np.testing.assert_array_equal(g["raw"][:, :6], g["rg"])          # the table enable_registers gives
    _identity(g["raw"])
    _keys_sane(g["raw"], IV)
    pe = demand.unpack(g["raw"][:, 7])[0]
    assert (pe > 0).any() and ((pe == 0) & (g["raw"][:, 2] > 0)).any()   # cells with feed-in and cells without
    assert not g["raw"][:, :, t["status"] == 1].any()                    # dead at construction: no key either
    np.testing.assert_array_equal(g["status"], t["status"])


@functools.lru_cache(maxsize=None)
def big_want7():
    from tmhpvsim_amd import demand
    kw = _kw("fp32", mp=big_params())
    pv, meter, cov = _traces((_sim(A_N, A_START, **kw), _sim(A_N, A_START, **kw)), A_WINDOWS)
    return demand.from_traces(pv, meter, cov, 7), _export_seconds(pv, meter, cov)


def test_peaks_on_held_seconds():
    """fp32, 32 modules, 7-second cells: a held second (DISC's kt band at mid irradiance) is its
    cell's peak about one time in seven, so the fixup's maxima decide many cells, and pieces
    whose ok seconds are all held occur: windows of one tmh_run each, then one pipelined run.
    (A build without the fixup's two maxima fails this test.)"""
    want, export_s = big_want7()
    assert export_s >= 100000
    sim = _sim(A_N, A_START, **_kw("fp32", mp=big_params()))
    raw = sim.enable_demand(A_STEPS, 7)
    _, guards = _run_windows(sim, A_WINDOWS)
    assert max(guards) > 0, guards
    got = _np(raw)
    diff = got != want
    print(f"guard records {guards}; cells differing from the traces' table: {int(diff[:, 6].sum())} peak import, "
          f"{int(diff[:, 7].sum())} peak export, {int(diff[:, :6].sum())} in the sums")
    np.testing.assert_array_equal(got, want)
    _identity(got)
    _keys_sane(got, 7)
    pipe = _sim(A_N, A_START, **_kw("fp32", mp=big_params()))
    rawp = pipe.enable_demand(A_STEPS, 7)
    pipe.run(A_STEPS, trace=(), window=4000)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(rawp), want)


@pytest.mark.parametrize("prec", ["fp32", "fp64"])
@pytest.mark.parametrize("interval_s", [7, 60, 128, 900])
@pytest.mark.parametrize("n", [1300, 64])
def test_demand_boundaries(n, interval_s, prec):
    """Boundaries inside four-second groups (7), several in a 128-s block (60), one per block
    (128), partial first and last intervals (900); the origin three steps before the run, so no
    interval edge coincides with a window edge; a partial wavefront and construction faults."""
    from tmhpvsim_amd import _lib, demand
    pv, meter, cov = c_traces(n, prec)
    assert (np.nan_to_num(pv).max(axis=1) == 0).any() and (np.nan_to_num(pv) > 0).any()   # night and daylight
    if n > 1000:
        assert (cov[0] == 255).any()                                                       # construction faults
    assert _export_seconds(pv, meter, cov) >= (600 if n > 1000 else 25)
    sim = _sim(n, C_START, **_kw(prec, C_STEPS))
    raw = sim.enable_demand(C_STEPS + C_LEAD, interval_s, step0=-C_LEAD)
    for w in C_WINDOWS:
        sim.run(w, trace=(), window=w)
        assert _last(sim) & 7 == _lib.OUT_DEMAND
    torch.cuda.synchronize()
    want = demand.from_traces(pv, meter, cov, interval_s, origin=C_LEAD)
    assert tuple(raw.shape) == want.shape == (-(-(C_STEPS + C_LEAD) // interval_s), 8, n)
    for w0 in np.cumsum((0,) + C_WINDOWS)[:-1]:                   # where a window begins (and the one before it ends)
        assert (int(w0) + C_LEAD) % interval_s != 0
    np.testing.assert_array_equal(_np(raw), want)
    _identity(_np(raw))
    _keys_sane(_np(raw), interval_s)
    live0 = want[0, 2] > 0                                        # the first cell begins at offset C_LEAD
    np.testing.assert_array_equal(demand.unpack(_np(raw)[0, 7, live0])[1].min(), C_LEAD)


def test_demand_compacted_windows_same_bits():
    """compact=True: from the second window on only the live chains run, in dense slots; a
    slot's column is its chain's (ids[slot]), so the table is the uncompacted one."""
    g, t = a_dm("fp32"), a_gpu("fp32")
    a_has_teeth(t["pv"], t["cov"], t["status"])
    sim = _sim(A_N, A_START, **_kw("fp32"))
    raw = sim.enable_demand(A_STEPS, IV)
    sim.run(A_STEPS, trace=(), window=3601, compact=True)
    torch.cuda.synchronize()
    assert len(sim.compact_slots) == 3 and sim.compact_slots[0] == A_N
    assert min(sim.compact_slots) < A_N, sim.compact_slots        # a window ran on fewer slots than chains
    assert sim.compact_slots[2] < sim.compact_slots[1]            # (A's in-window faults)
    np.testing.assert_array_equal(_np(raw), g["raw"])
    np.testing.assert_array_equal(_np(raw), g["want"])
    np.testing.assert_array_equal(sim.status(), g["status"])


@pytest.mark.parametrize("spec", ["default", "offset", "huge"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_statistics_unperturbed_by_the_demand_registers(prec, spec):
    """Statistics beside the demand registers are the statistics-only run's, bit for bit, and the
    table is the demand-only one.  `offset` and `huge` are histogram specs the fp32 kernels bin
    in fp64 (the OUT_DEMAND | OUT_B64 instantiations)."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib
    n, start, steps = 600, "2019-09-05 09:00:00", 1500
    kw = _kw(prec, steps)
    both, stats, dm = _sim(n, start, **kw), _sim(n, start, **kw), _sim(n, start, **kw)
    both.enable_stats(**HISTS[spec])
    stats.enable_stats(**HISTS[spec])
    ra, rc = both.enable_demand(steps, 600), dm.enable_demand(steps, 600)
    for s in (both, stats, dm):
        s.run(steps, trace=(), window=1000)
    torch.cuda.synchronize()
    assert _last(both) & 7 == _lib.OUT_DEMAND and _last(stats) & 7 == _lib.OUT_STATS
    assert int(stats.hist.sum()) > 0 and float(stats.chain_acc[0].sum()) > 0
    assert torch.equal(both.hist, stats.hist)
    assert torch.equal(both.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))
    assert torch.equal(ra, rc) and int(ra[:, 2].sum()) > 0
    assert int(both.hist.sum()) == int(ra[:, 2].sum())
    _identity(_np(ra))
    _keys_sane(_np(ra), 600)


@pytest.mark.parametrize("spec", ["default", "huge"])
@pytest.mark.parametrize("prec", ["fp32", "fp64"])
def test_demand_per_chain_sites(prec, spec):
    """The per-chain-sites kernels, with statistics beside the table: `huge` is a histogram
    spec that the fp32 kernel bins in fp64 (its OUT_B64 instantiation)."""
    from test_gpu_trace3 import HISTS
    from tmhpvsim_amd import _lib, demand
    from tmhpvsim_amd.params import ModelParams, site_grid
    n, steps, start = 512, 3000, "2019-06-21 04:45:00"
    sites = site_grid(32, 16)
    mp = ModelParams(seed=0x51E)
    sim = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    raw = sim.enable_demand(steps + 1, 450, step0=-1)
    stats = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    for s in (sim, stats):
        s.enable_stats(**HISTS[spec])
    stats.run(steps, trace=(), window=1700)
    assert _last(stats) & 7 == _lib.OUT_STATS
    sim.run(steps, trace=(), window=1700)
    assert _last(sim) == _lib.OUT_DEMAND | _lib.OUT_SITES | (_lib.OUT_FP64 if prec == "fp64" else 0)
    tr = _sim(n, start, prec=prec, mp=mp, horizon=steps, sites=sites)
    out = tr.run(steps, trace=("covered", "pv", "meter"))
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(raw), demand.from_traces(out["pv"], out["meter"], out["covered"], 450, origin=1))
    assert int(stats.hist.sum()) == int(raw[:, 2].sum()) > 0
    assert torch.equal(sim.hist, stats.hist)
    assert torch.equal(sim.chain_acc.view(torch.int64), stats.chain_acc.view(torch.int64))


def test_two_batches_fill_one_table():
    """Chains [5000, 5512) and [5512, 6000) as two sims writing column slices of one buffer."""
    big = torch.zeros(13, 8, A_N, dtype=torch.int64, device="cuda:0")
    for a, b in ((0, 512), (512, A_N)):
        s = _sim(b - a, A_START, prec="fp32", chain0=A_CHAIN0 + a, mp=a_params(), horizon=A_STEPS)
        view = big[:, :, a:b]
        got = s.enable_demand(A_STEPS, IV, buffer=view)
        assert got is view and s._demand.ld == A_N
        s.run(A_STEPS, trace=())
    torch.cuda.synchronize()
    np.testing.assert_array_equal(_np(big), a_dm("fp32")["raw"])
    with pytest.raises(ValueError, match="strides"):
        s.enable_demand(A_STEPS, IV, buffer=big[:, :, :2 * s.n:2])     # chains not contiguous
    with pytest.raises(ValueError, match="demand buffer"):
        s.enable_demand(A_STEPS, IV, buffer=torch.zeros(13, 6, s.n, dtype=torch.int64, device="cuda:0"))
    s.enable_demand(None)


def test_every_refusal():
    """Each case is refused with TMH_E_INVAL and a message before anything is launched: the
    chains' state stays as it was and the table all zeros."""
    from tmhpvsim_amd import _lib
    from tmhpvsim_amd.engine import BatchedSim
    from tmhpvsim_amd.params import RNG_INJECTED, ModelParams
    L = _lib.load()
    n, start = 600, "2019-09-05 09:00:00"

    def refused(sim, match, step0=0, k=100, trace=None, inj=None):
        before = sim.state.clone()
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
        assert torch.equal(before, sim.state)
        assert not bool(sim.demand_raw.any())

    sim = _sim(n, start, horizon=1000)
    sim.enable_demand(500, 60)
    out = torch.zeros(100, n, dtype=torch.float32, device="cuda:0")
    refused(sim, "demand registers are set: no traces", trace=_lib.Trace(None, None, out.data_ptr(), None, None, n))
    assert not bool(out.any())
    sim.enable_demand(None)
    ser = sim.enable_series(500)                                           # a fleet series, then the demand registers
    with pytest.raises(ValueError, match="fleet series"):
        sim.enable_demand(500, 60)
    buf = torch.zeros(9, 8, n, dtype=torch.int64, device="cuda:0")
    sim.demand_raw = buf
    _lib.check(L.tmh_set_demand(sim._eng, C.byref(_lib.Demand(buf.data_ptr(), 0, 500, 60, n))))
    refused(sim, "fleet series")
    sim.enable_series(None)
    _lib.check(L.tmh_set_demand(sim._eng, None))
    sim.demand_raw = None
    sim.enable_demand(500, 60)                                             # the demand registers, then a fleet series
    ser = sim.enable_series(500)
    refused(sim, "fleet series")
    assert not bool(ser.any())
    with pytest.raises(ValueError, match="fleet series"):
        sim.run(100, trace=())
    sim.enable_series(None)
    refused(sim, "outside the demand", step0=0, k=501)                     # past the end
    refused(sim, "outside the demand", step0=450, k=100)
    sim.enable_demand(500, 60, step0=10)
    refused(sim, "outside the demand", step0=0, k=100)                     # before the origin
    buf = sim.enable_demand(500, 60)
    small = _lib.Demand(buf.data_ptr(), 0, 500, 60, n - 1)                 # ld too small
    _lib.check(L.tmh_set_demand(sim._eng, C.byref(small)))
    refused(sim, "demand registers ld")
    for bad, word in ((_lib.Demand(buf.data_ptr() + 4, 0, 500, 60, n), b"8-byte aligned"),
                      (_lib.Demand(None, 0, 500, 60, n), b"buffer"), (_lib.Demand(buf.data_ptr(), 0, 500, 0, n), b"interval_s"),
                      (_lib.Demand(buf.data_ptr(), 0, 0, 60, n), b"n_steps"), (_lib.Demand(buf.data_ptr(), 0, 500, 60, 0), b"ld")):
        assert L.tmh_set_demand(sim._eng, C.byref(bad)) == -1 and word in L.tmh_last_error()   # the setter refuses a bad struct
        assert b"demand" in L.tmh_last_error()
    # the demand registers with intervals or with registers on one engine, set in either order
    sim.enable_demand(500, 60)
    ivbuf = torch.zeros(9, 4, n, dtype=torch.int64, device="cuda:0")
    rgbuf = torch.zeros(9, 6, n, dtype=torch.int64, device="cuda:0")
    ivs, rgs = _lib.Intervals(ivbuf.data_ptr(), 0, 500, 60, n), _lib.Registers(rgbuf.data_ptr(), 0, 500, 60, n)
    for setter, st, other, word in ((L.tmh_set_intervals, ivs, ivbuf, "demand registers and interval metering"),
                                    (L.tmh_set_registers, rgs, rgbuf, "demand registers and the import / export registers")):
        _lib.check(setter(sim._eng, C.byref(st)))
        refused(sim, word)
        _lib.check(L.tmh_set_demand(sim._eng, None))
        _lib.check(L.tmh_set_demand(sim._eng, C.byref(sim._demand)))       # (now the demand registers after the other)
        refused(sim, word)
        assert not bool(other.any())
        _lib.check(setter(sim._eng, None))
    with pytest.raises(ValueError, match="demand"):
        sim.enable_intervals(500, 60)
    with pytest.raises(ValueError, match="demand"):
        sim.enable_registers(500, 60)
    for enable, word in (("enable_intervals", "interval metering"), ("enable_registers", "registers")):
        other = _sim(64, start, horizon=1000)
        getattr(other, enable)(500, 60)
        with pytest.raises(ValueError, match=word):
            other.enable_demand(500, 60)
    seq = _sim(64, start, horizon=1000, kernel_path="sequential")          # the sequential path
    seq.enable_demand(500, 60)
    refused(seq, "demand registers need the time-parallel")
    inj = torch.rand(64, 4096, dtype=torch.float64, device="cuda:0")       # injected uniforms
    isim = BatchedSim(64, start, tz=A_TZ, params=ModelParams(rng_mode=RNG_INJECTED), device="cuda:0", injected=inj,
                      horizon=1000)
    isim.enable_demand(500, 60)
    refused(isim, "time-parallel", inj=isim._us)
    for key, val in (("Paco", float(L.tmh_series_max_w())), ("Pnt", float(L.tmh_series_max_w()))):
        mp = ModelParams()
        mp.inverter = dict(mp.inverter, **{key: val})                      # Paco, |Pnt| >= TMH_SERIES_MAX_W
        big = _sim(64, start, mp=mp, horizon=1000)
        big.enable_demand(500, 60)
        refused(big, "TMH_SERIES_MAX_W")

    # BatchedSim refuses before its first launch what a multi-window run would meet half way
    sim.enable_demand(500, 60)
    before = sim.state.clone()
    with pytest.raises(ValueError, match="trace"):
        sim.run(200, trace=("pv",), window=100)
    with pytest.raises(ValueError, match="outside the demand"):
        sim.run(600, trace=(), window=200)
    torch.cuda.synchronize()
    assert torch.equal(before, sim.state) and sim.step == 0 and not bool(sim.demand_raw.any())
    sim.run(100, trace=())                                                 # after all refusals the sim still runs
    torch.cuda.synchronize()
    raw = _np(sim.demand_raw)
    assert int(raw[0, 2].min()) >= 0 and int(raw[:2, 2].sum()) > 0
    assert not raw[2:].any()
    _identity(raw)
    _keys_sane(raw, 60)
    assert L.tmh_set_demand(sim._eng, None) == 0                           # NULL: off


def test_demand_cli(tmp_path):
    from click.testing import CliRunner
    from tmhpvsim_amd import demand
    from tmhpvsim_amd.cli import main
    f, z = tmp_path / "dm.csv", tmp_path / "dm.npz"
    r = CliRunner().invoke(main, ["demand", str(f), "--batch", "64", "--seconds", "1800", "--interval", "600",
                                  "--no-realtime", "--all-chains", str(z)])
    assert r.exit_code == 0, r.output
    rows = list(csv.reader(open(f)))
    assert rows[0] == ["time", "import_wh", "export_wh", "pv_wh", "meter_wh", "self_wh", "n_ok", "peak_import_w",
                       "t_peak_import_s", "peak_export_w", "t_peak_export_s"] and len(rows) == 1 + 3
    saved = np.load(z)
    assert saved["raw"].shape == (3, 8, 64) and int(saved["interval_s"]) == 600
    _identity(saved["raw"])
    _keys_sane(saved["raw"], 600)
    want = demand.to_watts(saved["raw"][:, :, :1], 600, n_steps=1800)       # column 0: chain 0
    assert [row[0] for row in rows[1:]] == ["2019-09-06 12:00:00", "2019-09-06 12:10:00", "2019-09-06 12:20:00"]
    keys = ("energy_wh_import", "energy_wh_export", "energy_wh_pv", "energy_wh_meter", "energy_wh_self", "n_ok",
            "peak_import", "t_peak_import", "peak_export", "t_peak_export")
    for k, row in enumerate(rows[1:]):
        assert [float(x) for x in row[1:]] == [float(want[key][k, 0]) for key in keys]
    assert float(rows[1][3]) > 0 and float(rows[1][6]) == 600 and float(rows[1][7]) > 0   # noon: chain 0 produces and draws
    full = demand.to_watts(saved["raw"], 600, n_steps=1800)
    for key in full:
        np.testing.assert_array_equal(saved[key], full[key])
